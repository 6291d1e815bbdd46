"""Writes profiles/stream_handoffs.json: per scenario of tests/test_gpu_stream_handoffs.py the warm host time, the hold, how many
candidates beside() probed, whether the run was vacuous, whether it passed, and whether the variant with the ordering removed was caught -
tests/test_gpu_stream_handoffs.measure(), through the functions the tests call.

    python tools/stream_handoffs_profile.py [out.json]
"""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from tests import test_gpu_stream_handoffs as handoffs
    with tempfile.TemporaryDirectory() as tmp:
        out = handoffs.measure(pathlib.Path(tmp))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    bad = {k: v for k, v in out["scenarios"].items() if "error" in v or not v.get("passed") or v.get("broken_variant_caught") is False}
    print(f"{len(out['scenarios'])} scenarios in {out['wall_s']} s, {len(bad)} not passing" + (f", stopped at {out['stopped_at']}" if out["stopped_at"] else ""))
    for k, v in bad.items():
        print(" ", k, v)
    return 1 if bad or out["stopped_at"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_handoffs.json")))
