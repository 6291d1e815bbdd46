"""Writes profiles/stream_contract.json: the hold calibration, every case's warm host time and hold, what the held-stream and the
capture runs saw, and the covered / captured / exempt lists - tests/test_gpu_stream_contract.measure(), through the helpers the tests call.

    python tools/stream_contract_profile.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from tests import test_gpu_stream_contract as contract
    out = contract.measure()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    bad = {k: v for k, v in out["cases"].items() if "error" in v or not v.get("bits_equal") or (v["kind"] == "enqueue" and not v.get("still_held"))}
    print(f"{len(out['cases'])} runs in {out['wall_s']} s, {len(bad)} not passing" + (f", stopped at {out['stopped_at']}" if out["stopped_at"] else ""))
    for k, v in bad.items():
        print(" ", k, v)
    return 1 if bad or out["stopped_at"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_contract.json")))
