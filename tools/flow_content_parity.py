"""Runs the content-level optical-flow cases (tests/flow_cases.py) on the GPU and writes profiles/flow_content_parity.json, the file
tests/test_gpu_flow_content.py takes its parity gate from:
  flow_vs_oracle_fp32   per case, the GPU flow's distance from the oracle in float64 in units of the float32 oracle's own distance (the
                        larger of the mean and the max ratio), and the worst of them
  flow_to_rgb_explained per boundary field, how many pixels differ from the oracle's image and are explained by a truncation within 1e-3
                        of an integer (and how many are not: the test wants none)
Usage: python tools/flow_content_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_content_parity.json"))
    args = ap.parse_args()
    import torch
    import relax_vqa_amd  # noqa: F401
    from tests import flow_cases as fc
    from tests import test_gpu_flow_content as t

    ratios = t.measure_ratios()
    for k, v in ratios.items():
        print(f"ratio {k}: {v:.3f}", flush=True)
    fields = {}
    for name in t.FIELDS:
        explained, unexplained, got = t.measure_field(name)
        fields[name] = {"pixels": int(got[..., 0].size), "explained": explained, "unexplained": len(unexplained)}
        print(f"flow_to_rgb {name}: {fields[name]}", flush=True)
    out = {
        "device": torch.cuda.get_device_name(0),
        "flow_vs_oracle_fp32": {"worst_ratio": max(ratios.values()), "cap": fc.PARITY_CAP, "cases": ratios},
        "flow_to_rgb_explained": fields,
        "rule": "gate = the next power of two above worst_ratio, capped; a ratio above the cap is a bug",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
