"""Runs the table of tests/flow_flag_cases.py (the Gaussian window, flags 256, and the initial flow, flags 4) through
relax_optical_flow_flags on the GPU and writes profiles/flow_flags_parity.json, the file tests/test_gpu_flow_flags.py takes its parity gate from:
  flow_vs_reference_fp32   per gated case and per edge case of gauss_solve_any's tile, the GPU flow's distance from
                           tests/flow_flag_ref.farneback_flags (same parameters) in float64 in units of the float32 reference's own distance -
                           the larger of the mean and the max ratio; the mean ratio alone where the case id ends in -mean - and the worst of them
The reference is the stated formulas in numpy, not an OpenCV build.
Usage: python tools/flow_flags_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_flags_parity.json"))
    args = ap.parse_args()
    import torch
    import relax_vqa_amd  # noqa: F401
    from tests import flow_cases as fc
    from tests import test_gpu_flow_flags as t

    ratios = t.measure_ratios()
    for k, v in ratios.items():
        print(f"ratio {k}: {v:.3f}", flush=True)
    out = {
        "device": torch.cuda.get_device_name(0),
        "flow_vs_reference_fp32": {"worst_ratio": max(ratios.values()), "cap": fc.PARITY_CAP, "cases": ratios},
        "reference": "tests/flow_flag_ref.farneback_flags in float64 (the stated formulas; no OpenCV build)",
        "rule": "gate = the next power of two above worst_ratio, capped; a ratio above the cap is a bug",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
