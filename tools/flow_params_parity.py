"""Runs the parameter sets of tests/flow_param_cases.py through relax_optical_flow_ex on the GPU and writes
profiles/flow_params_parity.json, the file tests/test_gpu_flow_params.py takes its parity gate from:
  flow_vs_oracle_fp32   per gated case, the GPU flow's distance from oracle/flow_ref.farneback (same six parameters) in float64 in units
                        of the float32 oracle's own distance - the larger of the mean and the max ratio; the mean ratio alone for the
                        sets of flow_param_cases.MEAN_ONLY - and the worst of them
Usage: python tools/flow_params_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_params_parity.json"))
    args = ap.parse_args()
    import torch
    import relax_vqa_amd  # noqa: F401
    from tests import flow_cases as fc
    from tests import flow_param_cases as pc
    from tests import test_gpu_flow_params as t

    ratios = t.measure_ratios()
    for k, v in ratios.items():
        print(f"ratio {k}: {v:.3f}", flush=True)
    out = {
        "device": torch.cuda.get_device_name(0),
        "flow_vs_oracle_fp32": {"worst_ratio": max(ratios.values()), "cap": fc.PARITY_CAP, "cases": ratios},
        "mean_term_only": list(pc.MEAN_ONLY),
        "ungated": list(pc.UNGATED),
        "rule": "gate = the next power of two above worst_ratio, capped; a ratio above the cap is a bug",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
