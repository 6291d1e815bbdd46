"""Runs the table of tests/flow_param_space.py through relax_optical_flow_ex on the GPU and writes profiles/flow_param_space_parity.json:
  cases   per case, the GPU flow's distance from oracle/flow_ref.farneback (same six parameters) in float64 in units of the float32 oracle's
          own distance - the mean and the max ratio -, the restated route (flow_param_space.route_word) and the pyramid levels used
  worst_ratio   the largest of the gated cases' ratios
The file is a record: tests/test_gpu_flow_param_space.py takes its gate from profiles/flow_params_parity.json.
Usage: python tools/flow_param_space_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_param_space_parity.json"))
    args = ap.parse_args()
    import torch
    import relax_vqa_amd  # noqa: F401
    from tests import flow_cases as fc
    from tests import flow_param_cases as pc
    from tests import flow_param_space as sp
    from tests import test_gpu_flow_param_space as t

    cases = t.measure()
    for k, v in cases.items():
        print(f"ratio {k}: mean {v['mean_ratio']:.3f} max {v['max_ratio']:.3f}" + (" (bits only)" if v["bits_only"] else ""), flush=True)
    gated = [max(v["mean_ratio"], v["max_ratio"]) for v in cases.values() if not v["bits_only"]]
    out = {
        "device": torch.cuda.get_device_name(0),
        "flow_vs_oracle_fp32": {"worst_ratio": max(gated), "gate": pc.parity_gate(), "cap": fc.PARITY_CAP, "cases": cases},
        "bits_only": {sp.case_id(c): why for c, why in sp.BITS_ONLY.items()},
        "rule": "a record, not a gate: the gate is profiles/flow_params_parity.json's; a ratio above it is a finding about csrc/flow.hip",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
