"""Measures the parity ratios of the f16x2 streaming attention (csrc/attention_stream_h2.hip) on the GPU and writes
profiles/attention_stream_h2_parity.json, the file tests/test_gpu_attention_stream_h2.py takes its gates from:
  operator_vs_torch_cpu_fp32  the kernel's distance from fp64 in units of torch-CPU fp32's own distance, over the operator cases
  model_vs_bf16x6_route       ViT-B tokens / pooled rows / CLS attention: distance from the CPU restatement under "att_h2_stream" 1 over the
                              distance under 0 (the bf16x6 streaming route)
Usage: python tools/attention_stream_h2_parity.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_stream_h2_parity.json"))
    args = ap.parse_args()
    import torch
    import relax_vqa_amd  # noqa: F401
    from tests import test_gpu_attention_stream_h2 as t
    from tests.gpu_common import engine

    eng = engine()
    before = eng.get_option("att_h2_stream")
    op = t.measure_operator()
    for k, v in op.items():
        print(f"operator {k}: {v:.3f}", flush=True)
    model = t.measure_model()
    for k, v in model.items():
        print(f"model {k}: {v:.3f}", flush=True)
    eng.set_option("att_h2_stream", before)
    eng.set_option("att_h2", 1)
    out = {
        "device": torch.cuda.get_device_name(0),
        "kernel": "attention_stream_h2 (key tile %d, %d queries per item)" % (t.TILE, t.QBLOCK),
        "operator_vs_torch_cpu_fp32": {"worst_ratio": max(op.values()), "cap": t.cases.PARITY_CAP, "cases": op},
        "model_vs_bf16x6_route": {"worst_ratio": max(model.values()), "cap": t.MODEL_CAP, "cases": model},
        "rule": "gate = the next power of two above worst_ratio, capped; a ratio above the cap is a bug",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
