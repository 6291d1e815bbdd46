"""DINO ViTs at patch size 8 (785 tokens, csrc/attention_stream.hip) on the MI355X -> profiles/vit_patch8_bench.json and
profiles/vit_patch8_parity.json, from ONE run.  Device events after a warm-up, the median of the repeats:

  - ms per 256 fragments of vit_features(pooled) for ViT-S/8 and ViT-B/8 under the default precision (f16x2) and under fp32, beside
    ViT-B/16 in the same run;
  - each attention kernel's share of a ViT-B/8 pass, from one rocprofv3 kernel trace taken in a child process of its own (before this
    process opens the GPU), per precision;
  - attention_stream_x6 and attention_stream_f32 alone at 256 images x 12 heads x 785 tokens in algorithmic TFLOP/s
    (4 ntok^2 64 FLOP per (image, head)), beside torch's fp32 scaled_dot_product_attention on the same tensors;
  - the parity record of tests/test_gpu_vit_patch8.py: the fp32 streaming kernel's distance from fp64 in units of torch-CPU fp32's own,
    on the test's 785-token cases.

  python tools/vit_patch8_bench.py [--batch 256] [--reps 7] [--no-trace]

Synthetic weights and random inputs: the timing does not depend on the values."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(torch, fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def _engine_with(name, patch):
    import relax_vqa_amd  # noqa: F401
    from relax_vqa_amd import synth
    from relax_vqa_amd.engine import RelaxEngine
    eng = RelaxEngine(0)
    eng.load_vit(synth.vit_state_dict(name, patch=patch), name)
    return eng


def trace_step(precision, batch):
    """the rocprofv3 target: three ViT-B/8 forwards in one precision"""
    import torch
    eng = _engine_with("vit_base", 8)
    eng.set_precision(precision)
    frags = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (batch, 224, 224, 3), dtype=np.uint8)).cuda()
    for _ in range(3):
        eng.vit_features(frags, tokens=False, pooled=True)
    torch.cuda.synchronize()


def kernel_shares(precision, batch):
    """-> {kernel name: percent of the traced GPU time} for the attention kernels, + the total; one kernel trace in a child of its own"""
    d = tempfile.mkdtemp(prefix="vit_patch8_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace-step", precision, "--batch", str(batch)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return {"not_measured": f"rocprofv3 rc {res.returncode}: {res.stderr[-300:]}"}
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"traced_ms": round(total / 1e6, 2), "batch": batch, "forwards": 3}
    for r in rows:
        if "attention" in r["Name"]:
            short = r["Name"].split("(")[0].replace("void relax::", "")
            out[short] = {"pct": round(100.0 * float(r["TotalDurationNs"]) / total, 2), "calls": int(r["Calls"]),
                          "avg_us": round(float(r["AverageNs"]) / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-step", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_patch8_bench.json"))
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "vit_patch8_parity.json"))
    args = ap.parse_args()
    if args.trace_step:
        return trace_step(args.trace_step, args.batch)

    out = {"batch": args.batch, "reps": args.reps, "timing": "device events, median of reps after 2 warm-up calls"}
    if not args.no_trace:   # children first: this process has not opened the GPU yet
        out["attention_share_vit_base_patch8"] = {p: kernel_shares(p, min(args.batch, 64)) for p in ("f16x2", "fp32")}

    import torch
    from tests import vit_patch8_cases as cases
    g = np.random.default_rng(0)
    frags = torch.from_numpy(g.integers(0, 256, (args.batch, 224, 224, 3), dtype=np.uint8)).cuda()
    scale = 256 / args.batch
    passes = {}
    for name, patch in (("vit_base", 16), ("vit_small", 8), ("vit_base", 8)):
        eng = _engine_with(name, patch)
        eng.reserve(args.batch)
        for prec in ("f16x2", "fp32"):
            eng.set_precision(prec)
            med, best = _time_ms(torch, lambda: eng.vit_features(frags, tokens=False, pooled=True), args.reps)
            passes[f"{name}/{patch} {prec}"] = {"ms_per_256_median": round(med * scale, 2), "ms_per_256_min": round(best * scale, 2)}
        del eng
        torch.cuda.empty_cache()
    out["ms_per_256_fragments"] = passes

    # the kernels alone: 256 images x 12 heads x 785 tokens
    n_img, heads, ntok = 256, 12, 785
    flop = 4.0 * ntok * ntok * 64 * n_img * heads
    qkv = torch.randn((n_img * ntok, 3 * heads * 64), device="cuda")
    eng = _engine_with("vit_tiny", 8)
    alone = {"shape": f"{n_img} images x {heads} heads x {ntok} tokens", "algorithmic_GFLOP": round(flop / 1e9, 1)}
    for prec, label in (("bf16x6", "attention_stream_x6"), ("fp32", "attention_stream_f32")):
        eng.set_precision(prec)
        med, best = _time_ms(torch, lambda: eng.op_attention_ex(qkv, n_img, ntok, heads), args.reps)
        alone[label] = {"ms_median": round(med, 3), "ms_min": round(best, 3), "TFLOPs_median": round(flop / (med * 1e-3) / 1e12, 2)}
    t = qkv.reshape(n_img, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = (x.contiguous() for x in (t[0], t[1], t[2]))
    med, best = _time_ms(torch, lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), args.reps)
    alone["torch_sdpa_fp32"] = {"ms_median": round(med, 3), "ms_min": round(best, 3), "TFLOPs_median": round(flop / (med * 1e-3) / 1e12, 2),
                                "note": "contiguous [B, heads, ntok, 64] inputs; the layout change is not timed"}
    out["attention_alone"] = alone
    del qkv, q, k, v, t

    # parity record: the gate of tests/test_gpu_vit_patch8.py is the next power of two above worst_ratio, capped at 8
    eng.set_precision("fp32")
    par = {}
    for ntok_, n_, h_ in [c for c in cases.CASES if c[0] == 785]:
        for s in cases.SCALES:
            x, ref64, cpu32 = cases.case(ntok_, n_, h_, s)
            par[f"{n_}x{h_} scale {s}"] = round(cases.parity_ratio(eng.op_attention_ex(x.cuda(), n_, ntok_, h_), ref64, cpu32), 4)
    parity = {"fp32_stream_vs_torch_cpu_fp32": {"ratios": par, "worst_ratio": max(par.values()), "cap": cases.PARITY_CAP,
                                                "definition": "max(mean |err| ratio, max |err| ratio) against fp64 on the CPU, ntok = 785"}}
    for path, obj in ((args.out, out), (args.parity_out, parity)):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(obj, indent=1) + "\n")
    print(json.dumps(out))
    print(json.dumps(parity))


if __name__ == "__main__":
    main()
