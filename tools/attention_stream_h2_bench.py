"""The f16x2 streaming attention (csrc/attention_stream_h2.hip) on the MI355X, beside the bf16x6 streaming route it replaces:

  - the kernel alone at 256 images x 12 heads x 785 tokens, beside attention_stream<X6> and attention_stream<F32> on the same tensor: one
    `rocprofv3 --kernel-trace` child (run before this process opens the GPU) that calls relax_op_attention_ex 2 + 7 times per
    arithmetic; each kernel's own duration per call, the two warm-up calls dropped, median of 7 and spread (the f16x2 operator entry's
    conversion kernels are separate rows of the trace and left out, which device events around the entry point could not do);
  - a pooled ViT-B/16 pass under f16x2 at 197 tokens (256 images), 785 (448 x 448, 64), 481 (270 x 480, 128) and 1981 (540 x 960, 32), and a
    pooled ViT-B/8 pass at 224 x 224 (785 tokens, 256 images): "att_h2_stream" 0 and 1 alternating in one process, device events after a
    warm-up, median of 7, each with its run-to-run spread ((max - min) / median);
  - the keep rule of the option's default: 1 only if the pass is faster with it by more than the larger of the two spreads at 785 AND at
    1981 tokens.

  python tools/attention_stream_h2_bench.py [--reps 7] [--no-trace] [--out profiles/attention_stream_h2_bench.json]

Synthetic weights (synth.vit_state_dict) and random inputs: the timing does not depend on the values."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

FAULT_STATUS = (134, 139, 124, 137, -6, -11, -9)
KERNEL_SHAPE = (256, 12, 785)      # images, heads, tokens
# (label, patch, Hc, Wc, images per batch)
PASSES = [("vit_base/16 224x224", 16, 224, 224, 256), ("vit_base/16 448x448", 16, 448, 448, 64), ("vit_base/16 270x480", 16, 270, 480, 128),
          ("vit_base/16 540x960", 16, 540, 960, 32), ("vit_base/8 224x224", 8, 224, 224, 256)]
TRACE_WARMUP, TRACE_REPS = 2, 7
KEEP_RULE_AT = ("vit_base/16 448x448", "vit_base/16 540x960")     # 785 and 1981 tokens


def trace_step():
    """the rocprofv3 target: relax_op_attention_ex on one tensor under fp32, bf16x6 and f16x2 with the option on"""
    n_img, heads, ntok = KERNEL_SHAPE
    eng = RelaxEngine(0)
    x = torch.randn((n_img * ntok, 3 * heads * 64), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    for precision, stream in (("fp32", 0), ("bf16x6", 0), ("f16x2", 1)):
        eng.set_precision(precision)
        eng.set_option("att_h2_stream", stream)
        for _ in range(TRACE_WARMUP + TRACE_REPS):
            eng.op_attention_ex(x, n_img, ntok, heads)
    torch.cuda.synchronize()


def kernel_times():
    """-> {kernel: median / min / max / spread of its own per-call durations} of the three attention kernels, from one kernel trace in a child"""
    d = tempfile.mkdtemp(prefix="att_stream_h2_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace-step"]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        raise SystemExit("attention_stream_h2_bench: the trace child ran into its time limit")
    if res.returncode in FAULT_STATUS:   # a fault, an abort or a time limit on the card: nothing more is started on it
        raise SystemExit(f"attention_stream_h2_bench: the trace child ended with status {res.returncode}: {res.stderr[-300:]}")
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if res.returncode != 0 or not files:
        return {"not_measured": f"rocprofv3 rc {res.returncode}: {res.stderr[-300:]}"}
    rows = list(csv.DictReader(open(files[0])))
    cols = {c.lower(): c for c in (rows[0].keys() if rows else [])}
    name_c, t0_c, t1_c = cols.get("kernel_name"), cols.get("start_timestamp"), cols.get("end_timestamp")
    if not (name_c and t0_c and t1_c):
        return {"not_measured": f"kernel trace columns {sorted(cols)[:12]}"}
    # per-call durations in dispatch order; the two warm-up calls of each kernel are dropped, the other TRACE_REPS give median and spread
    per = {}
    for r in sorted(rows, key=lambda r: int(r[t0_c])):
        name = r[name_c]
        if "attention_stream" not in name:
            continue
        short = ("attention_stream_h2" if "attention_stream_h2" in name else
                 "attention_stream_f32" if "attention_stream<0" in name.replace(" ", "") or "attention_streamILi0E" in name else "attention_stream_x6")
        per.setdefault(short, []).append((int(r[t1_c]) - int(r[t0_c])) / 1e6)
    out = {"images_heads_tokens": list(KERNEL_SHAPE), "source": "rocprofv3 --kernel-trace: each kernel's own duration per call (the f16x2 operator "
           "entry's conversion kernels are other rows); device events around relax_op_attention_ex would include them", "warmup_calls_dropped": TRACE_WARMUP}
    for short, ts in per.items():
        out[short] = {"calls_timed": len(ts) - TRACE_WARMUP, **_stats(ts[TRACE_WARMUP:])}
    if "attention_stream_h2" in out and "attention_stream_x6" in out:
        out["h2_over_x6"] = round(out["attention_stream_h2"]["ms_median"] / out["attention_stream_x6"]["ms_median"], 3)
    return out


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    med = float(np.median(ts))
    return {"ms_median": round(med, 3), "ms_min": round(float(np.min(ts)), 3), "ms_max": round(float(np.max(ts)), 3),
            "spread_pct": round(100.0 * (float(np.max(ts)) - float(np.min(ts))) / med, 2)}


def _time_alternating(fns, reps, warmup=2):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_event_ms(fn))
    return {k: _stats(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-step", action="store_true")
    args = ap.parse_args()
    if args.trace_step:
        return trace_step()
    kernel = {"not_measured": "--no-trace"} if args.no_trace else kernel_times()     # the child first: this process has not opened the GPU yet
    if not torch.cuda.is_available():
        raise SystemExit("attention_stream_h2_bench: no GPU - nothing is measured without one")
    eng = RelaxEngine(0)
    eng.set_precision("f16x2")
    g = np.random.default_rng(0)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "precision": "f16x2", "kernel_alone": kernel, "passes": {}}
    loaded = None
    for label, patch, Hc, Wc, n in PASSES:
        if loaded != patch:
            eng.load_vit(synth.vit_state_dict("vit_base", patch=patch), "vit_base")
            loaded = patch
        x = torch.from_numpy(g.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)).cuda()
        ntok = (Hc // patch) * (Wc // patch) + 1

        def run(stream):
            eng.set_option("att_h2_stream", stream)
            return eng.vit_features(x, tokens=False, pooled=True)[1]

        t = _time_alternating({"att_h2_stream=0": lambda: run(0), "att_h2_stream=1": lambda: run(1)}, args.reps)
        t0, t1 = t["att_h2_stream=0"], t["att_h2_stream=1"]
        gain = 100.0 * (1.0 - t1["ms_median"] / t0["ms_median"])
        spread = max(t0["spread_pct"], t1["spread_pct"])
        out["passes"][label] = {"tokens": ntok, "images_per_batch": n, **t, "gain_pct": round(gain, 2), "larger_spread_pct": spread,
                                "faster_beyond_spread": bool(gain > spread),
                                "bit_equal": bool(torch.equal(run(0), run(1)))}
        del x
    out["keep_rule"] = {"at": list(KEEP_RULE_AT), "default_1": bool(all(out["passes"][k]["faster_beyond_spread"] for k in KEEP_RULE_AT))}
    out["not_measured"] = ["real DINO checkpoints", "more than one GPU", "canvases near the 4096-patch limit (speed)"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
