"""The ViT on canvases other than 224 x 224 on the MI355X (relax_vit_features_canvas, csrc/vit.hip), ViT-B/16 under f16x2 and fp32, device
events after a warm-up, median of 7:

  - ms per batch at 224 x 224 through relax_vit_features_canvas and through relax_vit_features, alternating in the same run, each with its
    run-to-run spread ((max - min) / median over the repeats): the canvas argument must cost the 224 case nothing;
  - ms per batch and per image at 448 x 448 (785 tokens), 270 x 480 (481) and 540 x 960 (1981);
  - attention's share of the GPU time of a pass at each size: one `rocprofv3 --kernel-trace --stats` child per precision and size (two
    passes of a quarter batch each), run before this process opens the GPU; the kernels whose names contain "attention";
  - the cost of a position table: relax_vit_pos_embed on a cache miss (host taps, hipMalloc, two small copies, vit_pos_interp, a stream
    wait; host clock around a synchronised call, every call a grid the four-entry cache does not hold) and on a hit (a device copy).

  python tools/vit_canvas_bench.py [--reps 7] [--no-trace] [--out profiles/vit_canvas_bench.json]

Synthetic weights (synth.vit_state_dict) and random inputs: the timing does not depend on the values."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

DIM = 768
FAULT_STATUS = (134, 139, 124, 137, -6, -11, -9)
# (label, Hc, Wc, images per batch)
SIZES = [("224x224", 224, 224, 256), ("448x448", 448, 448, 64), ("270x480", 270, 480, 128), ("540x960", 540, 960, 32)]


def _engine():
    eng = RelaxEngine(0)
    eng.load_vit(synth.vit_state_dict("vit_base"), "vit_base")
    return eng


def trace_step(precision, label):
    """the rocprofv3 target: two pooled passes of a quarter batch at one size in one precision"""
    Hc, Wc, n = next((h, w, n) for lab, h, w, n in SIZES if lab == label)
    eng = _engine()
    eng.set_precision(precision)
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (max(n // 4, 1), Hc, Wc, 3), dtype=np.uint8)).cuda()
    for _ in range(2):
        eng.vit_features(x, tokens=False, pooled=True)
    torch.cuda.synchronize()


def attention_share(precision, label):
    """-> the attention kernels' percent of the traced GPU time of trace_step's two passes (the loader's weight conversions left out), per
    kernel and summed; one kernel trace in a child of its own"""
    d = tempfile.mkdtemp(prefix="vit_canvas_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace-step", precision, label]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"vit_canvas_bench: the trace child ({precision}, {label}) ran into its time limit")
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if res.returncode in FAULT_STATUS:   # a fault, an abort or a time limit on the card: nothing more is started on it
        raise SystemExit(f"vit_canvas_bench: the trace child ({precision}, {label}) ended with status {res.returncode}: {res.stderr[-300:]}")
    if res.returncode != 0 or not files:
        return {"not_measured": f"rocprofv3 rc {res.returncode}: {res.stderr[-300:]}"}
    rows = list(csv.DictReader(open(files[0])))
    load = ("to_sp3", "to_h2", "permute")           # the loader's conversion kernels are not part of a pass
    rows = [r for r in rows if not any(k in r["Name"] for k in load)]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"traced_ms": round(total / 1e6, 2), "passes": 2, "attention_pct": 0.0, "kernels": {}}
    for r in rows:
        if "attention" in r["Name"]:
            short = r["Name"].split("(")[0].replace("void relax::", "")
            pct = 100.0 * float(r["TotalDurationNs"]) / total
            out["kernels"][short] = {"pct": round(pct, 2), "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 1)}
            out["attention_pct"] = round(out["attention_pct"] + pct, 2)
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


def _time(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return _stats([_event_ms(fn) for _ in range(reps)])


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
    ap.add_argument("--trace-step", nargs=2, default=None, metavar=("PRECISION", "SIZE"))
    args = ap.parse_args()
    if args.trace_step:
        return trace_step(*args.trace_step)
    shares = {}
    if not args.no_trace:   # children first: this process has not opened the GPU yet
        shares = {p: {label: attention_share(p, label) for label, _, _, _ in SIZES} for p in ("f16x2", "fp32")}
    if not torch.cuda.is_available():
        raise SystemExit("vit_canvas_bench: no GPU - nothing is measured without one")
    eng = _engine()
    g = np.random.default_rng(0)
    out = {"model": "vit_base/16", "reps": args.reps, "precisions": {}}
    images = {label: torch.from_numpy(g.integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)).cuda() for label, Hc, Wc, n in SIZES}
    for precision in ("f16x2", "fp32"):
        eng.set_precision(precision)
        rec = {}
        # 224 x 224: the new entry point beside the old one
        f224 = images["224x224"]
        n224 = f224.shape[0]
        pooled_new = torch.empty((n224, 3 * DIM), dtype=torch.float32, device="cuda")
        pooled_old = torch.empty_like(pooled_new)

        def via_canvas():
            eng._check(eng.lib.relax_vit_features_canvas(eng.h, f224.data_ptr(), n224, 224, 224, None, pooled_new.data_ptr(), None, None),
                       "relax_vit_features_canvas")

        def via_features():
            eng._check(eng.lib.relax_vit_features(eng.h, f224.data_ptr(), n224, None, pooled_old.data_ptr(), None), "relax_vit_features")

        both = _time_alternating({"relax_vit_features_canvas": via_canvas, "relax_vit_features": via_features}, args.reps)
        both["images_per_batch"] = n224
        both["canvas_over_features_pct"] = round(100.0 * (both["relax_vit_features_canvas"]["ms_median"] /
                                                           both["relax_vit_features"]["ms_median"] - 1.0), 2)
        both["bit_equal"] = bool(torch.equal(pooled_new, pooled_old))
        rec["224x224_entry_points"] = both
        # every size: the pooled pass
        sizes = {}
        for label, Hc, Wc, n in SIZES:
            x = images[label]
            gh, gw, ntok = (14, 14, 197) if label == "224x224" else eng.vit_canvas_geometry(Hc, Wc)
            t = _time(lambda: eng.vit_features(x, tokens=False, pooled=True), args.reps)
            sizes[label] = {"grid": [gh, gw], "tokens": ntok, "images_per_batch": n, "pass": t,
                            "ms_per_image": round(t["ms_median"] / n, 4),
                            "us_per_token": round(1e3 * t["ms_median"] / (n * ntok), 4),
                            "attention_share": shares.get(precision, {}).get(label, {"not_measured": "--no-trace"})}
        rec["sizes"] = sizes
        out["precisions"][precision] = rec
    # the position table: every call of `miss` asks for a grid the four-entry cache does not hold
    pos = {}
    for label, (gh, gw) in (("28x28", (28, 28)), ("16x30", (16, 30)), ("33x60", (33, 60)), ("64x64", (64, 64))):
        others = [(gh + 1 + k, gw) if (gh + 1 + k) * gw <= 4096 else (gh - 1 - k, gw) for k in range(5)]
        miss, hit = [], []
        for _ in range(args.reps):
            for o in others:                      # five other grids push (gh, gw) out of the cache
                eng.vit_pos_embed(*o)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.vit_pos_embed(gh, gw)
            torch.cuda.synchronize()
            miss.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            eng.vit_pos_embed(gh, gw)
            torch.cuda.synchronize()
            hit.append((time.perf_counter() - t0) * 1e3)
        pos[label] = {"table_bytes": (1 + gh * gw) * DIM * 4, "miss_host_ms": _stats(miss), "hit_host_ms": _stats(hit)}
    out["pos_embed"] = pos
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
