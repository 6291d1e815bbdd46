"""ResNet-50 on canvases other than 224 x 224 on the MI355X (relax_resnet50_set_canvas, csrc/resnet50.hip, csrc/conv1_x6.hip), synthetic
weights under the default arithmetic (f16x2) and bf16x6, device events after a warm-up, median of 7 with [min, max]:

  - 224 x 224 x 256 images through resnet50_features_canvas and through resnet50_features, alternating in the same run, each with its
    run-to-run spread: the canvas on the handle must cost the default case nothing (same launches, same bits);
  - 448 x 448 x 256 images against FOUR passes of 224 x 224 x 256 (the same pixels): how the tiles fill at 112 x 112 / 56 x 56 / 28 x 28 maps
    was not known; the ratio is a finding, not a target;
  - 288 x 512 x 128 images (the whole-frame canvas of 16:9 video);
  - the stem alone, from one `rocprofv3 --kernel-trace --stats` child per precision run before this process opens the GPU: conv1_x6 at
    224 x 224 (the kernel compiled for that size) and conv1_x6_canvas at 448 x 448 (the 16 x 16-tile kernel), per output pixel.  The two
    kernels cannot be timed on the SAME canvas: 224 x 224 always runs the compiled geometry and nothing forces the other one there.

  python tools/resnet_canvas_bench.py [--reps 7] [--out profiles/resnet_canvas_bench.json]

Synthetic weights (synth.resnet50_state_dict) and random inputs: the timing does not depend on the values."""
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


FAULT_STATUS = (134, 139, 124, 137, -6, -11, -9)


def trace_step(precision):
    """the rocprofv3 target: two layer-stack passes of 64 images at 224 x 224 and at 448 x 448 in one precision"""
    eng = RelaxEngine(0)
    eng.load_resnet50(synth.resnet50_state_dict())
    eng.set_precision(precision)
    g = np.random.default_rng(0)
    for side in (224, 448):
        x = torch.from_numpy(g.integers(0, 256, (64, side, side, 3), dtype=np.uint8)).cuda()
        for _ in range(2):
            eng.resnet50_features_canvas(x, pool=False)
    torch.cuda.synchronize()


def stem_kernels(precision):
    """-> per stem kernel (conv1_x6: compiled for 224 x 224; conv1_x6_canvas: 16 x 16 tiles, here at 448 x 448) calls, average microseconds
    and nanoseconds per output pixel, from one kernel trace in a child of its own"""
    d = tempfile.mkdtemp(prefix="resnet_canvas_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace-step", precision]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"resnet_canvas_bench: the trace child ({precision}) ran into its time limit")
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if res.returncode in FAULT_STATUS:   # a fault, an abort or a time limit on the card: nothing more is started on it
        raise SystemExit(f"resnet_canvas_bench: the trace child ({precision}) ended with status {res.returncode}: {res.stderr[-300:]}")
    if res.returncode != 0 or not files:
        return {"not_measured": f"rocprofv3 rc {res.returncode}: {res.stderr[-300:]}"}
    out = {}
    for r in csv.DictReader(open(files[0])):
        if "conv1_x6" not in r["Name"] or "repack" in r["Name"]:
            continue
        canvas = "conv1_x6_canvas" in r["Name"]
        pixels = 64 * (224 * 224 if canvas else 112 * 112)
        out["conv1_x6_canvas at 448x448" if canvas else "conv1_x6 at 224x224"] = {
            "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "images": 64,
            "ns_per_output_pixel": round(float(r["AverageNs"]) / pixels, 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-step", default=None, metavar="PRECISION")
    args = ap.parse_args()
    if args.trace_step:
        return trace_step(args.trace_step)
    # children first: this process has not opened the GPU yet
    stems = {p: ({"not_measured": "--no-trace"} if args.no_trace else stem_kernels(p)) for p in ("f16x2", "bf16x6")}
    if not torch.cuda.is_available():
        raise SystemExit("resnet_canvas_bench: no GPU - nothing is measured without one")
    eng = RelaxEngine(0)
    eng.load_resnet50(synth.resnet50_state_dict())
    g = np.random.default_rng(0)
    n = args.images
    x224 = torch.from_numpy(g.integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)).cuda()
    x448 = torch.from_numpy(g.integers(0, 256, (n, 448, 448, 3), dtype=np.uint8)).cuda()
    x288 = torch.from_numpy(g.integers(0, 256, (n // 2, 288, 512, 3), dtype=np.uint8)).cuda()
    out = {"model": "resnet50", "reps": args.reps, "precisions": {}}
    for precision in ("f16x2", "bf16x6"):
        eng.set_precision(precision)
        rec = {}
        both = _time_alternating({"resnet50_features_canvas": lambda: eng.resnet50_features_canvas(x224),
                                  "resnet50_features": lambda: eng.resnet50_features(x224)}, args.reps)
        a, b = eng.resnet50_features_canvas(x224), eng.resnet50_features(x224)
        both["images_per_batch"] = n
        both["canvas_over_features_pct"] = round(100.0 * (both["resnet50_features_canvas"]["ms_median"] / both["resnet50_features"]["ms_median"] - 1.0), 2)
        both["bit_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        rec["224x224_methods"] = both
        four = _time_alternating({"448x448": lambda: eng.resnet50_features_canvas(x448),
                                  "4 x 224x224": lambda: [eng.resnet50_features(x224) for _ in range(4)]}, args.reps)
        four["images_per_batch"] = n
        four["ratio_448_over_four_224"] = round(four["448x448"]["ms_median"] / four["4 x 224x224"]["ms_median"], 4)
        four["ms_per_image_448"] = round(four["448x448"]["ms_median"] / n, 4)
        rec["448x448_against_four_224x224"] = four
        wide = _time_alternating({"288x512": lambda: eng.resnet50_features_canvas(x288)}, args.reps)["288x512"]
        rec["288x512"] = {"images_per_batch": n // 2, "pass": wide, "ms_per_image": round(wide["ms_median"] / (n // 2), 4),
                          "ms_per_image_224x224": round(both["resnet50_features"]["ms_median"] / n, 4),
                          "pixels_over_224x224": round(288 * 512 / (224 * 224), 3)}
        rec["stem"] = stems[precision]
        out["precisions"][precision] = rec
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
