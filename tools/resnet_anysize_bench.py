"""ResNet-50 on canvases the default rule refuses (relax_resnet50_set_canvas_ex with RELAX_RN_CANVAS_ANY; csrc/conv1_x6.hip: conv1_x6_any,
csrc/layers.hip: bn_relu_maxpool_any) on the MI355X, synthetic weights under the default arithmetic (f16x2) and bf16x6, device events after a
warm-up, median of 7 with [min, max], one card, one session:

  - 270 x 480 x 128 images against 288 x 512 x 128, and 540 x 960 x 32 against 544 x 960 x 32, alternating in the same run: ms per image and
    ns per INPUT pixel of the odd canvas over its neighbouring multiple-of-32 canvas.  The odd canvases lose the back-to-back forms on some
    maps and the fused means; what that costs per pixel is a finding with its spread, not a gate;
  - the two stem forms (conv1_x6_canvas: whole 16 x 16 tiles; conv1_x6_any: partial tiles, rows at any alignment) and the two max-pool forms
    (bn_relu_maxpool_nhwc: even maps; bn_relu_maxpool_any: any map, a ragged last block per image) on a canvas both take, 288 x 512 x 64 images: one
    `rocprofv3 --kernel-trace --stats` child per form, each a run of its own started before this process opens the GPU.  The any-size forms
    run there only with RELAX_RN_FORCE_ANY_FORMS=1 in the child's environment (csrc/resnet50.hip; this tool is its only user).  Each child also
    writes a digest of its rows: the two forms must give the same bits.

  python tools/resnet_anysize_bench.py [--reps 7] [--out profiles/resnet_anysize_bench.json]

Synthetic weights (synth.resnet50_state_dict) and random inputs: the timing does not depend on the values.  Not measured here: canvases near
1024 x 1024, real checkpoints, more than one GPU."""
import argparse
import csv
import glob
import hashlib
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

PRECISIONS = ("f16x2", "bf16x6")
PAIRS = (((270, 480), (288, 512), 128), ((540, 960), (544, 960), 32))
FORM_CANVAS, FORM_IMAGES = (288, 512), 64
FAULT_STATUS = (134, 139, 124, 137, -6, -11, -9)


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


def trace_step(digest_path):
    """the rocprofv3 target: two passes of 64 images at 288 x 512 under the any-size rule in each precision (which stem and max-pool run there
    is the environment's RELAX_RN_FORCE_ANY_FORMS), and a digest of the rows"""
    eng = RelaxEngine(0)
    eng.load_resnet50(synth.resnet50_state_dict())
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (FORM_IMAGES,) + FORM_CANVAS + (3,), dtype=np.uint8)).cuda()
    digest = {}
    for precision in PRECISIONS:
        eng.set_precision(precision)
        for _ in range(2):
            ls, pool = eng.resnet50_features_canvas(x, any_size=True)
        torch.cuda.synchronize()
        digest[precision] = hashlib.sha256(ls.cpu().numpy().tobytes() + pool.cpu().numpy().tobytes()).hexdigest()
    with open(digest_path, "w") as f:
        json.dump(digest, f)


def form_kernels(force_any):
    """-> per precision the stem and max-pool kernels of one form at 288 x 512 (calls, average microseconds, ns per output pixel) and the rows'
    digests, from one kernel trace in a child of its own"""
    d = tempfile.mkdtemp(prefix="resnet_anysize_trace_")
    digest_path = os.path.join(d, "digest.json")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--trace-step", digest_path]
    env = dict(os.environ, RELAX_RN_FORCE_ANY_FORMS="1" if force_any else "0")
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"resnet_anysize_bench: the trace child (force_any={force_any}) ran into its time limit")
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if res.returncode in FAULT_STATUS:   # a fault, an abort or a time limit on the card: nothing more is started on it
        raise SystemExit(f"resnet_anysize_bench: the trace child (force_any={force_any}) ended with status {res.returncode}: {res.stderr[-300:]}")
    if res.returncode != 0 or not files or not os.path.exists(digest_path):
        return {"not_measured": f"rocprofv3 rc {res.returncode}: {res.stderr[-300:]}"}
    stem_pixels = FORM_IMAGES * (FORM_CANVAS[0] // 2) * (FORM_CANVAS[1] // 2)
    out = {"digest": json.load(open(digest_path)), "kernels": {}}
    for r in csv.DictReader(open(files[0])):
        name = r["Name"]
        stem = "conv1_x6" in name and "repack" not in name
        if not stem and "bn_relu_maxpool" not in name:
            continue
        pixels = stem_pixels if stem else stem_pixels // 4
        out["kernels"][name.split("(")[0].replace("void relax::", "")] = {
            "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "images": FORM_IMAGES,
            "ns_per_output_pixel": round(float(r["AverageNs"]) / pixels, 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-step", default=None, metavar="DIGEST_FILE")
    args = ap.parse_args()
    if args.trace_step:
        return trace_step(args.trace_step)
    # children first: this process has not opened the GPU yet
    forms = {"not_measured": "--no-trace"} if args.no_trace else {"tile_forms": form_kernels(False), "any_size_forms": form_kernels(True)}
    if not args.no_trace and all("digest" in v for v in forms.values()):
        forms["rows_bit_equal"] = forms["tile_forms"]["digest"] == forms["any_size_forms"]["digest"]
    if not torch.cuda.is_available():
        raise SystemExit("resnet_anysize_bench: no GPU - nothing is measured without one")
    eng = RelaxEngine(0)
    eng.load_resnet50(synth.resnet50_state_dict())
    g = np.random.default_rng(0)
    out = {"model": "resnet50", "reps": args.reps, "forms_at_288x512": forms, "precisions": {},
           "not_measured": ["canvases near 1024 x 1024", "real checkpoints", "more than one GPU"]}
    for precision in PRECISIONS:
        eng.set_precision(precision)
        rec = {}
        for odd, even, n in PAIRS:
            xo = torch.from_numpy(g.integers(0, 256, (n,) + odd + (3,), dtype=np.uint8)).cuda()
            xe = torch.from_numpy(g.integers(0, 256, (n,) + even + (3,), dtype=np.uint8)).cuda()
            ko, ke = "%dx%d" % odd, "%dx%d" % even
            t = _time_alternating({ko: lambda: eng.resnet50_features_canvas(xo, any_size=True), ke: lambda: eng.resnet50_features_canvas(xe)}, args.reps)
            per_px = {k: t[k]["ms_median"] * 1e6 / (n * hw[0] * hw[1]) for k, hw in ((ko, odd), (ke, even))}
            t.update(images_per_batch=n, ms_per_image={k: round(t[k]["ms_median"] / n, 4) for k in (ko, ke)},
                     ns_per_input_pixel={k: round(v, 4) for k, v in per_px.items()}, per_pixel_odd_over_even=round(per_px[ko] / per_px[ke], 4))
            rec[f"{ko} against {ke}"] = t
            del xo, xe
        out["precisions"][precision] = rec
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
