"""The resize to any output size (relax_resize_frames_ex, csrc/resize.hip) on the MI355X, timed with device events after a warm-up.

Per shape (540p, 1080p, 2160p; T = 32 frames, both filters), ms per call as median / min / max over --repeats repeats of --calls
back-to-back calls:
  to_224_entry       relax_resize_frames: the same kernels through the 224 entry
  to_224_ex          relax_resize_frames_ex at 224 x 224      - the two timed alternately, repeat by repeat
  to_quarter         relax_resize_frames_ex at H/4 x W/4
  to_448             relax_resize_frames_ex at 448 x 448
Next to each time: the bytes the call moves through HBM by its byte model (the frame read once; per filter the uint8 intermediate
[T,H,out_w,3] written and read, the output written) and the time those bytes take at the 6.29 TB/s copy rate.
`ex_over_entry` is the entry-overhead check of the two 224 forms (equal bytes asserted; one kernel family, so a ratio away from 1 by
more than `spread_ms`, the larger of their max - min spreads, is the entries' host work).

Then one whole_frame_vit_canvas pass (ViT-B/16, T frames at 1080p -> 270 x 480 = 481 tokens) beside its LANCZOS resize alone: the
resize's share of the pass.

  python tools/resize_any_bench.py [--frames 32] [--repeats 7] [--calls 5] [--no-vit] [--out profiles/resize_any_bench.json]

Synthetic weights and random frames: the timing does not depend on the values."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

COPY_TBPS = 6.29
SHAPES = (("540p", 540, 960), ("1080p", 1080, 1920), ("2160p", 2160, 3840))


def _timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _stats(ts):
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4), "ms_max": round(float(np.max(ts)), 4)}


def _time_ms(fns, repeats, calls, warmup=2):
    """fns: the forms timed ALTERNATELY (one repeat of each in turn) -> one record per form"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ts[k].append(_timed(fn, calls))
    return [_stats(t) for t in ts]


def _with_bytes(rec, nbytes):
    rec["MB_moved"] = round(nbytes / 1e6, 1)
    rec["ms_at_copy_rate"] = round(nbytes / (COPY_TBPS * 1e12) * 1e3, 4)
    rec["GBps_median"] = round(nbytes / (rec["ms_median"] * 1e-3) / 1e9, 1)
    rec["share_of_copy_rate"] = round(rec["ms_at_copy_rate"] / rec["ms_median"], 3)
    return rec


def resize_bytes(T, H, W, oh, ow, filters=2):
    passes = (0 if ow == W or oh == H else 2.0 * T * H * ow * 3) + float(T) * oh * ow * 3
    return float(T) * H * W * 3 + filters * passes


def resize_shapes(eng, args):
    out = {}
    for label, H, W in SHAPES:
        T = args.frames
        frames = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda")
        rec = {"T": T, "H": H, "W": W}

        def bufs(oh, ow):
            return [torch.empty((T, oh, ow, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]

        b224, n224 = bufs(224, 224), bufs(224, 224)
        entry, ex = _time_ms([lambda: eng.resize_frames(frames, out_bilinear=b224[0], out_lanczos=b224[1]),
                              lambda: eng.resize_frames_to(frames, (224, 224), out_bilinear=n224[0], out_lanczos=n224[1])],
                             args.repeats, args.calls)
        assert torch.equal(b224[0], n224[0]) and torch.equal(b224[1], n224[1]), "the two 224 forms differ"
        rec["to_224_entry"] = _with_bytes(entry, resize_bytes(T, H, W, 224, 224))
        rec["to_224_ex"] = _with_bytes(ex, resize_bytes(T, H, W, 224, 224))
        rec["spread_ms"] = round(max(r["ms_max"] - r["ms_min"] for r in (entry, ex)), 4)
        rec["ex_over_entry"] = round(ex["ms_median"] / entry["ms_median"], 3)
        for name, (oh, ow) in (("to_quarter", (H // 4, W // 4)), ("to_448", (448, 448))):
            ob = bufs(oh, ow)
            r, = _time_ms([lambda: eng.resize_frames_to(frames, (oh, ow), out_bilinear=ob[0], out_lanczos=ob[1])], args.repeats, args.calls)
            r["out_h"], r["out_w"] = oh, ow
            rec[name] = _with_bytes(r, resize_bytes(T, H, W, oh, ow))
        out[label] = rec
        print(label, json.dumps(rec), flush=True)
        del frames
        torch.cuda.empty_cache()
    return out


def vit_canvas_pass(eng, args):
    eng.load_vit(synth.vit_state_dict("vit_base"), "vit_base")
    T, H, W, size = args.frames, 1080, 1920, 270
    frames = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device="cuda")
    oh, ow = eng.resize_output_size(H, W, size)
    whole, = _time_ms([lambda: eng.whole_frame_vit_canvas(frames, size)], args.repeats, 1, warmup=2)
    lan = torch.empty((T, oh, ow, 3), dtype=torch.uint8, device="cuda")
    stage, = _time_ms([lambda: eng.resize_frames_to(frames, size, bilinear=False, out_lanczos=lan)], args.repeats, 1, warmup=2)
    out = {"T": T, "H": H, "W": W, "canvas": [oh, ow], "tokens": eng.vit_canvas_geometry(oh, ow)[2], "model": "vit_base", "precision": eng.precision(),
           "whole_pass": whole, "lanczos_resize": _with_bytes(stage, resize_bytes(T, H, W, oh, ow, filters=1)),
           "resize_share_pct": round(100.0 * stage["ms_median"] / whole["ms_median"], 1),
           "frames_per_s": round(T / (whole["ms_median"] * 1e-3), 1)}
    print("whole_frame_vit_canvas", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-vit", action="store_true")
    ap.add_argument("--out", default="profiles/resize_any_bench.json")
    args = ap.parse_args()
    eng = RelaxEngine(0)
    out = {"copy_rate_TBps": COPY_TBPS, "repeats": args.repeats, "calls_per_repeat": args.calls, "resize": resize_shapes(eng, args)}
    if not args.no_vit:
        out["whole_frame_vit_canvas"] = vit_canvas_pass(eng, args)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
