"""The fused difference + resize (relax_resize_residual, csrc/resize.hip) on the MI355X, timed with device events after a warm-up.

Per shape (540p, 1080p, 2160p; T = 32 pairs), ms per call as median / min / max over --repeats repeats of --calls back-to-back calls:
  fused              relax_resize_residual, both filters, no residual output
  fused_residual     the same with the residual image written
  unfused_int16      the yardstick: (next.int16 - orig.int16).abs().uint8 in aten, then relax_resize_frames on the result
  unfused_minmax     the same yardstick with the cheaper aten difference, maximum(a, b) - minimum(a, b) on uint8
  resize_frames      relax_resize_frames alone on the T first frames
Next to each time: the bytes the form moves through HBM by its byte model, and the time those bytes take at the 6.29 TB/s copy rate.
`fused_not_slower` compares `fused` with the faster of the two yardsticks of the same run; the margin is the larger of the two
forms' max - min spreads.

Then one whole_residual_vectors pass over a config-4-shaped batch (--clips clips of 16 pairs at 540p, ResNet-50 + ViT-B) per
residual name, beside its input stage alone (difference + resize, or Farneback + resize): where the time of the ablation rows goes.

  python tools/whole_residual_bench.py [--pairs 32] [--repeats 7] [--calls 5] [--clips 16] [--no-vectors] [--out profiles/whole_residual_bench.json]

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


def _time_ms(fn, repeats, calls, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return {"ms_median": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4), "ms_max": round(float(np.max(ts)), 4)}


def _with_bytes(rec, nbytes):
    rec["MB_moved"] = round(nbytes / 1e6, 1)
    rec["ms_at_copy_rate"] = round(nbytes / (COPY_TBPS * 1e12) * 1e3, 4)
    rec["GBps_median"] = round(nbytes / (rec["ms_median"] * 1e-3) / 1e9, 1)
    return rec


def resize_shapes(eng, args):
    out = {}
    for label, H, W in SHAPES:
        T = args.pairs
        frames = torch.randint(0, 256, (T, 2, H, W, 3), dtype=torch.uint8, device="cuda")
        orig, nxt = frames[:, 0], frames[:, 1]
        bil, lan = (torch.empty((T, 224, 224, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
        frame = float(T) * H * W * 3
        # both filters: the uint8 intermediate [T,H,224,3] is written and read once per filter, the outputs written once
        passes = 2 * (2.0 * T * H * 224 * 3 + T * 224 * 224 * 3)

        def int16_diff():
            return (nxt.to(torch.int16) - orig.to(torch.int16)).abs().to(torch.uint8)

        def minmax_diff():
            return torch.maximum(nxt, orig) - torch.minimum(nxt, orig)

        forms = {
            "fused": (lambda: eng.residual_resize(frames, out_bilinear=bil, out_lanczos=lan), 2 * frame + passes),
            "fused_residual": (lambda: eng.residual_resize(frames, want_residual=True, out_bilinear=bil, out_lanczos=lan), 3 * frame + passes),
            # int16: 2 casts (1 read + 2 written each), subtract (4 + 2), abs (2 + 2), cast back (2 + 1); then the resize reads 1
            "unfused_int16": (lambda: eng.resize_frames(int16_diff(), out_bilinear=bil, out_lanczos=lan), (6 + 6 + 4 + 3 + 1) * frame + passes),
            # maximum, minimum (2 read + 1 written each), subtract (2 + 1); then the resize reads 1
            "unfused_minmax": (lambda: eng.resize_frames(minmax_diff(), out_bilinear=bil, out_lanczos=lan), (3 + 3 + 3 + 1) * frame + passes),
            "resize_frames": (lambda: eng.resize_frames(orig, out_bilinear=bil, out_lanczos=lan), frame + passes),
        }
        rec = {"T": T, "H": H, "W": W}
        for name, (fn, nbytes) in forms.items():
            rec[name] = _with_bytes(_time_ms(fn, args.repeats, args.calls), nbytes)
        yard = min(("unfused_int16", "unfused_minmax"), key=lambda k: rec[k]["ms_median"])
        spread = max(rec[k]["ms_max"] - rec[k]["ms_min"] for k in ("fused", yard))
        rec["yardstick"] = yard
        rec["spread_ms"] = round(spread, 4)
        rec["fused_over_yardstick"] = round(rec["fused"]["ms_median"] / rec[yard]["ms_median"], 3)
        rec["fused_over_resize_frames"] = round(rec["fused"]["ms_median"] / rec["resize_frames"]["ms_median"], 3)
        rec["fused_not_slower"] = bool(rec["fused"]["ms_median"] <= rec[yard]["ms_median"] + spread)
        out[label] = rec
        print(label, json.dumps(rec), flush=True)
        del frames, orig, nxt
        torch.cuda.empty_cache()
    return out


def vectors_pass(eng, args):
    eng.load_resnet50(synth.resnet50_state_dict())
    eng.load_vit(synth.vit_state_dict("vit_base"), "vit_base")
    clips = [torch.randint(0, 256, (16, 2, 540, 960, 3), dtype=torch.uint8, device="cuda") for _ in range(args.clips)]
    eng.reserve(16 * args.clips)
    out = {"clips": args.clips, "pairs_per_clip": 16, "H": 540, "W": 960, "backbones": "resnet50 + vit_base", "precision": eng.precision()}
    for name in ("frame_diff", "optical_flow"):
        whole = _time_ms(lambda: eng.whole_residual_vectors(clips, name), args.repeats, 1, warmup=1)

        def inputs():
            for c in clips:
                eng._whole_residual_inputs(c, name, True, True)
        stage = _time_ms(inputs, args.repeats, 1, warmup=1)
        out[name] = {"whole_pass": whole, "input_stage": stage,
                     "input_stage_share_pct": round(100.0 * stage["ms_median"] / whole["ms_median"], 1),
                     "clips_per_s": round(args.clips / (whole["ms_median"] * 1e-3), 1)}
        print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--no-vectors", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = RelaxEngine(0)
    out = {"copy_rate_TBps": COPY_TBPS, "repeats": args.repeats, "calls_per_repeat": args.calls, "resize": resize_shapes(eng, args)}
    if not args.no_vectors:
        out["whole_residual_vectors"] = vectors_pass(eng, args)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
