"""ViT attention visualisation on the MI355X (csrc/vit_attention_map.hip), timed with device events after a warm-up:

  - ms per 1024 fragments of vit_features(pooled), of the same call with attention=True, and of vit_attention alone (the forward
    stops after the last block's qkv GEMM), under f16x2;
  - attention_overlay in us per frame and GB/s (6 H W bytes per frame: 3 read, 3 written) at 1080p and 2160p with T = 32, against
    the 6.29 TB/s device copy rate.

  python tools/vit_attention_bench.py [--batch 256] [--reps 10] [--out profiles/vit_attention_bench.json]

Synthetic weights (synth.vit_state_dict) and random inputs: the timing does not depend on the values."""
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


def _time_ms(fn, reps, warmup=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = RelaxEngine(0)
    eng.load_vit(synth.vit_state_dict("vit_base"), "vit_base")
    eng.set_precision("f16x2")
    g = np.random.default_rng(0)
    frags = torch.from_numpy(g.integers(0, 256, (args.batch, 224, 224, 3), dtype=np.uint8)).cuda()
    eng.reserve(args.batch)
    scale = 1024 / args.batch
    out = {"batch": args.batch, "precision": "f16x2", "reps": args.reps}
    runs = {"pooled": lambda: eng.vit_features(frags, tokens=False, pooled=True),
            "pooled_with_attention": lambda: eng.vit_features(frags, tokens=False, pooled=True, attention=True),
            "attention_only": lambda: eng.vit_attention(frags)}
    vit = {}
    for name, fn in runs.items():
        med, best = _time_ms(fn, args.reps)
        vit[name] = {"ms_per_1024_median": round(med * scale, 2), "ms_per_1024_min": round(best * scale, 2)}
    base = vit["pooled"]["ms_per_1024_median"]
    vit["attention_overhead_pct"] = round(100.0 * (vit["pooled_with_attention"]["ms_per_1024_median"] / base - 1.0), 2)
    vit["attention_only_pct_of_pooled"] = round(100.0 * vit["attention_only"]["ms_per_1024_median"] / base, 1)
    out["vit"] = vit
    ov = {}
    T = args.frames
    for label, (H, W) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        frames = torch.from_numpy(g.integers(0, 256, (T, H, W, 3), dtype=np.uint8)).cuda()
        pos = np.full((T, 196, 2), -1, dtype=np.int32)
        flat = np.stack([g.permutation((H // 16) * (W // 16))[:196] for _ in range(T)])
        pos[..., 0], pos[..., 1] = flat // (W // 16), flat % (W // 16)
        pos, counts = torch.from_numpy(pos).cuda(), torch.full((T,), 196, dtype=torch.int32).cuda()
        vals = torch.rand((T, 196), device="cuda")
        o = eng.attention_overlay(frames, pos, counts, vals)
        med, best = _time_ms(lambda: eng.attention_overlay(frames, pos, counts, vals), args.reps)
        del o
        nbytes = 6.0 * H * W * T
        ov[label] = {"T": T, "us_per_frame_median": round(med * 1e3 / T, 2), "us_per_frame_min": round(best * 1e3 / T, 2),
                     "GBps_median": round(nbytes / (med * 1e-3) / 1e9, 1),
                     "pct_of_copy_rate": round(100.0 * nbytes / (med * 1e-3) / (COPY_TBPS * 1e12), 1)}
        del frames
    out["overlay"] = ov
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
