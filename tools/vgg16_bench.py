"""VGG-16 feature extraction on the MI355X: ms per 1024 fragments (layer stack + pool vector) and algorithmic TFLOP/s, under the
exact-fp32 arithmetic ("gemm_precision" 0) and the default f16x2 (3), with the contraction launches' share from relax_profile_*.

  python tools/vgg16_bench.py [--batch 256] [--reps 4] [--modes 0,3]

Synthetic weights (synth.vgg16_state_dict) and random fragments: the timing does not depend on the values."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

# algorithmic FLOPs of one 224^2 image: 13 convolutions (2 * H*W * Cout * 9 * Cin) and fc1 / fc2
_CONVS = [(224, 64, 3), (224, 64, 64), (112, 128, 64), (112, 128, 128), (56, 256, 128), (56, 256, 256), (56, 256, 256),
          (28, 512, 256), (28, 512, 512), (28, 512, 512), (14, 512, 512), (14, 512, 512), (14, 512, 512)]
FLOPS_PER_IMAGE = sum(2.0 * h * h * co * 9 * ci for h, co, ci in _CONVS) + 2.0 * 4096 * (25088 + 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--modes", default="0,3")
    args = ap.parse_args()
    eng = RelaxEngine(0)
    eng.load_vgg16(synth.vgg16_state_dict())
    g = np.random.default_rng(0)
    frags = torch.from_numpy(g.integers(0, 256, (args.batch, 224, 224, 3), dtype=np.uint8)).cuda()
    out = {"batch": args.batch, "gflop_per_image": FLOPS_PER_IMAGE / 1e9}
    for mode in [int(m) for m in args.modes.split(",")]:
        eng.set_option("gemm_precision", mode)
        eng.vgg16_features(frags)                       # warm-up (workspace, code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.vgg16_features(frags)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.reps
        eng.profile_enable(True)
        eng.vgg16_features(frags)
        torch.cuda.synchronize()
        kinds = {}
        for k, name in ((0, "fp32"), (3, "bf16x6"), (7, "f16x2"), (9, "f16x2_plain")):   # (relax_profile_read's FLOP views)
            r = eng.profile_read(k)
            if r[2]:
                kinds[name] = {"ms": round(r[0], 3), "tflops": round(r[1] / r[0] / 1e9, 1) if r[0] > 0 else None, "launches": r[2]}
        eng.profile_enable(False)
        per1024 = ms * 1024 / args.batch
        out[f"mode{mode}"] = {"ms_per_1024": round(per1024, 2),
                              "tflops": round(FLOPS_PER_IMAGE * 1024 / (per1024 * 1e-3) / 1e12, 1),
                              "profile_by_kind": kinds}
    eng.set_option("gemm_precision", 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
