#!/usr/bin/env python3
"""What the ViT forward computes and which contraction kernels it launches, for every route of host::vit_plan (GPU box only).
  python tools/vit_forward_digest.py [OUT.json]
RELAX_HIP_LIB selects the build: run once per build and compare - two builds whose forwards launch the same kernels on the same buffers
print the same digests and the same launch / work figures.
Matrix (synthetic state dicts of synth.py, seeded uint8 images, gemm_split_k 0, N = 2): vit_tiny/16 and vit_base/16 at 224 x 224 and 96 x 160
(61 tokens), vit_base/8 at 64 x 96 (97 tokens) and 224 x 224 (785 tokens, N = 1); gemm_precision 0 / 1 / 2 / 3 and, under 3, att_h2 and
att_h2_stream off in turn; vit_features (tokens + pooled + CLS attention), vit_attention alone (the forward that ends behind the last qkv GEMM),
vit_intermediate_layers with n = 1 and n = 3 (tokens, cls, pooled).  Per run: the sha256 of every output tensor and relax_profile_read's
launches and work of kinds 0 (fp32 / bf16x3), 3 (bf16x6), 7 (f16x2) and 9 (the plain f16x2 GEMMs)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from relax_vqa_amd.engine import RelaxEngine  # noqa: E402

SWITCHES = ("att_h2", "att_h2_stream")
KINDS = (0, 3, 7, 9)
MODELS = (("vit_tiny", 16, ((224, 224, 2), (96, 160, 2))), ("vit_base", 16, ((224, 224, 2), (96, 160, 2))),
          ("vit_base", 8, ((64, 96, 2), (224, 224, 1))))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def settings():
    return [(f"p{p}", {"gemm_precision": p}) for p in (0, 1, 2, 3)] + [(f"p3 {s}=0", {"gemm_precision": 3, s: 0}) for s in SWITCHES]


def profiled(eng, fn):
    """fn()'s tensors by name -> their digests, and {kind: [launches, work]} of the run"""
    eng.profile_enable(True)
    try:
        out = {k: sha(t) for k, t in fn().items()}
        reads = {k: eng.profile_read(k) for k in KINDS}
    finally:
        eng.profile_enable(False)
    out["profile"] = {str(k): [n, work] for k, (_, work, n) in reads.items()}
    return out


def digest():
    eng = RelaxEngine(0)
    eng.set_option("gemm_split_k", 0)
    out = {}
    for name, patch, canvases in MODELS:
        eng.load_vit(synth.vit_state_dict(name, patch=patch), name)
        for Hc, Wc, N in canvases:
            img = torch.from_numpy(np.random.default_rng(1000 * Hc + Wc).integers(0, 256, (N, Hc, Wc, 3), dtype=np.uint8)).cuda()
            for label, opts in settings():
                for s in SWITCHES:
                    eng.set_option(s, 1)
                for k, v in opts.items():
                    eng.set_option(k, v)
                runs = {"features": lambda: dict(zip(("tokens", "pooled", "cls_attention"), eng.vit_features(img, tokens=True, attention=True))),
                        "attention": lambda: {"cls_attention": eng.vit_attention(img, with_cls=True)},
                        "layers n=1": lambda: eng.vit_intermediate_layers(img, n=1, tokens=True),
                        "layers n=3": lambda: eng.vit_intermediate_layers(img, n=3, tokens=True)}
                for what, fn in runs.items():
                    out[f"{name}/{patch} {Hc}x{Wc} {label} {what}"] = profiled(eng, fn)
    torch.cuda.synchronize()
    eng.close()
    return out


if __name__ == "__main__":
    result = {"lib": os.path.basename(os.environ.get("RELAX_HIP_LIB", "in-tree")), "runs": digest()}
    text = json.dumps(result, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
