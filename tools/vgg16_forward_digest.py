#!/usr/bin/env python3
"""What the VGG-16 forward computes and which contraction kernels it launches, for every route of host::vgg_plan (GPU box only).
  python tools/vgg16_forward_digest.py [OUT.json]
RELAX_HIP_LIB selects the build: run once per build and compare - two builds whose forwards launch the same kernels on the same buffers
print the same digests and the same launch / work figures.
Matrix (synthetic state dict of synth.py, seeded uint8 fragments, gemm_split_k 0): gemm_precision 0 / 1 / 2 / 3 x {layer stack + pool vector +
all 15 taps, pool vector only, layer stack only} x N in {2, 33} (33: one chunk of 32 images and one of 1).  Per run: the sha256 of every output
tensor and relax_profile_read's launches and work of kinds 0 (fp32 / bf16x3), 3 (bf16x6), 7 (f16x2) and 9 (the plain f16x2 GEMMs).  One line
per run."""
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

KINDS = (0, 3, 7, 9)
REQUESTS = (("both + all taps", dict(taps=range(15))), ("pool only", dict(layer_stack=False)), ("layer stack only", dict(pool=False)))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(eng, frags, kwargs):
    """the outputs' digests by name, and {kind: [launches, work]} of the run"""
    eng.profile_enable(True)
    try:
        res = eng.vgg16_features(frags, **kwargs)
        out = {name: sha(t) for name, t in zip(("layer_stack", "pool"), res[:2]) if t is not None}
        if len(res) > 2:
            out.update({f"tap{k}": sha(t) for k, t in sorted(res[2].items())})
        reads = {k: eng.profile_read(k) for k in KINDS}
    finally:
        eng.profile_enable(False)
    out["profile"] = {str(k): [n, work] for k, (_, work, n) in reads.items()}
    return out


def digest():
    eng = RelaxEngine(0)
    eng.set_option("gemm_split_k", 0)
    eng.load_vgg16(synth.vgg16_state_dict())
    out = {}
    for n in (2, 33):
        frags = torch.from_numpy(np.random.default_rng(100 + n).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)).cuda()
        for p in (0, 1, 2, 3):
            eng.set_option("gemm_precision", p)
            for what, kwargs in REQUESTS:
                out[f"p{p} N={n} {what}"] = run(eng, frags, kwargs)
    torch.cuda.synchronize()
    eng.close()
    return out


if __name__ == "__main__":
    runs = digest()
    lines = ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in runs.items())
    text = '{"lib": %s, "runs": {\n%s\n}}' % (json.dumps(os.path.basename(os.environ.get("RELAX_HIP_LIB", "in-tree"))), lines)
    json.loads(text)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
