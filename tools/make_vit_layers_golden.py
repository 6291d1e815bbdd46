"""Writes tests/golden/vit_layers.npz: what the reference's own VisionTransformer.get_intermediate_layers returns
(src/extractor/visualise_vit_layer.py:252-260).  tests/test_vit_layers_cpu.py holds the restatement tests/vit_layers_ref.intermediate_layers
to it; the GPU tests are held to the restatement.

  python tools/make_vit_layers_golden.py --reference /path/to/ReLaX-VQA

The model is the tiny one of tests/golden/vit_canvas.npz (embed_dim 64, depth 2, one head; its weights are read from that file and not
stored again).  Every case asks for n = 3 layers: the model has two blocks, and the reference's `len(self.blocks) - i <= n` then returns
both of them - the recorded tap count (2) is part of the fixture.  Arrays only:
  <case>.shape, .seed, .sum   the input: default_rng(seed).integers(0, 256, shape, uint8), BGR; sum = its byte sum (a check)
  <case>.n                    the n that was asked for
  <case>.cls                  [taps, N, dim]: x[:, 0] of each returned tensor
  <case>.pooled               [taps, N, 3 dim]: mean | max | population std over x[:, 1:] of each returned tensor (numpy, fp32)
  <case>.tokens               [taps, N, ntok, dim]: the returned tensors themselves, on the small canvases only

The reference checkout is read at generation time only (imported with the stubs oracle/make_golden.py uses); the tests never read it."""
import argparse
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relax_vqa_amd  # noqa: E402,F401
from oracle import make_golden  # noqa: E402
from tests import vit_canvas_ref, vit_layers_ref  # noqa: E402

DIM, DEPTH, HEADS = 64, 2, 1
N_LAST = 3
# (name, patch, images, Hc, Wc, store the tokens): 3 x 5 patches (a count no multiple of 4), the table's own grid, patch 8's 8 x 5
CASES = [("p16_48x80", 16, 2, 48, 80, True), ("p16_224x224", 16, 1, 224, 224, False), ("p8_64x40", 8, 2, 64, 40, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=make_golden.REF)
    args = ap.parse_args()
    make_golden.REF = args.reference
    make_golden.REF_SRC = os.path.join(args.reference, "src")
    rv = make_golden.import_reference_vit()
    z = np.load(os.path.join(ROOT, "tests", "golden", "vit_canvas.npz"))
    out, models = {}, {}
    for i, (name, patch, n_img, Hc, Wc, keep_tokens) in enumerate(CASES):
        if patch not in models:
            m = rv.VisionTransformer(patch_size=patch, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, mlp_ratio=4, qkv_bias=True,
                                     norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
            m.load_state_dict(vit_canvas_ref.golden_state_dict(z, patch), strict=True)
            models[patch] = m.eval()
        seed, shape = 300 + i, (n_img, Hc, Wc, 3)
        img = vit_canvas_ref.golden_input(shape, seed)
        with torch.no_grad():
            taps = models[patch].get_intermediate_layers(vit_canvas_ref.preprocess_bgr_u8(img), N_LAST)
        ntok = (Hc // patch) * (Wc // patch) + 1
        assert len(taps) == min(N_LAST, DEPTH) and all(tuple(t.shape) == (n_img, ntok, DIM) for t in taps)
        out[f"{name}.shape"], out[f"{name}.seed"], out[f"{name}.sum"] = np.int64(shape), np.int64(seed), np.int64(img.sum(dtype=np.int64))
        out[f"{name}.n"] = np.int64(N_LAST)
        out[f"{name}.cls"] = np.stack([t[:, 0].numpy() for t in taps])
        out[f"{name}.pooled"] = np.stack([vit_layers_ref.pooled(t) for t in taps])
        if keep_tokens:
            out[f"{name}.tokens"] = np.stack([t.numpy() for t in taps])
        print(name, "taps", len(taps), "tokens", tuple(taps[0].shape))
    path = os.path.join(ROOT, "tests", "golden", "vit_layers.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
