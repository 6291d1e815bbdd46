"""Writes tests/golden/vit_canvas.npz: what the reference's own VisionTransformer computes on canvases other than 224 x 224, where its
prepare_tokens resamples the position table (interpolate_pos_encoding).  tests/test_vit_canvas_cpu.py holds the restatement
tests/vit_canvas_ref.forward_canvas to it; the GPU tests are held to the restatement.

  python tools/make_vit_canvas_golden.py --reference /path/to/ReLaX-VQA

A tiny model (embed_dim 64, depth 2, one head, qkv_bias, LayerNorm eps 1e-6) at patch 16 and patch 8: the two share their blocks and
final norm and differ in patch_embed and pos_embed.  pos_embed and cls_token are N(0,1) draws, so the resampled table matters in the
outputs.  Arrays only:
  w.<key> / w16.<key> / w8.<key>   weights as float16 - every value was rounded to fp16 BEFORE the reference ran, so the fp32 weights
                                   the reference saw are exactly these
  <case>.shape, .seed, .sum        the input: default_rng(seed).integers(0, 256, shape, uint8), BGR; sum = its byte sum (a check)
  <case>.cls, .tokens              forward's two outputs
  <case>.attn / .attn_rows         get_last_selfattention [1, 1, ntok, ntok], whole where ntok <= 64; else the query rows .attn_rows

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
from tests import vit_canvas_ref  # noqa: E402

DIM, DEPTH, HEADS = 64, 2, 1
# (name, patch, Hc, Wc): grids 6 x 10, 14 x 15 (dropped pixels), 7 x 28 (196 patches, not the table's grid), 1 x 1, 8 x 5
CASES = [("p16_96x160", 16, 96, 160), ("p16_230x250", 16, 230, 250), ("p16_112x448", 16, 112, 448), ("p16_16x16", 16, 16, 16),
         ("p8_64x40", 8, 64, 40)]
WEIGHT_SEED = 7


def fp16_exact(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def weights(seed=WEIGHT_SEED):
    """-> (shared, {16: .., 8: ..}): float16 arrays under the DINO state-dict keys"""
    rng = np.random.default_rng(seed)

    def normal(shape, std):
        return fp16_exact(rng.standard_normal(shape) * std)

    shared = {}
    for i in range(DEPTH):
        p = f"blocks.{i}."
        shared[p + "norm1.weight"] = fp16_exact(1 + 0.1 * rng.standard_normal(DIM))
        shared[p + "norm1.bias"] = normal(DIM, 0.1)
        shared[p + "attn.qkv.weight"] = normal((3 * DIM, DIM), 0.15)
        shared[p + "attn.qkv.bias"] = normal(3 * DIM, 0.1)
        shared[p + "attn.proj.weight"] = normal((DIM, DIM), 0.1)
        shared[p + "attn.proj.bias"] = normal(DIM, 0.1)
        shared[p + "norm2.weight"] = fp16_exact(1 + 0.1 * rng.standard_normal(DIM))
        shared[p + "norm2.bias"] = normal(DIM, 0.1)
        shared[p + "mlp.fc1.weight"] = normal((4 * DIM, DIM), 0.1)
        shared[p + "mlp.fc1.bias"] = normal(4 * DIM, 0.1)
        shared[p + "mlp.fc2.weight"] = normal((DIM, 4 * DIM), 0.05)
        shared[p + "mlp.fc2.bias"] = normal(DIM, 0.1)
    shared["norm.weight"] = fp16_exact(1 + 0.1 * rng.standard_normal(DIM))
    shared["norm.bias"] = normal(DIM, 0.1)
    shared["cls_token"] = normal((1, 1, DIM), 1.0)
    per_patch = {}
    for patch in (16, 8):
        side = 224 // patch
        per_patch[patch] = {
            "pos_embed": normal((1, 1 + side * side, DIM), 1.0),
            "patch_embed.proj.weight": normal((DIM, 3, patch, patch), 0.05),
            "patch_embed.proj.bias": normal(DIM, 0.1),
        }
    return shared, per_patch


def state_dict(w, patch):
    """the fp32 torch state dict of one patch size from weights()"""
    sd = dict(w[0])
    sd.update(w[1][patch])
    return {k: torch.from_numpy(np.asarray(v).astype(np.float32)) for k, v in sd.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=make_golden.REF)
    args = ap.parse_args()
    make_golden.REF = args.reference
    make_golden.REF_SRC = os.path.join(args.reference, "src")
    rv = make_golden.import_reference_vit()
    w = weights()
    out = {f"w.{k}": v for k, v in w[0].items()}
    for patch in (16, 8):
        out.update({f"w{patch}.{k}": v for k, v in w[1][patch].items()})
    models = {}
    for i, (name, patch, Hc, Wc) in enumerate(CASES):
        if patch not in models:
            m = rv.VisionTransformer(patch_size=patch, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, mlp_ratio=4, qkv_bias=True,
                                     norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
            m.load_state_dict(state_dict(w, patch), strict=True)
            models[patch] = m.eval()
        seed, shape = 100 + i, (1, Hc, Wc, 3)
        img = vit_canvas_ref.golden_input(shape, seed)
        x = vit_canvas_ref.preprocess_bgr_u8(img)
        with torch.no_grad():
            cls, tokens = models[patch](x)
            attn = models[patch].get_last_selfattention(x)
        ntok = (Hc // patch) * (Wc // patch) + 1
        assert tuple(tokens.shape) == (1, ntok - 1, DIM) and tuple(attn.shape) == (1, HEADS, ntok, ntok), (tokens.shape, attn.shape)
        out[f"{name}.shape"], out[f"{name}.seed"], out[f"{name}.sum"] = np.int64(shape), np.int64(seed), np.int64(img.sum(dtype=np.int64))
        out[f"{name}.cls"], out[f"{name}.tokens"] = cls.numpy(), tokens.numpy()
        if ntok <= 64:
            out[f"{name}.attn"] = attn.numpy()
        else:
            rows = np.int64([0, 1, ntok // 2, ntok - 1])
            out[f"{name}.attn_rows"], out[f"{name}.attn"] = rows, attn.numpy()[:, :, rows]
        print(name, "grid", Hc // patch, "x", Wc // patch, "tokens", tuple(tokens.shape))
    path = os.path.join(ROOT, "tests", "golden", "vit_canvas.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
