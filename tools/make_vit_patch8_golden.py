"""Writes tests/golden/vit_patch8_tiny.npz: what the reference's own VisionTransformer(patch_size=8) computes for vit_tiny on two
random fragments, with the synthetic patch-8 weights (synth.vit_state_dict("vit_tiny", patch=8)).  Arrays only: the seed of the input
fragments, the pooled 576-d rows (token mean | max | population std) and a few token rows.  tests/test_vit_geometry_cpu.py holds
oracle.vit_ref.forward_tokens(patch=8) to it within 1e-5.

  python tools/make_vit_patch8_golden.py --reference /path/to/ReLaX-VQA

The reference checkout is read at generation time only (imported with the stubs oracle/make_golden.py uses); the tests never read it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relax_vqa_amd  # noqa: E402,F401
from relax_vqa_amd import synth  # noqa: E402
from oracle import make_golden, vit_ref  # noqa: E402

SEED = 20
N_IMG = 2
TOKEN_ROWS = [0, 1, 27, 28, 391, 392, 755, 783]     # corners, row ends, the centre


def fragments(seed=SEED, n=N_IMG):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=make_golden.REF)
    args = ap.parse_args()
    make_golden.REF = args.reference
    make_golden.REF_SRC = os.path.join(args.reference, "src")
    rv = make_golden.import_reference_vit()
    sd = synth.vit_state_dict("vit_tiny", patch=8)
    gen = rv.VitGenerator("vit_tiny", 8, torch.device("cpu"), evaluate=True, random=True, verbose=False)
    gen.model.load_state_dict(vit_ref.to_torch_state_dict(sd), strict=True)
    x = vit_ref.preprocess_bgr_u8(fragments())
    with torch.no_grad():
        _cls, tokens = gen(x)
    tokens = tokens.numpy()
    assert tokens.shape == (N_IMG, 784, 192), tokens.shape
    pooled = np.concatenate([tokens.mean(axis=1), tokens.max(axis=1), tokens.std(axis=1)], axis=1).astype(np.float32)
    out = os.path.join(ROOT, "tests", "golden", "vit_patch8_tiny.npz")
    np.savez_compressed(out, seed=np.int64(SEED), n_img=np.int64(N_IMG), pooled=pooled, token_rows=np.int64(TOKEN_ROWS),
                        tokens=tokens[:, TOKEN_ROWS])
    print(out, os.path.getsize(out), "bytes; pooled", pooled.shape, "tokens", tokens[:, TOKEN_ROWS].shape)


if __name__ == "__main__":
    main()
