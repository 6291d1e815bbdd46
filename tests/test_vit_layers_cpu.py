"""The ViT layer stack without a GPU: the restatement tests/vit_layers_ref.intermediate_layers against what the reference's own
get_intermediate_layers returned (tests/golden/vit_layers.npz, tools/make_vit_layers_golden.py), its tap count and its last tap against
tests/vit_canvas_ref.forward_canvas, and the new entry point in the header and the ctypes table."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import relax_vqa_amd  # noqa: F401
from tests import vit_canvas_ref, vit_layers_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (case of the fixture, patch, images, grid, whole tokens stored)
GOLDEN_CASES = [("p16_48x80", 16, 2, (3, 5), True), ("p16_224x224", 16, 1, (14, 14), False), ("p8_64x40", 8, 2, (8, 5), True)]
DIM, DEPTH = 64, 2


def _case(golden_dir, name, patch):
    z = np.load(os.path.join(golden_dir, "vit_layers.npz"))
    img = vit_canvas_ref.golden_input(z[f"{name}.shape"], z[f"{name}.seed"])
    assert int(img.sum(dtype=np.int64)) == int(z[f"{name}.sum"]), "the seeded input is not the recorded one"
    weights = np.load(os.path.join(golden_dir, "vit_canvas.npz"))
    return z, img, vit_canvas_ref.golden_state_dict(weights, patch)


@pytest.mark.parametrize("name,patch,n_img,grid,whole", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_restatement_matches_the_reference_method(golden_dir, name, patch, n_img, grid, whole):
    """tolerance: the one tests/test_vit_canvas_cpu.py holds forward_canvas to its golden with (rtol = atol = 1e-4).  The fixture's model has
    two blocks and every case asked for n = 3: the reference returns both blocks then, and so must the restatement."""
    z, img, sd = _case(golden_dir, name, patch)
    assert img.shape[0] == n_img and (img.shape[1] // patch, img.shape[2] // patch) == grid
    n = int(z[f"{name}.n"])
    assert n == 3
    taps = vit_layers_ref.intermediate_layers(sd, vit_canvas_ref.preprocess_bgr_u8(img), 1, patch, n)
    ntok = grid[0] * grid[1] + 1
    assert len(taps) == z[f"{name}.cls"].shape[0] == DEPTH
    assert (f"{name}.tokens" in z.files) == whole
    for k, t in enumerate(taps):
        assert tuple(t.shape) == (n_img, ntok, DIM) and t.dtype == torch.float32
        np.testing.assert_allclose(t[:, 0].numpy(), z[f"{name}.cls"][k], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(vit_layers_ref.pooled(t), z[f"{name}.pooled"][k], rtol=1e-4, atol=1e-4)
        if whole:
            np.testing.assert_allclose(t.numpy(), z[f"{name}.tokens"][k], rtol=1e-4, atol=1e-4)


def test_n_counts_from_the_last_block(golden_dir):
    """n = depth returns depth taps; n = 1 returns the last of them; the last tap is forward's norm: its rows 1.. are forward_canvas' tokens and
    its row 0 forward_canvas' cls, bit for bit (the same operations on the same values)."""
    _, img, sd = _case(golden_dir, "p16_48x80", 16)
    x = vit_canvas_ref.preprocess_bgr_u8(img)
    taps = vit_layers_ref.intermediate_layers(sd, x, 1, 16, DEPTH)
    assert len(taps) == DEPTH
    one = vit_layers_ref.intermediate_layers(sd, x, 1, 16, 1)
    assert len(one) == 1 and torch.equal(one[0], taps[-1])
    assert not torch.equal(taps[0], taps[1])
    cls, tokens, _ = vit_canvas_ref.forward_canvas(sd, x, 1, 16)
    assert torch.equal(taps[-1][:, 1:], tokens) and torch.equal(taps[-1][:, 0], cls)


def test_restatement_runs_in_fp64(golden_dir):
    """the dtype parameter (the yardstick of the GPU test's distance-from-fp64 gate): fp64 taps, within the golden's bar of the fp32 ones"""
    _, img, sd = _case(golden_dir, "p8_64x40", 8)
    x = vit_canvas_ref.preprocess_bgr_u8(img)
    t32 = vit_layers_ref.intermediate_layers(sd, x, 1, 8, 2)
    t64 = vit_layers_ref.intermediate_layers(sd, x, 1, 8, 2, dtype=torch.float64)
    for a, b in zip(t32, t64):
        assert b.dtype == torch.float64 and a.dtype == torch.float32
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-4, atol=1e-4)
        assert vit_layers_ref.pooled(b).dtype == np.float64


def test_ctypes_table_lists_the_entry_point():
    from relax_vqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "relax_hip.h")).read()
    ctype_of = {"relax_handle*": C.c_void_p, "const uint8_t*": C.c_void_p, "float*": C.c_void_p, "relax_stream": C.c_void_p, "int": C.c_int}
    name = "relax_vit_intermediate_layers"
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, f"{name} is not declared in relax_hip.h"
    params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is C.c_int and argtypes == [ctype_of[p] for p in params], (name, params)
    # relax_vit_features_canvas' arguments with n_last before the outputs, three outputs as there
    assert len(argtypes) == len(_lib.PROTOTYPES["relax_vit_features_canvas"][1]) + 1
    comment = header[:m.start()].rsplit("/*", 1)[1]
    assert "252-260" in comment and "234-239" in comment, "the header comment does not cite the reference's lines"
