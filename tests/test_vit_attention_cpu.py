"""CPU checks of the attention visualisation: the restatement's block loop is the oracle's, the integer blend of
csrc/vit_attention_map.hip is cv2.addWeighted's float result, the default colour table is matplotlib's jet, and the numpy
transcription of map_attention_to_original agrees with a pixel loop on ragged frames."""
import numpy as np
import pytest
import torch

import relax_vqa_amd  # noqa: F401
from oracle import vit_ref
from relax_vqa_amd import colormap, synth
from tests import vit_attention_restated as var


def _frags(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def test_restated_block_loop_is_the_oracles():
    sd = synth.vit_state_dict("vit_tiny")
    frags = _frags(2, 5)
    want = vit_ref.forward_tokens(vit_ref.to_torch_state_dict(sd), vit_ref.preprocess_bgr_u8(frags), 3)
    got = var.all_blocks_tokens(sd, frags, 3, torch.float32)
    assert torch.equal(got, want)
    rows = var.cls_rows(sd, frags, 3)
    assert rows.shape == (2, 3, 197)
    assert np.allclose(rows.sum(axis=-1), 1.0, atol=1e-12) and (rows >= 0).all()


def test_integer_blend_is_addweighted_for_every_byte_pair():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    integer = ((6 * a.astype(np.int64) + 4 * b.astype(np.int64) + 5) // 10).astype(np.uint8)
    assert np.array_equal(integer, var.add_weighted_f32(a, b))
    r64 = 0.6 * a.astype(np.float64) + 0.4 * b.astype(np.float64)
    assert np.array_equal(integer, np.rint(r64).astype(np.uint8))
    assert np.abs(r64 - np.floor(r64) - 0.5).min() >= 0.09            # no tie anywhere: every rounding mode agrees


def test_default_lut_is_matplotlib_jet():
    matplotlib = pytest.importorskip("matplotlib")
    rgba = matplotlib.colormaps["jet"](np.arange(256))
    assert np.array_equal(colormap.jet_rgb_float(), rgba[:, :3])
    want = np.rint(rgba[:, :3] * 255.0)[:, ::-1].astype(np.uint8)
    lut = colormap.jet_lut_bgr()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3) and lut.flags.c_contiguous
    assert np.array_equal(lut, want)
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[255]) == (0, 0, 128)   # dark blue .. dark red, in BGR


def _case(H, W, count, seed, values=None):
    g = np.random.default_rng(seed)
    frame = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ph, pw = H // 16, W // 16
    flat = g.permutation(ph * pw)[:count]
    pos = np.full((196, 2), -1, dtype=np.int32)
    pos[:len(flat), 0], pos[:len(flat), 1] = flat // pw, flat % pw
    vals = g.random(196).astype(np.float32) if values is None else values
    return frame, pos, vals


@pytest.mark.parametrize("H,W,count,kind", [(97, 131, 48, "random"), (100, 200, 72, "random"), (40, 50, 6, "hot"),
                                            (64, 80, 20, "equal"), (224, 224, 196, "random"), (33, 47, 3, "duplicate")])
def test_numpy_restatement_equals_a_pixel_loop(H, W, count, kind):
    lut = colormap.jet_lut_bgr()
    vals = None
    if kind == "hot":
        vals = np.zeros(196, np.float32)
        vals[2] = 0.37
    elif kind == "equal":
        vals = np.full(196, 0.25, np.float32)
    frame, pos, vals = _case(H, W, count, H * W, vals)
    if kind == "duplicate":
        pos[2] = pos[0]                                    # a later slot on the same patch wins
    n = min(count, (H // 16) * (W // 16))
    want = var.overlay_pixel_loop(frame, vals, pos, n, lut)
    got = var.map_attention_to_original(frame, vals[:n], pos[:n], 16, lut)
    assert np.array_equal(got, want)
