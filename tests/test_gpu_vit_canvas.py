"""The ViT on any canvas, on the GPU: the resampled position table against torch-CPU fp32 (csrc/vit.hip: vit_pos_interp), the forwards
against the restatement tests/vit_canvas_ref.forward_canvas (itself pinned to the reference's class by tests/test_vit_canvas_cpu.py), the
224 x 224 call bit for bit against the entry points that never took a canvas, and the Python surface."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import vit_ref
from tests import gpu_common, vit_canvas_ref
from tests.gpu_common import assert_close, engine, synth

pytestmark = pytest.mark.gpu

HEADS = {"vit_tiny": 3, "vit_small": 6, "vit_base": 12}


@functools.lru_cache(maxsize=None)
def _weights(name, patch, adversarial):
    return synth.vit_state_dict(name, patch=patch, adversarial=adversarial)


def _load(name, patch=16, adversarial=False):
    """synthetic weights into the shared engine, through the other GPU tests' cache where it knows the model (patch 16)"""
    if patch == 16:
        return gpu_common.vit_weights(name, adversarial)
    key = f"vit{patch}:{name}:{adversarial}"
    if gpu_common._weights.get("vit_loaded") != key:
        engine().load_vit(_weights(name, patch, adversarial), name)
        gpu_common._weights["vit_loaded"] = key
    return _weights(name, patch, adversarial)


def _images(n, Hc, Wc, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)


# ---- the position table ----------------------------------------------------------------------------------------------------------------
def _pos_reference(sd, gh, gw):
    """-> (torch-CPU fp32 table [1 + gh*gw, dim], yardstick): the yardstick of a grid is the distance between torch's own fp32 and fp64
    F.interpolate on this table - what evaluating the source coordinates in fp32 costs (1.5e-6 .. 7e-6 on an N(0,1) table), in the
    table's own scale"""
    pos = torch.from_numpy(np.asarray(sd["pos_embed"]))
    f32 = vit_canvas_ref.interpolate_pos(pos, gh, gw, torch.float32)[0]
    f64 = vit_canvas_ref.interpolate_pos(pos, gh, gw, torch.float64)[0]
    return f32, float((f32.double() - f64).abs().max())


POS_GRIDS = [(16, (14, 14)), (16, (1, 1)), (16, (3, 5)), (16, (7, 28)), (16, (14, 15)), (16, (20, 14)), (16, (28, 28)), (16, (64, 64)),
             (8, (8, 5)), (8, (14, 14))]


@pytest.mark.parametrize("patch,grid", POS_GRIDS, ids=[f"p{p}-{g[0]}x{g[1]}" for p, g in POS_GRIDS])
def test_pos_embed_matches_torch_fp32(patch, grid):
    sd = _load("vit_tiny", patch)
    eng = engine()
    gh, gw = grid
    got = eng.vit_pos_embed(gh, gw)
    assert tuple(got.shape) == (1 + gh * gw, 192)
    want, yard = _pos_reference(sd, gh, gw)
    if (gh, gw) == (224 // patch, 224 // patch):
        assert torch.equal(got.cpu(), torch.from_numpy(np.asarray(sd["pos_embed"]))[0]), "the identity grid is not the loaded table"
    else:
        assert torch.equal(got[0].cpu(), want[0]), "the class row is not copied"
        err = float((got.cpu().double() - want.double()).abs().max())
        print(f"\npos_embed patch {patch} grid {gh} x {gw}: |gpu - torch fp32| {err:.3e}, yardstick |torch fp32 - fp64| {yard:.3e}, "
              f"max|pos| {float(want.abs().max()):.3e}")
        assert err <= yard, f"grid {gh} x {gw}: {err:.3e} from torch-CPU fp32, torch's own fp32 is {yard:.3e} from fp64"
    # the cache: the same bits on a second call, and after another grid has been asked for in between
    assert torch.equal(got, eng.vit_pos_embed(gh, gw))
    for other in ((2, 3), (5, 2), (9, 9), (4, 11), (6, 6)):       # more grids than the cache holds
        eng.vit_pos_embed(*other)
    assert torch.equal(got, eng.vit_pos_embed(gh, gw))


def test_pos_embed_cache_is_dropped_by_a_load():
    eng = engine()
    sd = _load("vit_tiny", 16)
    before = eng.vit_pos_embed(5, 7)
    other = dict(sd)
    other["pos_embed"] = (np.asarray(sd["pos_embed"]) * 2).astype(np.float32)
    eng.load_vit(other, "vit_tiny")
    gpu_common._weights["vit_loaded"] = "vit_canvas:doubled"
    after = eng.vit_pos_embed(5, 7)
    assert torch.equal(after[0], before[0] * 2) and not torch.equal(after, before)
    assert_close(after, (before * 2).cpu().numpy(), "the table of the reloaded model")


# ---- model level -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_reference(name, patch, adversarial, n, Hc, Wc):
    """-> (images, tokens, pooled, the last block's CLS attention row [n, heads, ntok]) of the restatement, once per case"""
    imgs = _images(n, Hc, Wc, seed=Hc * 1000 + Wc)
    tsd = vit_ref.to_torch_state_dict(_weights(name, patch, adversarial))
    _, tok, att = vit_canvas_ref.forward_canvas(tsd, vit_canvas_ref.preprocess_bgr_u8(imgs), HEADS[name], patch)
    tok = tok.numpy()
    return imgs, tok, vit_canvas_ref.pooled(tok), att[:, :, 0, :].numpy()


def _check_model(name, patch, adversarial, n, Hc, Wc, precision):
    imgs, tok, pooled, att = _model_reference(name, patch, adversarial, n, Hc, Wc)
    _load(name, patch, adversarial)
    eng = engine()
    eng.set_precision(precision)
    gh, gw = Hc // patch, Wc // patch
    assert eng.vit_canvas_geometry(Hc, Wc) == (gh, gw, gh * gw + 1)
    g_tok, g_pool, g_att = eng.vit_features(imgs, tokens=True, pooled=True, attention=True)
    what = f"{name}/{patch} {Hc}x{Wc} {precision}{' adversarial' if adversarial else ''}"
    dim = tok.shape[2]
    assert tuple(g_tok.shape) == (n, gh * gw, dim) and tuple(g_pool.shape) == (n, 3 * dim) and tuple(g_att.shape) == (n, HEADS[name], gh * gw)
    assert_close(g_tok, tok, f"{what} tokens")
    assert_close(g_pool, pooled, f"{what} pooled")
    assert_close(g_att, att[:, :, 1:], f"{what} CLS attention")
    row = eng.vit_attention(imgs, with_cls=True)
    assert tuple(row.shape) == (n, HEADS[name], gh * gw + 1)
    assert float((row.sum(dim=2) - 1).abs().max()) <= 1e-5, f"{what}: attention rows do not sum to 1"
    assert_close(row, att, f"{what} CLS attention row")
    assert torch.equal(row[:, :, 1:], g_att), f"{what}: vit_attention differs from vit_features(attention=True)"
    return g_tok, g_pool, g_att


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
@pytest.mark.parametrize("Hc,Wc", [(96, 160), (230, 250), (112, 448)], ids=["96x160", "230x250", "112x448"])
def test_vit_tiny_canvases_match_the_restatement(Hc, Wc, precision):
    """96 x 160: 61 tokens, two key tiles of the streaming kernels, the second nearly empty; 230 x 250: 14 x 15 patches, 6 rows and 10 columns
    of pixels dropped; 112 x 448: 7 x 28 = 196 patches, the single-tile kernels with a resampled table.  f16x2 runs vit_tiny on bf16x6."""
    got = _check_model("vit_tiny", 16, False, 3, Hc, Wc, precision)
    if (Hc, Wc) == (230, 250):      # the dropped margin is never read: 255 there or 0, the same bits
        imgs = _model_reference("vit_tiny", 16, False, 3, Hc, Wc)[0]
        eng = engine()
        for fill in (255, 0):
            m = imgs.copy()
            m[:, 224:, :, :] = fill
            m[:, :, 240:, :] = fill
            again = eng.vit_features(m, tokens=True, pooled=True, attention=True)
            for a, b, what in zip(got, again, ("tokens", "pooled", "attention")):
                assert torch.equal(a, b), f"margin filled with {fill}: {what} changed"


def test_vit_tiny_patch8_canvas_matches_the_restatement():
    _check_model("vit_tiny", 8, False, 2, 64, 40, "fp32")
    _check_model("vit_tiny", 8, False, 2, 64, 40, "f16x2")


@pytest.mark.parametrize("adversarial", [False, True], ids=["regular", "adversarial"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x2"])
def test_vit_base_canvas_matches_the_restatement(precision, adversarial):
    """112 x 176: 7 x 11 + 1 = 78 tokens; under f16x2 the f16x2 forward with the streaming attention writing fp16 planes, at a count that is
    neither 197 nor 785"""
    _check_model("vit_base", 16, adversarial, 2, 112, 176, precision)


def test_cls_attention_past_1024_keys():
    """528 x 528: 33^2 + 1 = 1090 tokens, the second instantiation of vit_cls_attention (17 keys per thread)"""
    _check_model("vit_tiny", 16, False, 1, 528, 528, "fp32")


# ---- 224 x 224 is what it was ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x2"])
def test_224_through_the_canvas_entry_point_is_bit_equal(precision):
    _load("vit_base")
    eng = engine()
    eng.set_precision(precision)
    frags = torch.from_numpy(_images(3, 224, 224, seed=224)).cuda()
    n, dim, heads = 3, 768, 12
    tk, pl, at = eng.vit_features(frags, tokens=True, pooled=True, attention=True)            # relax_vit_features_canvas
    tk0 = torch.empty((n, 196, dim), dtype=torch.float32, device="cuda")
    pl0 = torch.empty((n, 3 * dim), dtype=torch.float32, device="cuda")
    eng._check(eng.lib.relax_vit_features(eng.h, frags.data_ptr(), n, tk0.data_ptr(), pl0.data_ptr(), None), "relax_vit_features")
    assert torch.equal(tk, tk0) and torch.equal(pl, pl0)
    tk1, pl1, at1 = torch.empty_like(tk0), torch.empty_like(pl0), torch.empty((n, heads, 197), dtype=torch.float32, device="cuda")
    eng._check(eng.lib.relax_vit_features_ex(eng.h, frags.data_ptr(), n, tk1.data_ptr(), pl1.data_ptr(), at1.data_ptr(), None),
               "relax_vit_features_ex")
    assert torch.equal(tk, tk1) and torch.equal(pl, pl1) and torch.equal(at, at1[:, :, 1:])


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
def test_shapes_follow_the_call_and_224_is_untouched_by_other_canvases():
    _load("vit_tiny")
    eng = engine()
    f224 = _images(2, 224, 224, seed=1)
    before = eng.vit_features(f224, tokens=True, pooled=True, attention=True)
    assert tuple(before[0].shape) == (2, 196, 192) and tuple(before[2].shape) == (2, 3, 196)
    tok, pool = eng.vit_features(_images(2, 96, 160, seed=2), tokens=True, pooled=True)
    assert tuple(tok.shape) == (2, 60, 192) and tuple(pool.shape) == (2, 576)
    assert tuple(eng.vit_features(_images(1, 100, 100, seed=3)[0], tokens=True, pooled=False)[0].shape) == (1, 36, 192)   # one [H,W,3] image
    after = eng.vit_features(f224, tokens=True, pooled=True, attention=True)
    for a, b in zip(before, after):
        assert a.shape == b.shape and torch.equal(a, b)
    assert eng.vit_geometry() == (16, 197, 192, 3) and (eng.vit_ntok, eng.vit_npatch) == (197, 196)


def test_refused_canvases_name_the_value():
    _load("vit_tiny")
    eng = engine()
    with pytest.raises(RuntimeError, match=r"\b15\b"):
        eng.vit_features(np.zeros((1, 15, 300, 3), dtype=np.uint8))
    with pytest.raises(RuntimeError, match=r"\b15\b"):
        eng.vit_canvas_geometry(15, 300)
    with pytest.raises(RuntimeError, match=r"1040 x 1040.*4225 patches"):
        eng.vit_attention(np.zeros((1, 1040, 1040, 3), dtype=np.uint8))
    assert eng.vit_canvas_geometry(1024, 1024) == (64, 64, 4097)
    with pytest.raises(RuntimeError, match="65 x 64"):
        eng.vit_pos_embed(65, 64)
    with pytest.raises(ValueError):
        eng.vit_features(np.zeros((1, 32, 32, 4), dtype=np.uint8))
    rc = eng.lib.relax_vit_features_canvas(eng.h, C.c_void_p(16), 1, 32, 32, None, None, None, None)
    assert rc != 0 and b"no output" in eng.lib.relax_last_error(eng.h)


def test_visualise_vit_crops_to_patch_multiples():
    from relax_vqa_amd import runtime
    from relax_vqa_amd.extractor import visualise_vit, visualise_vit_layer
    try:
        model = visualise_vit_layer.VitGenerator("vit_tiny", 16, None, random=True)
        img = _images(1, 100, 150, seed=7)[0]                         # crops to 96 x 144: 6 x 9 patches
        maps = visualise_vit.visualize_attention(model, img, 16, None)
        assert maps.shape == (3, 96, 144) and maps.dtype == np.float32
        tsd = vit_ref.to_torch_state_dict(synth.vit_state_dict("vit_tiny"))
        _, want_tok, att = vit_canvas_ref.forward_canvas(tsd, vit_canvas_ref.preprocess_bgr_u8(img[None, :96, :144]), 3, 16)
        want = att[0, :, 0, 1:].reshape(3, 6, 9).numpy()
        assert_close(maps[:, ::16, ::16], want, "visualize_attention 100 x 150")
        assert (maps.reshape(3, 6, 16, 9, 16) == maps[:, ::16, ::16][:, :, None, :, None]).all(), "a value is not repeated over its patch"
        tokens = visualise_vit_layer.process_fragment_array(img[:96, :144], model)
        assert tokens.shape == (54, 192)
        assert_close(tokens, want_tok[0].numpy(), "process_fragment_array 96 x 144")
        heads, _ = visualise_vit.process_video_frame(img, "v", "original", model, 16, None)      # the reference's resize to 224 stays
        assert len(heads) == 3 and heads[0].shape == (224, 224)
    finally:
        runtime.set_weights(vit=synth.vit_state_dict("vit_base"), vit_name="vit_base")   # what the other host-API tests run on


def test_fragment_vit_vectors_at_448():
    _load("vit_tiny")
    eng = engine()
    clip = torch.from_numpy(synth.synthetic_clip(2, 540, 960, clip_id=6)).cuda()
    rows = eng.fragment_vit_vectors(clip, target_size=448)
    assert tuple(rows.shape) == (2, 6 * 192)
    fr = eng.fragment_pairs(clip, top_n=None, patch_size=16, target_size=448)
    assert tuple(fr["ori_frag"].shape) == (2, 448, 448, 3)
    _, po = eng.vit_features(fr["ori_frag"], tokens=False, pooled=True)
    _, pd = eng.vit_features(fr["diff_frag"], tokens=False, pooled=True)
    assert_close(rows, torch.cat([po, pd], dim=1).cpu().numpy(), "fragment_vit_vectors(448)")
    _, both = eng.vit_features(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), tokens=False, pooled=True)
    assert torch.equal(rows, torch.cat([both[:2], both[2:]], dim=1))
    # and against the restatement, on the fragments the GPU cut
    tsd = vit_ref.to_torch_state_dict(synth.vit_state_dict("vit_tiny"))
    _, tok, _ = vit_canvas_ref.forward_canvas(tsd, vit_canvas_ref.preprocess_bgr_u8(fr["ori_frag"][:1].cpu().numpy()), 3, 16)
    assert tuple(tok.shape) == (1, 784, 192)
    assert_close(rows[:1, :576], vit_canvas_ref.pooled(tok.numpy()), "the 448 fragment's pool against the restatement")
    # the default canvas is extract_clip's 'vit' block; the clip paths still take 224 only
    out = eng.extract_clip(clip, resnet=False, vit=True)
    assert torch.equal(eng.fragment_vit_vectors(clip), out["vit"])
    with pytest.raises(ValueError, match="target_size=448"):
        eng.extract_clip(clip, target_size=448)
