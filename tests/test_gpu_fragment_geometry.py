"""Fragments at patch sizes 8, 16 and 32 on any canvas, and their overlays, on the GPU: every array bit-equal to
oracle.fragment_ref.fragment_pair(..., patch_size, target_size, top_n) / tests.vit_attention_restated.map_attention_to_original.
The shapes are the smallest at which each kernel path can go wrong (aligned 16-byte path with split chunks at P = 8 and a cropped
right edge at P = 32, byte-load path, unaligned base pointer, canvases other than 224, fewer patches than slots)."""
import functools

import numpy as np
import pytest
import torch

from oracle import fragment_ref
from relax_vqa_amd import colormap, demo_visual, main_fragment_layerstack as ml, runtime
from tests import gpu_common, vit_attention_restated as var
from tests.gpu_common import engine, synth

pytestmark = pytest.mark.gpu

LUT = colormap.jet_lut_bgr()


def _slots(p, target):
    return (target // p) ** 2


@functools.lru_cache(maxsize=None)
def _clip(T, h, w, clip_id):
    clip = synth.synthetic_clip(T, h, w, clip_id=clip_id)
    clip.setflags(write=False)
    return clip


@functools.lru_cache(maxsize=None)
def _ref(T, h, w, clip_id, p, target, top_n):
    """the oracle's result for every pair of _clip(T, h, w, clip_id), computed once"""
    clip = _clip(T, h, w, clip_id)
    return tuple(fragment_ref.fragment_pair(clip[t, 0], clip[t, 1], p, target, top_n) for t in range(T))


def _dev(a):
    """a host array (the shared clips are read-only: copied) on the device"""
    return torch.from_numpy(np.array(a)).cuda()


def _run_pairs(frames, p, target, top_n=None):
    if not torch.is_tensor(frames):
        frames = _dev(frames)
    out = engine().fragment_pairs(frames, top_n=top_n, want_scores=True, patch_size=p, target_size=target)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_against(out, t, ref, p, target, expect_count=None):
    slots = _slots(p, target)
    assert out["positions"].shape[1:] == (slots, 2) and out["diff_frag"].shape[1:] == (target, target, 3)
    assert out["scores"][t].shape == ref["score"].shape
    assert np.array_equal(out["scores"][t].astype(np.float64), ref["score"]), "patch scores differ"
    n = len(ref["positions"])
    if expect_count is not None:
        assert n == expect_count, f"the oracle selects {n}, the case was built for {expect_count}"
    assert out["counts"][t] == n
    assert np.array_equal(out["positions"][t, :n], ref["positions"]), "fragment index map differs"
    assert (out["positions"][t, n:] == -1).all(), "padding past the count is not -1"
    assert np.array_equal(out["diff_frag"][t], ref["diff_frag"]), "residual fragment differs"
    assert np.array_equal(out["ori_frag"][t], ref["ori_frag"]), "original fragment differs"


def _check_pairs(frames_np, p, target, top_n=None, expect_count=None, frames_dev=None):
    out = _run_pairs(frames_np if frames_dev is None else frames_dev, p, target, top_n)
    want_n = _slots(p, target) if top_n is None else top_n
    for t in range(frames_np.shape[0]):
        ref = fragment_ref.fragment_pair(frames_np[t, 0], frames_np[t, 1], p, target, want_n)
        _check_against(out, t, ref, p, target, expect_count)
    return out


def _check_image(img, p, target, top_n=None):
    """fragment_image on a single residual image against the oracle's score + extract_important_patches"""
    want_n = _slots(p, target) if top_n is None else top_n
    out = engine().fragment_image(_dev(img[None]), top_n=top_n, want_scores=True, patch_size=p, target_size=target)
    diff = fragment_ref.get_patch_diff(img, p)
    frag, pos = fragment_ref.extract_important_patches(img, diff, p, target, want_n)
    n = len(pos)
    assert np.array_equal(out["scores"][0].cpu().numpy().astype(np.float64), diff)
    assert int(out["counts"][0]) == n
    got_pos = out["positions"][0].cpu().numpy()
    assert np.array_equal(got_pos[:n], pos) and (got_pos[n:] == -1).all()
    assert np.array_equal(out["frag"][0].cpu().numpy(), frag)


# ---- (a) (b): the aligned 16-byte path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p,target,count", [
    (64, 96, 8, 64, 64),          # W*3 = 288: 18 chunks, every third one split between two patches; all 64 slots of 96 patches
    (256, 512, 8, 224, 784),      # 784 of 2048 patches; 768 chunks per strip: two passes of the chunk loop
    (64, 112, 8, 64, 64),         # pw = 14: 21 chunks, seven of them split
    (70, 80, 32, 224, 4),         # pw = 2, 16 columns and 6 rows left over: the chunk loop stops at the last whole patch
    (250, 336, 32, 224, 49),      # 16 columns left over, 7 x 10 = 70 patches
    (256, 512, 32, 224, 49),
])
def test_aligned_path(h, w, p, target, count):
    assert (w * 3) % 16 == 0
    clip = _clip(2, h, w, h + w + p)
    _check_pairs(clip, p, target, expect_count=count)
    _check_image(fragment_ref.absdiff(clip[0, 1], clip[0, 0]), p, target)


# ---- (c): the byte-load path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p,count", [(250, 333, 8, 784), (250, 333, 32, 49), (100, 130, 8, 192)])
def test_byte_load_path(h, w, p, count):
    """100 x 130 at P = 8 has 192 patches for 784 slots: zero tiles and -1 padding past the count"""
    assert (w * 3) % 16 != 0
    clip = _clip(2, h, w, 7)
    out = _run_pairs(clip, p, 224)
    for t, ref in enumerate(_ref(2, h, w, 7, p, 224, _slots(p, 224))):
        _check_against(out, t, ref, p, 224, count)
    if count < _slots(p, 224):
        k = count                                   # the first empty tile
        per = 224 // p
        assert not out["ori_frag"][0, (k // per) * p:(k // per + 1) * p, (k % per) * p:].any()
    _check_image(fragment_ref.absdiff(clip[1, 1], clip[1, 0]), p, 224)


@pytest.mark.parametrize("p,target,count", [(8, 64, 64), (32, 64, 4), (16, 224, 24)])
def test_unaligned_base_pointer(p, target, count):
    """a 64 x 96 clip (aligned rows) whose storage starts at an odd byte: the 16-byte path must not be taken"""
    clip = _clip(2, 64, 96, 5)
    flat = torch.empty(clip.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = _dev(clip).reshape(-1)
    view = flat[1:].view(clip.shape)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    _check_pairs(clip, p, target, expect_count=count, frames_dev=view)


# ---- (d): canvases other than 224 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p,target,count", [
    (250, 333, 32, 96, 9), (256, 512, 32, 96, 9),
    (256, 512, 16, 448, 512),     # 784 slots, 512 patches
    (250, 333, 16, 448, 300),
    (100, 130, 8, 64, 64), (64, 96, 8, 64, 64),
    (250, 333, 8, 448, 1271),     # the largest canvas: 3136 slots
])
def test_other_canvases(h, w, p, target, count):
    clip = _clip(2, h, w, 11)
    _check_pairs(clip, p, target, expect_count=count)
    _check_image(fragment_ref.absdiff(clip[0, 1], clip[0, 0]), p, target)


# ---- (e): top_n -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_n", [0, 1, 100, 784])
def test_top_n_edges(top_n):
    clip = _clip(2, 250, 333, 7)
    out = _run_pairs(clip, 8, 224, top_n)
    for t, ref in enumerate(_ref(2, 250, 333, 7, 8, 224, top_n)):
        _check_against(out, t, ref, 8, 224, top_n)
    if top_n == 0:
        assert not out["ori_frag"].any() and not out["diff_frag"].any()


# ---- (f): ties and the top of the radix range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [8, 32])
def test_ties_take_the_lowest_flat_indices(p):
    h, w = 16 * p, 36 * p + 5                       # 16 x 36 = 576 patches, 49 taken
    a = np.zeros((h, w, 3), np.uint8)
    b = a.copy()
    b[:, :, 0] = 7                                  # every score p * p * 7
    out = _check_pairs(np.stack([a, b])[None], p, 224, top_n=49, expect_count=49)
    assert np.array_equal(out["positions"][0, :49], np.stack(np.divmod(np.arange(49), 36), axis=1))
    # two score values, more patches of the higher one than fit / fewer than fit: the boundary lies inside a tie either way
    g = np.random.default_rng(p)
    for frac in (0.7, 0.02):
        lvl = (g.random((16, 36)) < frac).astype(np.uint8) * 3 + 1
        b = np.zeros_like(a)
        b[:, :36 * p] = np.repeat(np.repeat(lvl, p, 0), p, 1)[..., None]
        _check_pairs(np.stack([a, b])[None], p, 224, top_n=49, expect_count=49)


def test_scores_at_the_top_of_the_radix_range():
    """0 against 255 at P = 32: 32 * 32 * 3 * 255 = 783360, the largest score the two 10-bit levels have to hold"""
    h, w = 8 * 32, 9 * 32 + 16
    a = np.zeros((h, w, 3), np.uint8)
    b = np.full((h, w, 3), 255, np.uint8)
    out = _check_pairs(np.stack([a, b])[None], 32, 224, expect_count=49)
    assert (out["scores"] == 783360).all()
    # full-scale patches among ordinary ones: the selection has to rank 783360 above everything else
    g = np.random.default_rng(3)
    b = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    hot = g.random((8, 9)) < 0.3
    b[:, :9 * 32][np.repeat(np.repeat(hot, 32, 0), 32, 1)] = 255
    out = _check_pairs(np.stack([a, b])[None], 32, 224, top_n=30, expect_count=30)
    assert (np.sort(out["scores"][0].ravel())[-int(hot.sum()):] == 783360).all()


# ---- (g): gather with the caller's positions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,target", [(8, 64), (32, 96), (8, 224)])
def test_gather_gives_zero_tiles_for_out_of_range_positions(p, target):
    h, w = 5 * p + 3, 7 * p + 1
    img = np.random.default_rng(p).integers(1, 256, (2, h, w, 3), dtype=np.uint8)
    slots, per = _slots(p, target), target // p
    pos = np.full((2, slots, 2), -1, np.int32)
    pos[:, 0] = (1, 2)
    pos[:, 1] = (5, 0)                  # y one past the 5 x 7 grid
    pos[:, 2] = (0, 7)                  # x one past it
    pos[:, 3] = (-7, 0)
    pos[:, 4] = (2, 1 << 30)
    pos[:, 5] = (4, 6)                  # the last patch of the grid
    pos[:, 6] = (0, 0)                  # past the count: not copied
    cnt = np.array([6, 6], np.int32)
    got = engine().gather_patches(torch.from_numpy(img).cuda(), torch.from_numpy(pos), torch.from_numpy(cnt), patch_size=p,
                                  target_size=target).cpu().numpy()
    assert got.shape == (2, target, target, 3)
    for t in range(2):
        want = fragment_ref.get_original_frame_patches(img[t], [(1, 2), (4, 6)], p, target)        # tiles 0 and 1 of the oracle ...
        tile = lambda a, k: a[(k // per) * p:(k // per + 1) * p, (k % per) * p:(k % per + 1) * p]  # noqa: E731
        assert np.array_equal(tile(got[t], 0), tile(want, 0)) and np.array_equal(tile(got[t], 5), tile(want, 1))
        rest = got[t].copy()
        tile(rest, 0)[:] = 0
        tile(rest, 5)[:] = 0
        assert not rest.any(), "a tile of an out-of-range position or past the count is not zero"


# ---- (h): the old entry points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(100, 130), (224, 224)])
def test_defaults_equal_the_explicit_16_224_geometry_and_the_oracle(h, w):
    eng = engine()
    clip = _clip(2, h, w, 13)
    dev = _dev(clip)
    old = eng.fragment_pairs(dev, want_scores=True)
    new = eng.fragment_pairs(dev, want_scores=True, patch_size=16, target_size=224)
    for k in old:
        assert old[k].shape == new[k].shape and torch.equal(old[k], new[k]), k
    assert tuple(old["positions"].shape) == (2, 196, 2) and tuple(old["ori_frag"].shape) == (2, 224, 224, 3)
    out = {k: v.cpu().numpy() for k, v in old.items()}
    for t in range(2):
        _check_against(out, t, fragment_ref.fragment_pair(clip[t, 0], clip[t, 1]), 16, 224)
    # the C entry point without the geometry arguments, called as before
    pos = torch.full((2, 196, 2), 7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    ori, diff = torch.empty_like(old["ori_frag"]), torch.empty_like(old["diff_frag"])
    fb = h * w * 3
    rc = eng.lib.relax_fragment_pairs(eng.h, dev.data_ptr(), dev.data_ptr() + fb, 2 * fb, 2, h, w, 196, pos.data_ptr(), cnt.data_ptr(),
                                      ori.data_ptr(), diff.data_ptr(), None, None)
    assert rc == 0
    assert torch.equal(pos, old["positions"]) and torch.equal(cnt, old["counts"])
    assert torch.equal(ori, old["ori_frag"]) and torch.equal(diff, old["diff_frag"])
    img = dev[:, 1].contiguous()
    a, b = eng.fragment_image(img), eng.fragment_image(img, patch_size=16, target_size=224)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(eng.gather_patches(img, old["positions"], old["counts"]),
                       eng.gather_patches(img, old["positions"], old["counts"], patch_size=16, target_size=224))


# ---- (i): error paths -------------------------------------------------------------------------------------------------------------
def test_rejected_geometries_raise_and_launch_nothing():
    eng = engine()
    lib, h = eng.lib, eng.h
    clip = _clip(2, 64, 96, 5)
    dev = _dev(clip)
    for kw, msg in ((dict(patch_size=4), "patch_size=4"), (dict(patch_size=12), "patch_size=12"), (dict(patch_size=64), "patch_size=64"),
                    (dict(patch_size=16, target_size=100), "target_size=100"), (dict(patch_size=32, target_size=480), "target_size=480"),
                    (dict(patch_size=8, target_size=0), "target_size=0")):
        for call in (lambda: eng.fragment_pairs(dev, **kw), lambda: eng.fragment_image(dev[:, 0], **kw),
                     lambda: eng.gather_patches(dev[:, 0], torch.zeros((2, 196, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), **kw)):
            with pytest.raises(ValueError, match=msg):
                call()
    with pytest.raises(RuntimeError, match=r"top_n=50 must be in \[0,49\]"):
        eng.fragment_pairs(dev, top_n=50, patch_size=32)
    with pytest.raises(RuntimeError, match=r"top_n=785 must be in \[0,784\]"):
        eng.fragment_image(dev[:, 0], top_n=785, patch_size=8)
    with pytest.raises(RuntimeError, match=r"top_n=-1"):
        eng.fragment_pairs(dev, top_n=-1, patch_size=8)
    with pytest.raises(ValueError, match="patch_size=12"):
        eng.attention_overlay(dev[:, 0], torch.zeros((2, 196, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 196)),
                              patch_size=12)
    for name in ("extract_clip", "clip_vector", "full_clip_vector", "attention_overlays"):
        with pytest.raises(ValueError, match="out of scope"):
            getattr(eng, name)(dev, target_size=224)
    with pytest.raises(ValueError, match="out of scope"):
        eng.clip_vectors([dev], target_size=448)
    with pytest.raises(ValueError, match="patch_size=12"):
        eng.extract_clip(dev, patch_size=12)

    # the C-ABI itself: RELAX_ERR_INVALID, the offending value in the message, outputs untouched
    fb = 64 * 96 * 3
    pos = torch.full((2, 3136, 2), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    frag = torch.full((2, 448, 448, 3), 7, dtype=torch.uint8, device="cuda")

    def pairs(p, target, top_n):
        return lib.relax_fragment_pairs_ex(h, dev.data_ptr(), dev.data_ptr() + fb, 2 * fb, 2, 64, 96, p, target, top_n, pos.data_ptr(),
                                           cnt.data_ptr(), frag.data_ptr(), None, None, None)

    def image(p, target, top_n):
        return lib.relax_fragment_image_ex(h, dev.data_ptr(), 2 * fb, 2, 64, 96, p, target, top_n, pos.data_ptr(), cnt.data_ptr(),
                                           frag.data_ptr(), None, None)

    def gather(p, target, top_n):
        return lib.relax_gather_patches_ex(h, dev.data_ptr(), 2 * fb, 2, 64, 96, p, target, pos.data_ptr(), cnt.data_ptr(), frag.data_ptr(), None)

    cases = [(4, 224, 1, b"patch_size=4"), (12, 224, 1, b"patch_size=12"), (64, 448, 1, b"patch_size=64"), (33, 33, 1, b"patch_size=33"),
             (0, 224, 1, b"patch_size=0"), (-8, 224, 1, b"patch_size=-8"), (16, 100, 1, b"target_size=100"), (32, 480, 1, b"target_size=480"),
             (8, 456, 1, b"target_size=456"), (8, 0, 0, b"target_size=0"), (16, -224, 0, b"target_size=-224")]
    for fn in (pairs, image, gather):
        for p, target, top_n, msg in cases:
            assert fn(p, target, top_n) == -1, (fn.__name__, p, target)
            assert msg in lib.relax_last_error(h), (fn.__name__, p, target, lib.relax_last_error(h))
    for fn in (pairs, image):
        for p, target, top_n, msg in ((32, 224, 50, b"top_n=50"), (8, 224, 785, b"top_n=785"), (16, 448, -1, b"top_n=-1")):
            assert fn(p, target, top_n) == -1 and msg in lib.relax_last_error(h), (fn.__name__, p, target, top_n)
    assert b"radix" in (pairs(64, 448, 1), lib.relax_last_error(h))[1]
    vals = torch.zeros((2, 3136), device="cuda")
    lut = torch.from_numpy(LUT).cuda()
    for p, slots, msg in ((12, 196, b"patch_size=12"), (64, 49, b"patch_size=64"), (8, 0, b"slots=0"), (8, 3137, b"slots=3137")):
        rc = lib.relax_attention_overlay_ex(h, dev.data_ptr(), 2 * fb, 2, 64, 96, p, slots, pos.data_ptr(), cnt.data_ptr(), vals.data_ptr(),
                                            lut.data_ptr(), frag.data_ptr(), None)
        assert rc == -1 and msg in lib.relax_last_error(h), (p, slots, lib.relax_last_error(h))
    torch.cuda.synchronize()
    assert (pos == 7).all() and (cnt == 7).all() and (frag == 7).all(), "a rejected call wrote to its outputs"
    # and the engine works afterwards
    _check_pairs(clip, 8, 64, expect_count=64)


# ---- (j): overlay -----------------------------------------------------------------------------------------------------------------
def _load8(name):
    """synthetic patch-8 weights into the shared engine (keyed as tests/test_gpu_vit_patch8.py keys them in the shared cache)"""
    sd = _weights8(name)
    key = f"vit8:{name}:False"
    if gpu_common._weights.get("vit_loaded") != key:
        engine().load_vit(sd, name)
        gpu_common._weights["vit_loaded"] = key
    return sd


@functools.lru_cache(maxsize=None)
def _weights8(name):
    return synth.vit_state_dict(name, patch=8)


def _restated_overlay(frame, values, positions, n, p):
    """tests.vit_attention_restated.map_attention_to_original on the first n slots.  The reference is undefined for a negative value
    (a negative float cast to uint8) and for NaN (np.max gives NaN); the header states the engine's choice - such a slot paints level
    0 and does not take part in the maximum, which always includes 0 here (H, W are not multiples of P) - and that is the
    transcription fed with 0 in their place."""
    v = np.asarray(values[:n], dtype=np.float32).copy()
    v[np.isnan(v) | (v < 0)] = 0.0
    return var.map_attention_to_original(frame, v, positions[:n], p, LUT)


@pytest.mark.parametrize("h,w", [(100, 130), (250, 333), (70, 80), (72, 112)])
@pytest.mark.parametrize("p", [8, 32])
def test_overlay_matches_the_restatement(h, w, p):
    """100 x 130 / 250 x 333: one thread per pixel; 70 x 80 / 72 x 112 (W % 16 == 0): the 16-pixel kernel - two patches per thread
    at P = 8, half a patch at P = 32 with 16 columns past the last whole patch"""
    eng = engine()
    if p == 8:
        _load8("vit_tiny")          # (a patch-16 model would refuse 8 x 8 slots; 32 goes with whatever is loaded)
    T = 2
    clip = _clip(T, h, w, 17)
    dev = _dev(clip)
    fr = eng.fragment_pairs(dev, top_n=None, patch_size=p)
    slots = _slots(p, 224)
    pos = fr["positions"].cpu().numpy().copy()
    cnt = fr["counts"].cpu().numpy().copy()
    g = np.random.default_rng(h + p)
    vals = g.random((T, slots)).astype(np.float32)
    for t in range(T):
        n = int(cnt[t])
        assert n >= 4
        if n < slots:               # room for two more slots: a duplicate of slot 1 (the later one wins) and one outside the grid
            dup, oor = n, n + 1
            cnt[t] = n + 2
            pos[t, oor] = (h // p, 0)
        else:
            dup, oor = n - 1, n - 2
            pos[t, oor] = (0, w // p)
        pos[t, dup] = pos[t, 1]
        vals[t, 0] = -0.5
        vals[t, 2] = np.nan
        vals[t, oor] = 50.0         # the out-of-range slot would set the maximum if it were painted
    got = eng.attention_overlay(dev[:, 0], torch.from_numpy(pos), torch.from_numpy(cnt), torch.from_numpy(vals), patch_size=p).cpu().numpy()
    for t in range(T):
        want = _restated_overlay(clip[t, 0], vals[t], pos[t], int(cnt[t]), p)
        assert np.array_equal(got[t], want), f"frame {t}: {int((got[t] != want).any(axis=-1).sum())} pixels differ"
    # strided frames (the first of every pair) against a packed copy
    assert np.array_equal(got, eng.attention_overlay(dev[:, 0].contiguous(), pos, cnt, vals, patch_size=p).cpu().numpy())


def test_overlay_rule_between_fragment_patch_and_vit_patch():
    eng = engine()
    clip = _dev(_clip(2, 100, 130, 17))
    _load8("vit_tiny")
    with pytest.raises(ValueError, match="patch size 8"):
        eng.attention_overlays(clip, patch_size=16)
    gpu_common.vit_weights("vit_tiny")
    with pytest.raises(ValueError, match=r"patch size is 8.*patch size 16"):
        eng.attention_overlays(clip, patch_size=8)
    # 32 x 32 slots under a patch-16 model: the mean of the 2 x 2 tokens' head-mean attention
    out = eng.attention_overlays(clip, patch_size=32)
    assert tuple(out["patch_means"].shape) == (2, 49) and tuple(out["attention"].shape) == (2, 3, 196)
    hm = out["attention"].mean(dim=1).cpu().numpy().reshape(2, 7, 2, 7, 2)
    want = np.stack([demo_visual.get_activation_png(np.repeat(np.repeat(a.reshape(1, 14, 14), 16, 1), 16, 2), "frame_diff", 32)
                     for a in out["attention"].mean(dim=1).cpu().numpy()]).reshape(2, 49)
    np.testing.assert_allclose(out["patch_means"].cpu().numpy(), want, rtol=1e-5)
    np.testing.assert_allclose(out["patch_means"].cpu().numpy(), hm.mean(axis=(2, 4)).reshape(2, 49), rtol=1e-5)
    pos, cnt, pm = out["positions"].cpu().numpy(), out["counts"].cpu().numpy(), out["patch_means"].cpu().numpy()
    frames = clip[:, 0].cpu().numpy()
    for t in range(2):
        assert np.array_equal(out["overlay"][t].cpu().numpy(), _restated_overlay(frames[t], pm[t], pos[t], int(cnt[t]), 32))


# ---- (k): end to end, synthetic weights -------------------------------------------------------------------------------------------
def test_patch8_model_end_to_end():
    eng = engine()
    gpu_common.rn50_weights()
    _load8("vit_small")
    T, h, w = 2, 250, 333
    clip = _clip(T, h, w, 7)
    dev = _dev(clip)
    out = eng.attention_overlays(dev, patch_size=8)
    assert tuple(out["patch_means"].shape) == (T, 784) and tuple(out["attention"].shape) == (T, 6, 784)
    assert tuple(out["positions"].shape) == (T, 784, 2) and (out["counts"].cpu().numpy() == 784).all()
    pm, pos = out["patch_means"].cpu().numpy(), out["positions"].cpu().numpy()
    for t, ref in enumerate(_ref(T, h, w, 7, 8, 224, 784)):
        assert np.array_equal(pos[t], ref["positions"])
        want = _restated_overlay(clip[t, 0], pm[t], pos[t], 784, 8)
        assert np.array_equal(out["overlay"][t].cpu().numpy(), want), f"frame {t}"
    for p, top_n in ((8, 784), (32, 49)):
        refs = _ref(T, h, w, 7, p, 224, top_n)
        both = torch.from_numpy(np.stack([r["ori_frag"] for r in refs] + [r["diff_frag"] for r in refs])).cuda()
        got = eng.extract_clip(dev, patch_size=p, top_n=top_n)
        assert tuple(got["positions"].shape) == (T, top_n, 2)
        ls, pool = eng.resnet50_clip_features(both, T)
        assert torch.equal(got["resnet"], torch.cat([ls, pool], dim=1)), f"P = {p}: ResNet-50 rows"
        _, pooled = eng.vit_features(both, tokens=False, pooled=True)
        assert torch.equal(got["vit"], torch.cat([pooled[:T], pooled[T:]], dim=1)), f"P = {p}: ViT rows"
        rows = eng.clip_vectors([dev], patch_size=p, top_n=top_n)
        assert tuple(rows.shape) == (1, got["resnet"].shape[1] + got["vit"].shape[1])


# ---- the reference-named functions ------------------------------------------------------------------------------------------------
def test_reference_named_functions_at_other_geometries(monkeypatch):
    monkeypatch.setattr(runtime, "get_engine", lambda device=None: engine())
    clip = _clip(2, 100, 130, 17)
    o, n = clip[0, 0], clip[0, 1]
    residual = fragment_ref.absdiff(n, o)
    for p, target, top_n in ((8, 224, 784), (32, 224, 49), (32, 96, 5), (16, 448, 784)):
        ref = fragment_ref.fragment_pair(o, n, p, target, top_n)
        assert np.array_equal(ml.get_patch_diff(residual, p), ref["score"])
        frag, pos = ml.extract_important_patches(residual, None, p, target, top_n)
        assert np.array_equal(frag, ref["diff_frag"]) and pos == [tuple(x) for x in ref["positions"].tolist()]
        assert np.array_equal(ml.get_original_frame_patches(o, pos, p, target), ref["ori_frag"])
        d, of, pos2 = ml.fragment_pair(o, n, top_n, None, p, target)
        assert np.array_equal(d, ref["diff_frag"]) and np.array_equal(of, ref["ori_frag"]) and pos2 == pos
    pos = [tuple(x) for x in fragment_ref.fragment_pair(o, n, 32, 224, 49)["positions"].tolist()]
    vals = np.random.default_rng(4).random(len(pos)).astype(np.float32)
    assert np.array_equal(demo_visual.map_attention_to_original(o, vals, pos, 32), var.map_attention_to_original(o, vals, pos, 32, LUT))
