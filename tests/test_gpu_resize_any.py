"""relax_resize_frames_ex / relax_resize_residual_ex (csrc/resize.hip) and the engine methods on them: the resize to any output size,
bit for bit against oracle/resize_ref.resize (pinned to Pillow at the same cases in tests/test_resize_any_cpu.py) - down, up, mixed, with
either pass or both skipped, on the 16-byte and the bytewise row path, into guarded buffers, from strided items -, the 224 entries on the
same kernels (both entries against the oracle at 224 x 224, their widest rows, the table cache turning over under them), the residual form
against the plain one on the torch-made difference, the refusals, and whole_frame_vit_canvas."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import fragment_ref, resize_ref
from relax_vqa_amd.engine import _ptr, _stream
from tests import resize_any_cases as cases
from tests.gpu_common import engine, rn50_weights, vit_weights

pytestmark = pytest.mark.gpu

GUARD = 64          # bytes of 0xA5 on either side of an output (a multiple of 16: the guarded output keeps its alignment)
MAX_OUT, MAX_IN_W = 2048, 8192
_ids = [f"{h}x{w}-{oh}x{ow}" for (h, w), (oh, ow), _ in cases.CASES]


def _guarded(n, oh, ow):
    size = n * oh * ow * 3
    buf = torch.full((2 * GUARD + size,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + size].view(n, oh, ow, 3)


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()     # (a copy: the shared cases are read-only)


def _strided(frames):
    """the frames as clip[:, 0] of a [N,2,H,W,3] device tensor whose other half is 0x5A"""
    clip = torch.full((frames.shape[0], 2) + frames.shape[1:], 0x5A, dtype=torch.uint8, device="cuda")
    clip[:, 0] = _dev(frames)
    return clip[:, 0]


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} bytes differ"


@pytest.mark.parametrize("hw,out,n", cases.CASES, ids=_ids)
def test_bit_equal_to_the_oracle(hw, out, n):
    view = _strided(cases.frames(hw, n))
    want = [cases.reference(hw, out, n, f) for f in (resize_ref.BILINEAR, resize_ref.LANCZOS)]
    bb, vb = _guarded(n, *out)
    bl, vl = _guarded(n, *out)
    gb, gl = engine().resize_frames_to(view, out, out_bilinear=vb, out_lanczos=vl)
    assert gb is vb and gl is vl
    _same(vb, want[0], "bilinear")
    _same(vl, want[1], "lanczos")
    assert _guards_intact(bb) and _guards_intact(bl), "bytes outside an output were written"
    # one filter at a time: the same bytes, and the buffer offered for the other one keeps its sentinel
    for k, name in ((0, "bilinear"), (1, "lanczos")):
        bufs = [_guarded(n, *out), _guarded(n, *out)]
        got = engine().resize_frames_to(view, out, bilinear=k == 0, lanczos=k == 1, out_bilinear=bufs[0][1], out_lanczos=bufs[1][1])
        assert got[k] is bufs[k][1] and got[1 - k] is None
        _same(bufs[k][1], want[k], name + " alone")
        assert bool((bufs[1 - k][0] == 0xA5).all()), f"the other buffer was written with {name} alone"
        assert _guards_intact(bufs[k][0])


def test_base_one_byte_off_takes_the_bytewise_path():
    hw, out, n = (40, 64), (24, 40), 2
    frames = cases.frames(hw, n)
    buf = torch.empty(1 + frames.size, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(frames.shape)
    view.copy_(_dev(frames))
    assert view.data_ptr() % 16 == 1 and view.is_contiguous() and hw[1] * 3 % 16 == 0
    gb, gl = engine().resize_frames_to(view, out)
    _same(gb, cases.reference(hw, out, n, resize_ref.BILINEAR), "bilinear")
    _same(gl, cases.reference(hw, out, n, resize_ref.LANCZOS), "lanczos")


def test_the_shorter_side_rule():
    hw, n = (135, 240), 2
    eng = engine()
    assert eng.resize_output_size(135, 240, 68) == (68, 120)
    gb, gl = eng.resize_frames_to(_dev(cases.frames(hw, n)), 68)
    _same(gb, cases.reference(hw, (68, 120), n, resize_ref.BILINEAR), "bilinear")
    _same(gl, cases.reference(hw, (68, 120), n, resize_ref.LANCZOS), "lanczos")


@pytest.mark.parametrize("hw", [(20, 16), (270, 480)], ids=["20x16", "270x480"])
def test_equals_the_224_kernels_at_224(hw):
    """resize_frames and resize_frames_to(..., (224, 224)) reach the same kernels through two entries: each equals the oracle, and
    they equal each other."""
    frames = _strided(cases.frames(hw, 2))
    eng = engine()
    wb, wl = eng.resize_frames(frames)
    gb, gl = eng.resize_frames_to(frames, (224, 224))
    for filt, name, w, g in ((resize_ref.BILINEAR, "bilinear", wb, gb), (resize_ref.LANCZOS, "lanczos", wl, gl)):
        want = cases.reference(hw, (224, 224), 2, filt)
        _same(w, want, f"resize_frames {name}")
        _same(g, want, f"resize_frames_to {name}")
    assert torch.equal(gb, wb) and torch.equal(gl, wl)


@pytest.mark.parametrize("w", cases.WIDEST_224, ids=["5456-16-byte-rows", "5461-bytewise-lds-opt-in"])
def test_widest_rows_of_the_224_entries(w):
    """The last widths relax_resize_frames / relax_resize_residual take: 5456 (16-byte rows, 4 * 16368 + 32 bytes of LDS, the last
    width under 64 KiB) and 5461 (bytewise rows, 4 * 16384 + 32 bytes: the dynamic-LDS opt-in).  H = 5: two workgroups, the second
    with one row."""
    hw, n = (5, w), 2
    assert (w * 3 % 16 == 0) == (w == 5456)
    orig = cases.frames(hw, n)
    nxt = np.random.default_rng(w).integers(0, 256, orig.shape, dtype=np.uint8)
    diff = fragment_ref.absdiff(nxt, orig)
    pairs = torch.from_numpy(np.stack([orig, nxt], axis=1)).cuda()
    eng = engine()
    bufs = [_guarded(n, 224, 224) for _ in range(4)]
    eng.resize_frames(pairs[:, 0], out_bilinear=bufs[0][1], out_lanczos=bufs[1][1])
    _, _, gr = eng.residual_resize(pairs, want_residual=True, out_bilinear=bufs[2][1], out_lanczos=bufs[3][1])
    for k, filt in enumerate((resize_ref.BILINEAR, resize_ref.LANCZOS)):
        _same(bufs[k][1], cases.reference(hw, (224, 224), n, filt), f"resize_frames filter {filt}")
        _same(bufs[2 + k][1], np.stack([resize_ref.resize(d, 224, 224, filt) for d in diff]), f"residual_resize filter {filt}")
    _same(gr, diff, "residual image")
    assert all(_guards_intact(b) for b, _ in bufs), "bytes outside an output were written"


def test_table_eviction_under_the_224_entries():
    """Nine shapes ask for 36 tables of the 16 the handle caches; the first shape, whose tables have gone by then, comes back right."""
    eng = engine()
    shapes = [(10 + i, 20 + i) for i in range(9)]
    for hw in shapes + shapes[:1]:
        gb, gl = eng.resize_frames(_dev(cases.frames(hw, 1)))
        _same(gb, cases.reference(hw, (224, 224), 1, resize_ref.BILINEAR), f"bilinear {hw}")
        _same(gl, cases.reference(hw, (224, 224), 1, resize_ref.LANCZOS), f"lanczos {hw}")


# down | vertical skipped | horizontal skipped (the difference goes through the workspace) | copy | 16-byte rows | several workgroups
RESIDUAL_CASES = [((37, 53), (16, 30)), ((37, 53), (37, 20)), ((37, 53), (50, 53)), ((33, 60), (33, 60)), ((40, 64), (24, 40)),
                  ((135, 240), (68, 120))]


@pytest.mark.parametrize("hw,out", RESIDUAL_CASES, ids=[f"{h}x{w}-{oh}x{ow}" for (h, w), (oh, ow) in RESIDUAL_CASES])
def test_residual_form_equals_the_plain_one_on_the_difference(hw, out):
    t = 3
    g = np.random.default_rng(hw[0] + 7 * out[1])
    pairs = torch.from_numpy(g.integers(0, 256, (t, 2) + hw + (3,), dtype=np.uint8)).cuda()
    a, b = pairs[:, 0].to(torch.int16), pairs[:, 1].to(torch.int16)
    diff = (b - a).abs().to(torch.uint8).contiguous()
    eng = engine()
    wb, wl = eng.resize_frames_to(diff, out)
    gb, gl, gr = eng.residual_resize(pairs, want_residual=True, size=out)
    assert torch.equal(gr, diff), "residual image"
    assert torch.equal(gb, wb) and torch.equal(gl, wl)
    # without the residual image, one filter; and the residual image alone
    gb2, gl2, gr2 = eng.residual_resize(pairs, bilinear=False, size=out)
    assert gb2 is None and gr2 is None and torch.equal(gl2, wl)
    gb3, gl3, gr3 = eng.residual_resize(pairs, bilinear=False, lanczos=False, want_residual=True, size=out)
    assert gb3 is None and gl3 is None and torch.equal(gr3, diff)


def test_refusals_name_the_value():
    eng = engine()
    h, w = 8, 12
    frames = torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((2, 16, 16, 3), dtype=torch.uint8, device="cuda")

    def frames_ex(fr, n, hh, ww, oh, ow, ob, ol):
        eng._check(eng.lib.relax_resize_frames_ex(eng.h, _ptr(fr), hh * ww * 3, n, hh, ww, oh, ow, _ptr(ob), _ptr(ol), _stream()),
                   "relax_resize_frames_ex")

    def residual_ex(oh, ow, ob, ol, res):
        eng._check(eng.lib.relax_resize_residual_ex(eng.h, _ptr(frames[:1]), _ptr(frames[1:]), h * w * 3, 1, h, w, oh, ow, _ptr(ob), _ptr(ol),
                                                    _ptr(res), _stream()), "relax_resize_residual_ex")

    with pytest.raises(RuntimeError, match="out_h=0 "):
        frames_ex(frames, 2, h, w, 0, 16, out, None)
    with pytest.raises(RuntimeError, match=f"out_w={MAX_OUT + 1} "):
        frames_ex(frames, 2, h, w, 16, MAX_OUT + 1, out, None)
    with pytest.raises(RuntimeError, match=f"out_h={MAX_OUT + 1} "):
        residual_ex(MAX_OUT + 1, 16, out, None, None)
    wide = torch.zeros((1, 1, MAX_IN_W + 1, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=f"W={MAX_IN_W + 1} too wide"):
        frames_ex(wide, 1, 1, MAX_IN_W + 1, 16, 16, out, None)
    with pytest.raises(RuntimeError, match="no output requested"):
        frames_ex(frames, 2, h, w, 16, 16, None, None)
    with pytest.raises(RuntimeError, match="no output requested"):
        residual_ex(16, 16, None, None, None)
    with pytest.raises(RuntimeError, match="N=0"):
        frames_ex(frames, 0, h, w, 16, 16, out, None)
    with pytest.raises(RuntimeError, match="size=0 "):
        eng.resize_output_size(h, w, 0)
    with pytest.raises(ValueError):
        eng.resize_frames_to(frames, (16, 16), out_bilinear=torch.empty((2, 16, 15, 3), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


def test_whole_frame_vit_canvas_is_vit_features_on_the_pillow_resize():
    vit_weights("vit_tiny")
    eng = engine()
    frames = np.array(cases.frames((135, 240), 2))
    oh, ow = eng.resize_output_size(135, 240, 64)
    assert (oh, ow) == (64, 113)
    host = np.stack([np.asarray(Image.fromarray(f).resize((ow, oh), Image.LANCZOS)) for f in frames])
    want_tk, want_pl = eng.vit_features(torch.from_numpy(host).cuda(), tokens=True, pooled=True)
    tk, pl = eng.whole_frame_vit_canvas(frames, 64, tokens=True, pooled=True)
    assert tuple(tk.shape) == (2, 4 * 7, eng.vit_dim)
    assert torch.equal(tk, want_tk) and torch.equal(pl, want_pl)


def test_whole_frame_vit_canvas_at_224_is_whole_frame_features():
    rn50_weights()
    vit_weights("vit_tiny")
    eng = engine()
    frames = _dev(cases.frames((135, 240), 2))
    _, want = eng.whole_frame_features(frames)
    _, got = eng.whole_frame_vit_canvas(frames, (224, 224))
    assert torch.equal(got, want)


def test_whole_residual_features_on_a_vit_canvas():
    """vit_size: the ViT rows are vit_features of the LANCZOS difference image at that size; None is the 224 call."""
    vit_weights("vit_tiny")
    eng = engine()
    g = np.random.default_rng(5)
    pairs = torch.from_numpy(g.integers(0, 256, (2, 2, 135, 240, 3), dtype=np.uint8)).cuda()
    lan = eng.residual_resize(pairs, bilinear=False, size=64)[1]
    want = eng.vit_features(lan)[1]
    got = eng.whole_residual_features(pairs, resnet=False, vit=True, vit_size=64)
    assert list(got) == ["vit"] and torch.equal(got["vit"], want)
    base = eng.whole_residual_features(pairs, resnet=False, vit=True)
    assert torch.equal(base["vit"], eng.whole_residual_features(pairs, resnet=False, vit=True, vit_size=None)["vit"])
