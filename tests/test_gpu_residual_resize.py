"""relax_resize_residual (csrc/resize.hip): the whole frame difference |next - orig| of a pair, resized to 224 x 224 the way Pillow
does it, with the difference taken while the rows are staged.  Everything is bit-exact: against Pillow on the host-made difference
image (oracle/fragment_ref.absdiff), against relax_resize_frames on the device-made one, on both pair layouts, on the bytewise path
of a misaligned view, for every subset of the three outputs, at the extremes of the byte range; the refusals are refused on the host."""
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import fragment_ref
from relax_vqa_amd.engine import _ptr, _stream
from tests.gpu_common import engine

pytestmark = pytest.mark.gpu

# (H, W): upscale + unaligned rows | unaligned rows, H % 4 != 0 | identity tables | aligned W, odd H | aligned downscales | the workload's row
SHAPES = [(100, 130), (250, 333), (224, 224), (301, 224), (270, 480), (540, 960), (1080, 1920)]
_cases = {}


def _case(h, w):
    """T pairs [T,2,H,W,3] of seeded random bytes (half of one frame quantised to multiples of 16, as test_gpu_resize.py does), the
    host-made difference images and their two Pillow resizes; made once per shape and never written to."""
    if (h, w) not in _cases:
        t = 1 if h * w > 2e6 else 3
        g = np.random.default_rng(h + 3 * w)
        frames = g.integers(0, 256, (t, 2, h, w, 3), dtype=np.uint8)
        frames[0, 0, : h // 2] = frames[0, 0, : h // 2] // 16 * 16
        d = fragment_ref.absdiff(frames[:, 1], frames[:, 0])
        bil = np.stack([np.asarray(Image.fromarray(d[i]).resize((224, 224), Image.BILINEAR)) for i in range(t)])
        lan = np.stack([np.asarray(Image.fromarray(d[i]).resize((224, 224), Image.LANCZOS)) for i in range(t)])
        _cases[(h, w)] = (frames, d, bil, lan)
    return _cases[(h, w)]


def _raw(orig, nxt, pair_stride, t, h, w, out_bilinear=None, out_lanczos=None, residual=None):
    eng = engine()
    rc = eng.lib.relax_resize_residual(eng.h, _ptr(orig), _ptr(nxt), pair_stride, t, h, w, _ptr(out_bilinear), _ptr(out_lanczos),
                                       _ptr(residual), _stream())
    eng._check(rc, "relax_resize_residual")


def _same(got, want, what):
    assert np.array_equal(got.cpu().numpy(), want), what


@pytest.mark.parametrize("h,w", SHAPES)
def test_matches_pillow_on_the_host_made_difference(h, w):
    frames, d, bil, lan = _case(h, w)
    gb, gl, gr = engine().residual_resize(torch.from_numpy(frames).cuda(), want_residual=True)
    assert tuple(gb.shape) == tuple(gl.shape) == (frames.shape[0], 224, 224, 3) and tuple(gr.shape) == d.shape
    _same(gr, d, "residual image")
    for i in range(frames.shape[0]):
        _same(gb[i], bil[i], f"bilinear pair {i}")
        _same(gl[i], lan[i], f"lanczos pair {i}")


@pytest.mark.parametrize("h,w", [(224, 300), (301, 224), (224, 224)])
def test_skipped_passes_at_224(h, w):
    """A side that is already 224 has no pass, as in Pillow: H == 224 - the horizontal pass writes the outputs; W == 224 - the difference
    goes through the workspace once and serves both filters' vertical passes; both - the outputs are the difference image."""
    t = 2
    frames = np.random.default_rng(7 * h + w).integers(0, 256, (t, 2, h, w, 3), dtype=np.uint8)
    d = fragment_ref.absdiff(frames[:, 1], frames[:, 0])
    gb, gl, gr = engine().residual_resize(torch.from_numpy(frames).cuda(), want_residual=True)
    _same(gr, d, "residual image")
    for i in range(t):
        img = Image.fromarray(d[i])
        _same(gb[i], np.asarray(img.resize((224, 224), Image.BILINEAR)), f"bilinear pair {i}")
        _same(gl[i], np.asarray(img.resize((224, 224), Image.LANCZOS)), f"lanczos pair {i}")


@pytest.mark.parametrize("h,w", [(250, 333), (270, 480)])
def test_separate_orig_and_next_tensors(h, w):
    """pair_stride = one frame: orig and next are two [T,H,W,3] tensors, not the interleaved [T,2,H,W,3] one."""
    frames, d, bil, lan = _case(h, w)
    t = frames.shape[0]
    orig = torch.from_numpy(np.ascontiguousarray(frames[:, 0])).cuda()
    nxt = torch.from_numpy(np.ascontiguousarray(frames[:, 1])).cuda()
    gb, gl = (torch.empty((t, 224, 224, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    gr = torch.empty((t, h, w, 3), dtype=torch.uint8, device="cuda")
    _raw(orig, nxt, h * w * 3, t, h, w, gb, gl, gr)
    _same(gb, bil, "bilinear")
    _same(gl, lan, "lanczos")
    _same(gr, d, "residual")


def test_misaligned_view_takes_the_bytewise_path():
    """W * 3 % 16 == 0, but the pairs start one byte into a buffer: same bytes through the bytewise loads."""
    h, w = 270, 480
    frames, d, bil, lan = _case(h, w)
    buf = torch.empty(1 + frames.size, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(frames.shape)
    view.copy_(torch.from_numpy(frames))
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    gb, gl, gr = engine().residual_resize(view, want_residual=True)
    _same(gb, bil, "bilinear")
    _same(gl, lan, "lanczos")
    _same(gr, d, "residual")
    # ... and a misaligned residual output alone sends an aligned pair down the same path
    out = torch.empty(1 + d.size, dtype=torch.uint8, device="cuda")
    res = out[1:].view(d.shape)
    aligned = torch.from_numpy(frames).cuda()
    _raw(aligned[:, 0], aligned[:, 1], 2 * h * w * 3, frames.shape[0], h, w, residual=res)
    _same(res, d, "misaligned residual output")


@pytest.mark.parametrize("want", [s for s in itertools.product([False, True], repeat=3) if any(s)],
                         ids=lambda s: "".join(n for n, on in zip("blr", s) if on))
def test_every_subset_of_the_outputs(want):
    """Requested outputs carry the expected bytes; a buffer offered for an output that is not requested keeps its sentinel."""
    h, w = 250, 333
    frames, d, bil, lan = _case(h, w)
    t = frames.shape[0]
    wb, wl, wr = want
    bb, bl = (torch.full((t, 224, 224, 3), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    gb, gl, gr = engine().residual_resize(torch.from_numpy(frames).cuda(), bilinear=wb, lanczos=wl, want_residual=wr,
                                          out_bilinear=bb, out_lanczos=bl)
    assert (gb is not None, gl is not None, gr is not None) == want
    for on, got, buf, exp, name in ((wb, gb, bb, bil, "bilinear"), (wl, gl, bl, lan, "lanczos")):
        if on:
            assert got is buf
            _same(buf, exp, name)
        else:
            assert bool((buf == 0xA5).all()), f"{name} buffer was written although not requested"
    if wr:
        _same(gr, d, "residual")


@pytest.mark.parametrize("h,w", [(100, 130), (270, 480)])
def test_equal_frames_give_zero_and_full_range_gives_255(h, w):
    """next == orig -> every output 0; orig = 0, next = 255 -> every output 255 (the tap sums stay inside 32 bits and clip8)."""
    g = np.random.default_rng(7)
    one = torch.from_numpy(g.integers(0, 256, (2, 1, h, w, 3), dtype=np.uint8)).cuda()
    for out in engine().residual_resize(torch.cat([one, one], dim=1).contiguous(), want_residual=True):
        assert int(out.max()) == 0
    ext = torch.zeros((2, 2, h, w, 3), dtype=torch.uint8, device="cuda")
    ext[:, 1] = 255
    for out in engine().residual_resize(ext, want_residual=True):
        assert int(out.min()) == 255


@pytest.mark.parametrize("h,w", [(250, 333), (540, 960)])
def test_equals_resize_frames_on_the_residual(h, w):
    frames, _, _, _ = _case(h, w)
    eng = engine()
    gb, gl, gr = eng.residual_resize(torch.from_numpy(frames).cuda(), want_residual=True)
    fb, fl = eng.resize_frames(gr)
    assert torch.equal(gb, fb) and torch.equal(gl, fl)


def test_refusals_are_made_on_the_host():
    h, w = 32, 48
    fb = h * w * 3
    frames = torch.zeros((2, 2, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((2, 224, 224, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="no output requested"):
        _raw(frames[:, 0], frames[:, 1], 2 * fb, 2, h, w)
    with pytest.raises(RuntimeError, match="bad arguments"):
        _raw(frames[:, 0], frames[:, 1], 2 * fb, 0, h, w, out)
    with pytest.raises(RuntimeError, match="bad arguments"):
        _raw(frames[:, 0], None, 2 * fb, 2, h, w, out)
    with pytest.raises(RuntimeError, match="pair stride smaller than a frame"):
        _raw(frames[:, 0], frames[:, 1], fb - 1, 2, h, w, out)
    with pytest.raises(RuntimeError, match="W=6000 too wide"):
        engine().residual_resize(torch.zeros((1, 2, 2, 6000, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        engine().residual_resize(torch.zeros((2, 3, h, w, 3), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
