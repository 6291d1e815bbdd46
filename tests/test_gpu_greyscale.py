"""The greyscale screen on the GPU (csrc/greyscale.hip: relax_greyscale_scan, relax_yuv_greyscale_scan; RelaxEngine.greyscale_scan,
yuv_greyscale_scan; data_processing/check_greyscale.py) against the numpy statement of the rule (tests/greyscale_cases.py) and, for
the fused YUV scan, against relax_greyscale_scan on relax_yuv_to_bgr's output.  Everything is an integer: every comparison exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from relax_vqa_amd import _lib, metrics, sampling
from relax_vqa_amd.data_processing import check_greyscale
from tests import greyscale_cases as cases
from tests.gpu_common import engine

pytestmark = pytest.mark.gpu

PRESET = 0x7f


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scan(buf, first, stride, N, H, W, expect_rc=0):
    """relax_greyscale_scan on frames at buf[first + n * stride], into records that held 0x7f bytes -> host int32 [N,8]."""
    lib = _lib.load()
    out = torch.full((max(N, 1) * cases.WORDS * 4,), PRESET, dtype=torch.uint8, device="cuda")
    rc = lib.relax_greyscale_scan(C.c_void_p(buf.data_ptr() + first), stride, N, H, W, C.c_void_p(out.data_ptr()), _stream())
    assert rc == expect_rc, lib.relax_last_error(None).decode()
    rec = out.cpu().numpy().view(np.int32).reshape(-1, cases.WORDS)
    return rec if expect_rc else rec[:N]


def _aligned(nbytes, off=0):
    """A device byte buffer whose element `off` lies at a 16-byte-aligned address."""
    raw = torch.zeros(nbytes + 32, dtype=torch.uint8, device="cuda")
    shift = (-(raw.data_ptr() + off)) % 16
    return raw[shift:shift + nbytes]


@pytest.mark.parametrize("H,W", cases.SIZES)
def test_bgr_scan_equals_the_rule_aligned_off_by_one_and_in_padded_slots(H, W):
    slot = H * W * 3
    for near in (True, False):
        frames = cases.random_frames(3 + H * W, 5, H, W, near_grey=near)
        want = cases.records(frames)
        got = engine().greyscale_scan(torch.from_numpy(frames).cuda())
        assert np.array_equal(got["records"].cpu().numpy(), want), (H, W, near)
        assert np.array_equal(got.is_greyscale().cpu().numpy(), cases.is_greyscale(want))
        assert np.array_equal(got.is_greyscale(mode="abs").cpu().numpy(), cases.is_greyscale(want, mode="abs"))
        assert np.array_equal(got.is_greyscale(threshold=1).cpu().numpy(), cases.is_greyscale(want, threshold=1))
        for pad in (0, 7, 16):
            for first in (0, 1):                                   # frame 0 at an aligned address, then one byte behind it
                buf = _aligned(first + 5 * (slot + pad), 0)
                host = np.full(buf.numel(), 0xEE, np.uint8)
                for n in range(5):
                    host[first + n * (slot + pad):first + n * (slot + pad) + slot] = frames[n].reshape(-1)
                buf.copy_(torch.from_numpy(host))
                a = _scan(buf, first, slot + pad, 5, H, W)
                assert np.array_equal(a, want), (H, W, near, pad, first)
                assert np.array_equal(_scan(buf, first, slot + pad, 5, H, W), a)          # a second call: the same bits


def test_clip_tensor_its_views_and_single_channel_frames():
    eng = engine()
    for H, W in ((6, 48), (7, 50)):
        frames = cases.random_frames(41, 8, H, W)
        clip = torch.from_numpy(frames.reshape(4, 2, H, W, 3)).cuda()
        want = cases.records(frames)
        assert np.array_equal(eng.greyscale_scan(clip)["records"].cpu().numpy(), want)
        assert np.array_equal(eng.greyscale_scan(clip[1:3])["records"].cpu().numpy(), want[2:6])
        assert np.array_equal(eng.greyscale_scan(clip[:, 1])["records"].cpu().numpy(), want[1::2])      # stride of two slots
        assert np.array_equal(eng.greyscale_scan(clip[2, 0:1])["records"].cpu().numpy(), want[4:5])
        assert np.array_equal(eng.greyscale_scan(frames)["wrapped"].cpu().numpy(), want[:, 0:3])          # a host array is uploaded
        res = eng.greyscale_scan(clip)
        assert np.array_equal(res["abs"].cpu().numpy(), want[:, 3:6]) and not res["status"].any()
        assert check_greyscale.is_greyscale_image(clip[0, 1]) == bool(cases.is_greyscale(want[1]))
        assert check_greyscale.is_greyscale_image(clip[0, 0]) == bool(cases.is_greyscale(want[0]))
        with pytest.raises(ValueError, match="packed rows"):
            eng.greyscale_scan(clip[:, :, :, ::2])
    gray = eng.greyscale_scan(torch.randint(0, 256, (3, 5, 7), dtype=torch.uint8, device="cuda"))
    assert tuple(gray["records"].shape) == (3, 8) and not gray["records"].any() and gray.is_greyscale().all()


@pytest.mark.parametrize("H,W", cases.SIZES)
def test_single_pixel_cases(H, W):
    frames, which = cases.single_pixel_frames(H, W)
    want = cases.records(frames)
    got = engine().greyscale_scan(torch.from_numpy(frames).cuda())
    assert np.array_equal(got["records"].cpu().numpy(), want)
    ref, ab = got.is_greyscale().cpu().numpy(), got.is_greyscale(mode="abs").cpu().numpy()
    for k, (name, v, p, want_ref, want_abs) in enumerate(which):
        assert (bool(ref[k]), bool(ab[k])) == (want_ref, want_abs), (name, v, p)


def test_frames_are_independent_and_n_past_65535_is_split_over_launches():
    H, W, N = 2, 16, 65537
    host = np.repeat(np.arange(N, dtype=np.uint32) % 251, H * W * 3).astype(np.uint8).reshape(N, H, W, 3)     # grey v,v,v
    marked = {100: (20, 21, 20), 65534: (9, 9, 30), 65536: (60, 50, 50)}          # the last: the second launch's last frame
    for n, px in marked.items():
        host[n, 1, 15] = px
    want = np.zeros((N, cases.WORDS), np.int32)
    for n in marked:
        want[n] = cases.records(host[n:n + 1])[0]
    assert want[65536, 0] == 10 and want[100, 0] == 255 and want[65534, 1] == 235
    got = _scan(torch.from_numpy(host).cuda(), 0, H * W * 3, N, H, W)
    assert np.array_equal(got[[99, 101, 65533, 65535]], np.zeros((4, cases.WORDS), np.int32))
    assert np.array_equal(got, want)


# ---- the fused YUV scan -------------------------------------------------------------------------------------------------------------
LAYOUTS = {"420p": sampling.YUV_420P, "422p": sampling.YUV_422P, "444p": sampling.YUV_444P, "nv12": sampling.YUV_NV12}
YUV_SIZES = [(2, 16), (6, 48), (7, 50), (3, 17)]


def _yuv_scan(src, offsets, layout, H, W, matrix, full_range):
    lib = _lib.load()
    off = torch.tensor(offsets, dtype=torch.int64).cuda()
    out = torch.full((len(offsets) * cases.WORDS * 4,), PRESET, dtype=torch.uint8, device="cuda")
    rc = lib.relax_yuv_greyscale_scan(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(off.data_ptr()), len(offsets), layout, H, W,
                                      sampling.YUV_MATRICES[matrix], int(full_range), C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, lib.relax_last_error(None).decode()
    return out.cpu().numpy().view(np.int32).reshape(-1, cases.WORDS)


def _yuv_to_bgr(src, offsets, layout, H, W, matrix, full_range):
    """relax_yuv_to_bgr into packed slots -> the device BGR buffer (first byte 16-byte aligned)."""
    lib = _lib.load()
    slot = H * W * 3
    items = torch.tensor([(o, n * slot) for n, o in enumerate(offsets)], dtype=torch.int64).cuda()
    out = _aligned(len(offsets) * slot)
    status = torch.full((len(offsets),), -7, dtype=torch.int32, device="cuda")
    rc = lib.relax_yuv_to_bgr(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(items.data_ptr()), len(offsets), layout, H, W,
                              sampling.YUV_MATRICES[matrix], int(full_range), C.c_void_p(out.data_ptr()), out.numel(),
                              C.c_void_p(status.data_ptr()), _stream())
    assert rc == 0 and not status.any()
    return out


def _yuv_frames(layout, H, W, seed):
    """Random planes; U = V = 128 under a luma ramp over 0..255; and the ramp with one chroma sample at 127, 129, 120, 136."""
    fb = sampling.yuv_frame_bytes(layout, H, W)
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(2)]
    ramp = np.full(fb, 128, np.uint8)
    ramp[:H * W] = np.linspace(0, 255, H * W).round().astype(np.uint8) if H * W > 1 else 255
    frames.append(ramp)
    frames.append(np.concatenate([np.tile(np.arange(256, dtype=np.uint8), -(-H * W // 256))[:H * W], ramp[H * W:]]))
    for k, value in enumerate((127, 129, 120, 136)):
        f = ramp.copy()
        f[H * W + (k * 5) % (fb - H * W)] = value                 # one sample of U, of V, or of NV12's interleaved pairs
        frames.append(f)
    return np.stack(frames), fb


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_fused_yuv_scan_equals_the_scan_of_the_converted_frames(name):
    layout = LAYOUTS[name]
    for H, W in YUV_SIZES:
        frames, fb = _yuv_frames(layout, H, W, 7 + H)
        N = len(frames)
        slot = (fb + 15) // 16 * 16
        packed = np.concatenate([np.zeros(1, np.uint8), frames.reshape(-1)])          # frame n at 1 + n * fb: unaligned
        padded = np.zeros(N * slot, np.uint8)                                         # frame n at n * slot: aligned
        for n in range(N):
            padded[n * slot:n * slot + fb] = frames[n]
        for offsets, host in (([1 + n * fb for n in range(N)], packed), ([n * slot for n in range(N)], padded)):
            src = _aligned(host.size)
            src.copy_(torch.from_numpy(host))
            for matrix in ("bt601", "bt709"):
                for full in (False, True):
                    fused = _yuv_scan(src, offsets, layout, H, W, matrix, full)
                    bgr = _yuv_to_bgr(src, offsets, layout, H, W, matrix, full)
                    unfused = _scan(bgr, 0, H * W * 3, N, H, W)
                    assert np.array_equal(fused, unfused), (name, H, W, matrix, full, offsets[0])
                    want = cases.records(np.stack([sampling.yuv_frame_bgr(*sampling.yuv_planes(f, layout, H, W), matrix=matrix,
                                                                          full_range=full) for f in frames]))
                    assert np.array_equal(fused, want), (name, H, W, matrix, full, offsets[0])
                    assert not fused[2:4, :6].any()                                   # U = V = 128 over the whole luma range


def test_engine_yuv_scan_and_an_out_of_range_frame():
    eng = engine()
    H, W = 6, 48
    for pixfmt in ("yuv420p", "yuvj422p", "nv12"):
        layout, full = sampling.yuv_layout(pixfmt)
        frames, fb = _yuv_frames(layout, H, W, 3)
        got = eng.yuv_greyscale_scan(torch.from_numpy(frames).cuda(), H, W, pixfmt, matrix="bt709")
        want = eng.greyscale_scan(eng.yuv_to_bgr(torch.from_numpy(frames).cuda(), H, W, pixfmt, matrix="bt709"))
        assert torch.equal(got["records"], want["records"]) and torch.equal(got.is_greyscale(), want.is_greyscale())
        assert torch.equal(eng.yuv_greyscale_scan(frames, H, W, pixfmt, matrix="bt709")["records"], want["records"])
    layout, fb = sampling.YUV_420P, sampling.yuv_frame_bytes(sampling.YUV_420P, H, W)
    frames, _ = _yuv_frames(layout, H, W, 5)
    src = torch.from_numpy(frames[:3].reshape(-1)).cuda()
    offsets = [0, 3 * fb, fb, 2 * fb + 16, -16, 2 * fb]                               # past the end, ending 16 bytes past it, negative
    got = _yuv_scan(src, offsets, layout, H, W, "bt601", False)
    ok = _yuv_scan(src, [0, fb, 2 * fb], layout, H, W, "bt601", False)
    assert got[:, 6].tolist() == [0, 1, 0, 1, 1, 0]
    assert np.array_equal(got[[0, 2, 5]], ok) and not got[[1, 3, 4], :6].any() and not got[:, 7].any()
    with pytest.raises(ValueError, match="whole number"):
        eng.yuv_greyscale_scan(torch.zeros(7, dtype=torch.uint8, device="cuda"), 2, 2, "yuv420p")
    with pytest.raises(ValueError, match="yuv420p10le"):
        eng.yuv_greyscale_scan(torch.zeros(12, dtype=torch.uint8, device="cuda"), 2, 2, "yuv420p10le")


# ---- whole files ----------------------------------------------------------------------------------------------------------------------
def _raw_file(tmp_path, colour_at):
    W, H, n = 48, 6, 40
    fb = sampling.yuv_frame_bytes(sampling.YUV_420P, H, W)
    rng = np.random.default_rng(13)
    data = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    data[:, H * W:] = 128
    if colour_at is not None:
        data[colour_at, H * W:] = rng.integers(0, 256, fb - H * W, dtype=np.uint8)
    path = str(tmp_path / f"v{colour_at}.yuv")
    data.tofile(path)
    return path, W, H, n


@pytest.mark.parametrize("colour_at", [0, 17, 39, None])
def test_whole_file_scanner_equals_the_host_loop(tmp_path, colour_at):
    path, W, H, n = _raw_file(tmp_path, colour_at)
    host = cases.records(sampling.load_frames_from_yuv(path, W, H, "yuv420p", list(range(n))))
    colour = np.flatnonzero(~cases.is_greyscale(host))
    first = int(colour[0]) if colour.size else None
    assert first == colour_at
    for chunk in (1, 7, 64):
        res = check_greyscale.scan_yuv_file(path, W, H, "yuv420p", chunk_frames=chunk)
        assert res["first_colour_frame"] == first and res["n_frames"] == n
        eff = min(chunk, n)
        limit = n if first is None else min(n, (first // eff + 2) * eff)            # the chunk holding it plus one chunk
        assert (res["frames_scanned"] == n) if first is None else (first < res["frames_scanned"] <= limit), (chunk, res["frames_scanned"])
        assert np.array_equal(res["records"], host[:res["frames_scanned"]])
        assert check_greyscale.check_video_greyscale(path, W, H, "yuv420p", chunk_frames=chunk) == (first is None, True)
    full = check_greyscale.scan_yuv_file(path, W, H, "yuv420p", chunk_frames=7, stop_at_colour=False)
    assert full["frames_scanned"] == n and np.array_equal(full["records"], host) and full["first_colour_frame"] == first


def test_directory_of_png_frames(tmp_path):
    eng = engine()
    H, W = 6, 48
    grey = np.repeat(np.random.default_rng(3).integers(0, 256, (3, H, W, 1), dtype=np.uint8), 3, axis=3)
    for name, frames, want in (("grey", grey, (True, True)), ("colour", np.concatenate([grey, cases.random_frames(1, 1, H, W, False)]), (False, True))):
        d = tmp_path / name
        d.mkdir()
        eng.write_png([str(d / f"f_{k:03d}.png") for k in range(len(frames))], torch.from_numpy(frames).cuda())
        assert check_greyscale.check_video_greyscale(str(d), chunk_frames=2) == want


# ---- the row drop in the protocol ---------------------------------------------------------------------------------------------------
def _protocol_set():
    rng = np.random.RandomState(6)
    x = rng.uniform(0, 10, size=(90, 48)).astype(np.float32)
    mos = 3 + np.sin(x[:, 0] * 0.5) + 0.1 * x[:, 1] + 0.05 * rng.standard_normal(90)
    return x, mos


PROTOCOL_CFG = dict(n_splits=2, epochs=4, hidden_features=128, batch_size=32, seed=1)
PROTOCOL_KEYS = [f"{m}_{side}" for m in metrics.METRICS for side in ("train", "test")]


def _same_protocol(a, b):
    for key in PROTOCOL_KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for ra, rb in zip(a["repeats"], b["repeats"]):
        assert np.array_equal(ra["test_rows"], rb["test_rows"]) and np.array_equal(ra["y_test_pred"], rb["y_test_pred"])
        assert np.array_equal(ra["mos_test"], rb["mos_test"])


def test_holdout_protocol_with_drop_indices_equals_the_shortened_set():
    eng = engine()
    x, mos = _protocol_set()
    drop = [4, 17, 17, 60, 89]
    keep = np.delete(np.arange(90), drop)
    feats = torch.as_tensor(x).to(eng.device)
    groups = np.arange(90) // 2
    got = eng.holdout_protocol(feats, mos, PROTOCOL_CFG, n_repeats=2, groups=groups, drop_indices=drop)
    want = eng.holdout_protocol(feats[torch.as_tensor(keep, device=eng.device)], mos[keep], PROTOCOL_CFG, n_repeats=2, groups=groups[keep])
    _same_protocol(got, want)
    assert len(got["repeats"][0]["train_rows"]) + len(got["repeats"][0]["test_rows"]) == 86
    with pytest.raises(IndexError, match="index 90 "):
        eng.holdout_protocol(feats, mos, PROTOCOL_CFG, n_repeats=1, drop_indices=[90])


def test_holdout_protocol_without_drop_indices_is_unchanged():
    eng = engine()
    x, mos = _protocol_set()
    feats = torch.as_tensor(x).to(eng.device)
    _same_protocol(eng.holdout_protocol(feats, mos, PROTOCOL_CFG, n_repeats=2, drop_indices=None),
                   metrics.holdout_protocol(eng, feats, mos, PROTOCOL_CFG, 2))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value_and_launch_nothing():
    lib = _lib.load()
    buf = torch.zeros(2 * 96, dtype=torch.uint8, device="cuda")
    buf[5] = 200                                                        # a colour pixel: a launch would raise the maxima
    for kw, named in ((dict(H=0), "H = 0"), (dict(H=sampling.YUV_MAX_DIM + 1), f"H = {sampling.YUV_MAX_DIM + 1}"), (dict(W=-3), "W = -3"),
                      (dict(W=sampling.YUV_MAX_DIM + 1), f"W = {sampling.YUV_MAX_DIM + 1}"), (dict(N=-1), "N = -1")):
        a = dict(N=2, H=2, W=16)
        a.update(kw)
        out = _scan(buf, 0, 96, a["N"], a["H"], a["W"], expect_rc=-1)
        assert named in lib.relax_last_error(None).decode(), (kw, lib.relax_last_error(None).decode())
        torch.cuda.synchronize()
        assert (out.view(np.uint8) == PRESET).all()
    out = torch.full((64,), PRESET, dtype=torch.uint8, device="cuda")
    assert lib.relax_greyscale_scan(None, 96, 2, 2, 16, C.c_void_p(out.data_ptr()), _stream()) == -1
    assert "frames is NULL" in lib.relax_last_error(None).decode()
    assert lib.relax_greyscale_scan(C.c_void_p(buf.data_ptr()), 96, 2, 2, 16, None, _stream()) == -1
    assert "out is NULL" in lib.relax_last_error(None).decode()
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    for kw, named in ((dict(H=0), "H = 0"), (dict(W=sampling.YUV_MAX_DIM + 1), f"W = {sampling.YUV_MAX_DIM + 1}"), (dict(N=-1), "N -1"),
                      (dict(layout=9), "layout 9"), (dict(matrix=5), "matrix 5"), (dict(full_range=2), "full_range 2"), (dict(src=None), "NULL")):
        a = dict(src=C.c_void_p(buf.data_ptr()), N=2, layout=0, H=2, W=16, matrix=0, full_range=0)
        a.update(kw)
        rc = lib.relax_yuv_greyscale_scan(a["src"], buf.numel(), C.c_void_p(off.data_ptr()), a["N"], a["layout"], a["H"], a["W"],
                                          a["matrix"], a["full_range"], C.c_void_p(out.data_ptr()), _stream())
        assert rc == -1 and named in lib.relax_last_error(None).decode(), (kw, lib.relax_last_error(None).decode())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == PRESET).all()
