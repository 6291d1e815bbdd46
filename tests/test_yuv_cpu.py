"""Raw YUV input on the host (sampling.yuv_*, load_clip_from_yuv, video_frames_extract; csrc/yuv_core.h): the integer colour
arithmetic against float64 over every (Y,U,V) triple, the frame layout for odd sizes, frame counting, pairing, and the layout
and bounds code of the kernel under AddressSanitizer + UBSan as a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import _lib, sampling, video_frames_extract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")
PIXFMTS = ["yuv420p", "yuvj420p", "yuv422p", "yuvj422p", "yuv444p", "yuvj444p", "nv12"]
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def _float_coefficients(matrix, full_range):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    crv, cbu = 2 * (1 - kr), 2 * (1 - kb)
    s = 1.0 if full_range else 255.0 / 224.0
    return (1.0 if full_range else 255.0 / 219.0), crv * s, cbu * s, kb * cbu / kg * s, kr * crv / kg * s


@pytest.mark.parametrize("matrix,full_range", [(m, f) for m in ("bt601", "bt709") for f in (False, True)])
def test_constants_are_the_rounded_float_coefficients(matrix, full_range):
    cy, oy, crv, cbu, cgu, cgv = sampling.yuv_coefficients(matrix, full_range)
    want = [round(65536 * x) for x in _float_coefficients(matrix, full_range)]
    assert oy == (0 if full_range else 16)
    # BT.601 full range: cgv is the table's 46801 (65536 * 0.714136 = 46801.6, truncated), one below the rounded value
    slack = [0, 0, 0, 0, 1 if (matrix, full_range) == ("bt601", True) else 0]
    for got, w, s in zip((cy, crv, cbu, cgu, cgv), want, slack):
        assert abs(got - w) <= s, (matrix, full_range, got, w)


# share of differing values per channel, measured over all 2^24 triples (printed by the test below):
#   bt601 limited  B 0.0092 %  G 0.0378 %  R 0.0046 %      bt601 full  B 0.0519 %  G 0.0486 %  R 0 (crv * 127 stays under half a step)
#   bt709 limited  B 0.0061 %  G 0.0407 %  R 0.0046 %      bt709 full  B 0       G 0.0471 %  R 0
# BT.601's largest is 0.052 % and its cap 0.1 %; BT.709 stays below BT.601 and gets the same cap.  A value can differ only where
# the exact result lies within the constants' rounding error (at most 3 x 0.5/65536 x 255 = 0.006 code values) of a rounding
# boundary: for equidistributed fractions that is under 0.6 % at the very worst and about a tenth of it in the mean.
SHARE_CAP = 0.001


@pytest.mark.parametrize("matrix,full_range", [(m, f) for m in ("bt601", "bt709") for f in (False, True)])
def test_every_triple_is_within_one_of_float64(matrix, full_range):
    Y, U, V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    Y, U, V = Y.reshape(4096, 4096), U.reshape(4096, 4096), V.reshape(4096, 4096)
    got = sampling.yuv_frame_bgr(Y, U, V, matrix=matrix, full_range=full_range)
    fy, frv, fbu, fgu, fgv = _float_coefficients(matrix, full_range)
    y = fy * (Y.astype(np.float64) - (0 if full_range else 16))
    u, v = U.astype(np.float64) - 128, V.astype(np.float64) - 128
    for name, ch, val in (("B", 0, y + fbu * u), ("G", 1, y - fgu * u - fgv * v), ("R", 2, y + frv * v)):
        want = np.clip(np.floor(val + 0.5), 0, 255).astype(np.int16)
        diff = np.abs(got[..., ch].astype(np.int16) - want)
        share = float((diff != 0).mean())
        print(f"{matrix} {'full' if full_range else 'limited'} {name}: max diff {int(diff.max())}, differing {100 * share:.4f} %")
        assert diff.max() <= 1
        assert share < SHARE_CAP, (matrix, full_range, name, share)


def _frame_bgr_by_pixel(frame, layout, H, W, matrix, full_range):
    """The conversion one pixel at a time from the flat frame, with the offsets written out."""
    cy, oy, crv, cbu, cgu, cgv = sampling.yuv_coefficients(matrix, full_range)
    cw = W if layout == sampling.YUV_444P else (W + 1) // 2
    ch = (H + 1) // 2 if layout in (sampling.YUV_420P, sampling.YUV_NV12) else H
    out = np.zeros((H, W, 3), np.uint8)
    f = [int(x) for x in frame]
    for r in range(H):
        for c in range(W):
            cr = r // 2 if layout in (sampling.YUV_420P, sampling.YUV_NV12) else r
            cc = c if layout == sampling.YUV_444P else c // 2
            if layout == sampling.YUV_NV12:
                U, V = f[H * W + (cr * cw + cc) * 2], f[H * W + (cr * cw + cc) * 2 + 1]
            else:
                U, V = f[H * W + cr * cw + cc], f[H * W + ch * cw + cr * cw + cc]
            y = cy * (f[r * W + c] - oy) + 32768
            out[r, c] = [min(max(v >> 16, 0), 255) for v in (y + cbu * (U - 128), y - cgu * (U - 128) - cgv * (V - 128), y + crv * (V - 128))]
    return out


@pytest.mark.parametrize("pixfmt", PIXFMTS)
def test_layout_and_replication_for_odd_sizes(pixfmt):
    layout, full = sampling.yuv_layout(pixfmt)
    lib = _lib.load()
    rng = np.random.default_rng(11)
    for H, W in ((1, 1), (2, 2), (3, 5), (5, 4), (7, 9), (18, 34)):
        p = sampling.yuv_plan(layout, H, W)
        cw = W if layout == sampling.YUV_444P else (W + 1) // 2
        ch = (H + 1) // 2 if layout in (sampling.YUV_420P, sampling.YUV_NV12) else H
        assert (p["cw"], p["ch"], p["frame_bytes"], p["u_off"]) == (cw, ch, H * W + 2 * cw * ch, H * W)
        assert lib.relax_yuv_frame_bytes(layout, H, W) == p["frame_bytes"]
        frame = rng.integers(0, 256, p["frame_bytes"], dtype=np.uint8)
        y, u, v = sampling.yuv_planes(frame, layout, H, W)
        assert y.shape == (H, W) and u.shape == v.shape == (ch, cw)
        for matrix in ("bt601", "bt709"):
            assert np.array_equal(sampling.yuv_frame_bgr(y, u, v, matrix=matrix, full_range=full),
                                  _frame_bgr_by_pixel(frame, layout, H, W, matrix, full)), (H, W, matrix)
    assert sampling.yuv_frame_bytes(sampling.yuv_layout("yuv420p")[0], 1080, 1920) == 3110400
    assert sampling.yuv_frame_bytes(sampling.yuv_layout("yuv420p")[0], 18, 34) == 918


def test_refused_geometry_and_pixfmts():
    lib = _lib.load()
    for layout, H, W in ((-1, 4, 4), (4, 4, 4), (0, 0, 4), (0, 4, 0), (0, -1, 4), (0, 4, sampling.YUV_MAX_DIM + 1)):
        assert lib.relax_yuv_frame_bytes(layout, H, W) < 0
        with pytest.raises(ValueError):
            sampling.yuv_plan(layout, H, W)
    assert sampling.YUV_MAX_DIM >= 8192 and lib.relax_yuv_frame_bytes(0, sampling.YUV_MAX_DIM, sampling.YUV_MAX_DIM) == 3 * sampling.YUV_MAX_DIM ** 2 // 2
    assert [sampling.yuv_layout(p) for p in PIXFMTS] == [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, False)]
    for p in ("yuv420p10le", "yuv422p10le", "yuv444p10le", "yuv420p12le", "uyvy422", "yuyv422", "pal8", "rgb24", "bgr24", "gbrp", "yuva420p",
              "gray", "nv21", "p010le", "", "YUV420P"):
        with pytest.raises(ValueError, match=re.escape(repr(p))):
            sampling.yuv_layout(p)
    # the C entry refuses before it launches anything (no GPU needed), naming the value
    bad = [dict(layout=7), dict(H=0), dict(W=sampling.YUV_MAX_DIM + 1), dict(matrix=2), dict(full_range=3)]
    for kw in bad:
        a = dict(layout=0, H=4, W=4, matrix=0, full_range=0)
        a.update(kw)
        rc = lib.relax_yuv_to_bgr(None, 0, None, 0, a["layout"], a["H"], a["W"], a["matrix"], a["full_range"], None, 0, None, None)
        assert rc == -1
        (name, value), = kw.items()
        assert str(value) in lib.relax_last_error(None).decode(), (kw, lib.relax_last_error(None).decode())
    assert lib.relax_yuv_to_bgr(None, 0, None, 0, 0, 4, 4, 0, 0, None, 0, None, None) == 0      # N = 0: nothing to do


def _write_video(path, pixfmt, H, W, n_frames, seed):
    layout, _ = sampling.yuv_layout(pixfmt)
    fb = sampling.yuv_frame_bytes(layout, H, W)
    data = np.random.default_rng(seed).integers(0, 256, (n_frames, fb), dtype=np.uint8)
    data.tofile(path)
    return data


def test_frame_count_and_truncated_file(tmp_path):
    p = str(tmp_path / "v.yuv")
    data = _write_video(p, "yuv420p", 17, 33, 5, 1)
    fb = data.shape[1]
    assert fb == 17 * 33 + 2 * 9 * 17 and sampling.yuv_frame_count(p, 33, 17, "yuv420p") == 5
    with open(p, "ab") as f:
        f.write(bytes(7))
    with pytest.raises(ValueError, match=rf"{5 * fb + 7} bytes.*5 frames and 7 bytes over"):
        sampling.yuv_frame_count(p, 33, 17, "yuv420p")
    with pytest.raises(ValueError):
        sampling.load_clip_from_yuv(p, 33, 17, "yuv420p", 25)


@pytest.mark.parametrize("framerate", [1, 2.5, 25, 30])
@pytest.mark.parametrize("pixfmt", ["yuv420p", "yuvj422p", "nv12"])
def test_pairing_equals_pair_frames_of_the_converted_video(tmp_path, framerate, pixfmt):
    H, W, n = 10, 14, 61
    p = str(tmp_path / "v.yuv")
    data = _write_video(p, pixfmt, H, W, n, 3)
    layout, full = sampling.yuv_layout(pixfmt)
    video = np.stack([sampling.yuv_frame_bgr(*sampling.yuv_planes(f, layout, H, W), full_range=full) for f in data])
    want = sampling.pair_frames(video, framerate)
    got = sampling.load_clip_from_yuv(p, W, H, pixfmt, framerate)
    assert got.dtype == np.uint8 and got.shape == want.shape and want.shape[0] > 0 and np.array_equal(got, want)
    calls = []

    def alloc(shape):
        calls.append(shape)
        return np.zeros(shape, np.uint8)
    got2 = sampling.load_clip_from_yuv(p, W, H, pixfmt, framerate, alloc=alloc)
    assert calls == [want.shape] and np.array_equal(got2, want)
    # the reference's two entry points
    k = sampling.frame_interval(framerate)
    clip = video_frames_extract.process_video_residual("live_qualcomm", "v", k, p, str(tmp_path / "unused"), W, H, pixfmt, framerate)
    assert np.array_equal(clip, want) and not os.path.exists(tmp_path / "unused")
    frames = video_frames_extract.process_video("live_qualcomm", "v", k, p, str(tmp_path / "unused"), W, H, pixfmt, framerate)
    assert np.array_equal(frames, video[::k])


def test_no_pair_and_container_types_raise(tmp_path):
    p = str(tmp_path / "one.yuv")
    _write_video(p, "yuv420p", 4, 4, 1, 5)
    with pytest.raises(FileNotFoundError):
        sampling.load_clip_from_yuv(p, 4, 4, "yuv420p", 30)
    for fn in (video_frames_extract.process_video, video_frames_extract.process_video_residual):
        with pytest.raises(NotImplementedError, match="decoder"):
            fn("youtube_ugc", "v", 12, "v.mkv", str(tmp_path), 4, 4, "yuv420p", 25)


def test_sanitizer_program_walks_the_grid_clean():
    """csrc/yuv_host.cpp (yuv_core.h with its own main) under AddressSanitizer + UBSan: a plain child process.  Its plan lines
    equal the Python arithmetic."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no AddressSanitizer")
    subprocess.run(["make", "-C", CSRC, "sanitize_yuv"], check=True, capture_output=True)
    res = subprocess.run([os.path.join(CSRC, "yuv_san")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.strip().endswith("ok") and "MISMATCH" not in res.stdout
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    plans = re.findall(r"plan (\d+) (\d+) (\d+) : frame_bytes (\d+) u_off (\d+) v_off (\d+) cw (\d+) ch (\d+) c_stride (\d+) c_step (\d+) "
                       r"units (\d+) fast (\d)", res.stdout)
    seen = set()
    for row in plans:
        layout, H, W, fb, uo, vo, cw, ch, cs, step, units, fast = map(int, row)
        p = sampling.yuv_plan(layout, H, W)
        assert (fb, uo, vo, cw, ch, cs, step) == (p["frame_bytes"], p["u_off"], p["v_off"], p["cw"], p["ch"], p["c_stride"], p["c_step"]), row
        rows = (H + 1) // 2 if layout in (0, 3) else H
        assert units == rows * ((W + 15) // 16) and fast == (W % 16 == 0)
        seen.add((layout, H, W))
    for layout in range(4):
        for hw in ((2, 2), (2, 16), (18, 34), (131, 97), (32, 64)):          # the GPU tests' sizes (H, W)
            assert (layout,) + hw in seen


def test_read_yuv_frames_reads_runs_into_padded_slots(tmp_path):
    """The loader's file reads: each run of adjacent frames is one read, every frame lands at its 16-byte-aligned slot."""
    p = str(tmp_path / "v.yuv")
    data = _write_video(p, "yuv420p", 18, 34, 40, 9)
    fb = data.shape[1]
    assert fb == 918 and fb % 16
    slot = (fb + 15) // 16 * 16
    for frames, reads in (([0, 1, 12, 13, 24, 25, 36, 37], 4), (list(range(40)), 1), ([3], 1), ([0, 2, 3, 4, 39], 3)):
        host = np.full(len(frames) * slot + 5, 0xEE, np.uint8)
        assert sampling.read_yuv_frames(p, frames, fb, slot, host) == reads
        for k, n in enumerate(frames):
            assert np.array_equal(host[k * slot:k * slot + fb], data[n]), (frames, n)
            assert (host[k * slot + fb:(k + 1) * slot] == 0xEE).all()
        assert (host[len(frames) * slot:] == 0xEE).all()
    with pytest.raises(OSError, match="frame 39"):
        sampling.read_yuv_frames(p, [39, 40], fb, slot, np.zeros(2 * slot, np.uint8))
