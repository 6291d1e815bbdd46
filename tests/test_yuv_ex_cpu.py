"""The RELAX_YUVF_* formats on the host (sampling.yuv_format / yuv_samples / yuv_frame_bgr_ex, load_clip_from_yuv(extended=True);
relax_yuv_frame_bytes_ex, relax_yuv_format_info; csrc/yuv_core.h under AddressSanitizer + UBSan as a stand-alone program): frame
sizes against numbers written out, the one formula against float64 at depths 10 and 12, the int32 bound, and the layouts byte by
byte.  No GPU.  `python -m tests.test_yuv_ex_cpu` rewrites profiles/yuv_ex_parity.json from the float64 comparison."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import _lib, sampling
from tests import yuv_ex_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def test_frame_bytes_against_written_out_numbers_and_refusals():
    lib = _lib.load()
    for (name, W, H), want in cases.FRAME_BYTES.items():
        fmt, _ = sampling.yuv_format(name)
        assert lib.relax_yuv_frame_bytes_ex(fmt, H, W) == want, (name, W, H)
        assert sampling.yuv_frame_bytes_ex(fmt, H, W) == want, (name, W, H)
    for name in cases.NEW_NAMES + cases.OLD_NAMES:                            # every format at every size: library == Python
        fmt, _ = sampling.yuv_format(name)
        for W, H in cases.CPU_SIZES + [(16384, 16384)]:
            assert lib.relax_yuv_frame_bytes_ex(fmt, H, W) == sampling.yuv_frame_bytes_ex(fmt, H, W) > 0
    for layout in range(4):
        assert lib.relax_yuv_frame_bytes_ex(layout, 17, 33) == lib.relax_yuv_frame_bytes(layout, 17, 33)
    for fmt, H, W in ((-1, 4, 4), (16, 4, 4), (99, 4, 4), (9, 0, 4), (9, 4, 0), (6, 16385, 4), (6, 4, 16385), (8, -1, 4)):
        assert lib.relax_yuv_frame_bytes_ex(fmt, H, W) == -1, (fmt, H, W)
        with pytest.raises(ValueError):
            sampling.yuv_frame_bytes_ex(fmt, H, W)
    import ctypes as C
    out = (C.c_int32 * 8)()
    for bad in (-1, 16):
        assert lib.relax_yuv_format_info(bad, out) != 0 and str(bad) in lib.relax_last_error(None).decode()
    for fmt, row in enumerate(cases.FORMAT_INFO):                             # the whole table, written out
        assert lib.relax_yuv_format_info(fmt, out) == 0 and list(out) == row + [0], fmt
        assert list(sampling.yuv_format_info(fmt).values()) == row, fmt
    for bad in (True, False, 1.0, "1", None, 16):
        with pytest.raises(ValueError):
            sampling.yuv_format_info(bad)


def test_yuv_format_accepts_exactly_the_19_names():
    assert len(cases.OLD_NAMES) + len(cases.NEW_NAMES) == 19 == len(sampling._YUV_FORMATS)
    for name in cases.OLD_NAMES:
        assert sampling.yuv_format(name) == sampling.yuv_layout(name)
    for name, fmt in cases.NEW_FORMATS.items():
        assert sampling.yuv_format(name) == (fmt, False)
        with pytest.raises(ValueError, match=re.escape(repr(name))):          # the default surface still refuses them
            sampling.yuv_layout(name)
    for name in cases.REFUSED_NAMES:
        with pytest.raises(ValueError, match=re.escape(repr(name))):
            sampling.yuv_format(name)


def test_layouts_byte_by_byte():
    """Frames written out by hand, 4 x 2 (W x H) and one odd width: which byte is which sample."""
    b = np.arange(1, 65, dtype=np.uint8)
    y, u, v, d = sampling.yuv_samples(b[:16], 5, 2, 4)                         # yuyv422: Y0 U Y1 V
    assert d == 8 and y.tolist() == [[1, 3, 5, 7], [9, 11, 13, 15]] and u.tolist() == [[2, 6], [10, 14]] and v.tolist() == [[4, 8], [12, 16]]
    y, u, v, d = sampling.yuv_samples(b[:16], 6, 2, 4)                         # uyvy422: U Y0 V Y1
    assert y.tolist() == [[2, 4, 6, 8], [10, 12, 14, 16]] and u.tolist() == [[1, 5], [9, 13]] and v.tolist() == [[3, 7], [11, 15]]
    y, u, v, d = sampling.yuv_samples(b[:8], 6, 1, 3)                          # odd W: the last group's second luma (byte 8) is never shown
    assert y.tolist() == [[2, 4, 6]] and u.tolist() == [[1, 5]] and v.tolist() == [[3, 7]]
    y, u, v, d = sampling.yuv_samples(b[:12], 4, 2, 4)                         # nv21: V first
    assert y.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8]] and v.tolist() == [[9, 11]] and u.tolist() == [[10, 12]]
    y, u, v, d = sampling.yuv_samples(b[:12], 7, 2, 4)                         # yuv411p: one chroma sample per four pixels and row
    assert u.tolist() == [[9], [10]] and v.tolist() == [[11], [12]]
    y, u, v, d = sampling.yuv_samples(b[:33], 8, 5, 5)                         # yuv410p: 5 x 5 -> chroma 2 x 2
    assert y.shape == (5, 5) and u.tolist() == [[26, 27], [28, 29]] and v.tolist() == [[30, 31], [32, 33]]
    words = np.array([0x0001, 0x03FF, 0xFFFF, 0xFC00, 0x0200, 0x0155], "<u2")
    y, u, v, d = sampling.yuv_samples(words.view(np.uint8), 11, 1, 2)          # yuv444p10le: low 10 bits, higher bits masked off
    assert d == 10 and y.tolist() == [[1, 1023]] and u.tolist() == [[1023, 0]] and v.tolist() == [[512, 0x155]]
    y, u, v, d = sampling.yuv_samples(words.view(np.uint8), 14, 1, 2)          # yuv444p12le: low 12 bits
    assert d == 12 and u.tolist() == [[4095, 0xC00]]
    words = np.array([0x0040, 0xFFFF, 0x003F, 0xFFC0, 0x8000, 0x8040], "<u2")
    y, u, v, d = sampling.yuv_samples(words.view(np.uint8), 15, 2, 2)          # p010le: the high 10 bits, U first
    assert d == 10 and y.tolist() == [[1, 1023], [0, 1023]] and u.tolist() == [[512]] and v.tolist() == [[513]]
    rng = np.random.default_rng(1)
    for name in cases.NEW_NAMES:                                              # pack_frame (the tests' frame builder) is the inverse
        fmt, _ = cases.fmt(name)
        t, p = sampling.yuv_format_info(fmt), sampling.yuv_plan_ex(fmt, 7, 9)
        yy, uu, vv = (rng.integers(0, 1 << t["depth"], s) for s in ((7, 9), (p["ch"], p["cw"]), (p["ch"], p["cw"])))
        y, u, v, d = sampling.yuv_samples(cases.pack_frame(name, yy, uu, vv, filler=0xFF if t["shift"] == 0 else 0x3F), fmt, 7, 9)
        assert np.array_equal(y, yy) and np.array_equal(u, uu) and np.array_equal(v, vv) and d == t["depth"]


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_depth_8_is_yuv_frame_bgr_bit_for_bit(layout):
    rng = np.random.default_rng(40 + layout)
    for W, H in cases.CPU_SIZES:
        frame = rng.integers(0, 256, sampling.yuv_frame_bytes(layout, H, W), dtype=np.uint8)
        y, u, v, depth = sampling.yuv_samples(frame, layout, H, W)
        planes = sampling.yuv_planes(frame, layout, H, W)
        assert depth == 8 and all(np.array_equal(a, b) for a, b in zip((y, u, v), planes))
        for matrix, full in cases.COMBOS:
            assert np.array_equal(sampling.yuv_frame_bgr_ex(y, u, v, 8, matrix=matrix, full_range=full),
                                  sampling.yuv_frame_bgr(*planes, matrix=matrix, full_range=full))


def _float_coefficients(matrix, full_range):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    crv, cbu = 2 * (1 - kr), 2 * (1 - kb)
    s = 1.0 if full_range else 255.0 / 224.0
    return (1.0 if full_range else 255.0 / 219.0), crv * s, cbu * s, kb * cbu / kg * s, kr * crv / kg * s


def _grid(depth):
    """depth 10: every Y x every 4th U and V plus 0 and 1023; depth 12: every 16th of each, plus the ends."""
    top = (1 << depth) - 1
    if depth == 10:
        c = np.unique(np.concatenate([np.arange(0, 1024, 4), [0, top]]))
        return np.arange(1024), c, c
    c = np.unique(np.concatenate([np.arange(0, 4096, 16), [0, top]]))
    return c, c, c


def _parity(depth, matrix, full_range):
    """-> {channel: (max diff, share of differing values)} of yuv_frame_bgr_ex against the float64 conversion rounded to 8 bits."""
    s = depth - 8
    ys, us, vs = _grid(depth)
    fy, frv, fbu, fgu, fgv = _float_coefficients(matrix, full_range)
    worst, differing, total = [0, 0, 0], [0, 0, 0], 0
    for y0 in range(0, len(ys), 64):                                          # in chunks of 64 luma values
        Y, U, V = np.meshgrid(ys[y0:y0 + 64], us, vs, indexing="ij")
        Y, U, V = (a.reshape(len(a), -1) for a in (Y, U, V))
        got = sampling.yuv_frame_bgr_ex(Y, U, V, depth, matrix=matrix, full_range=full_range)
        y = fy * (Y.astype(np.float64) - ((0 if full_range else 16) << s))
        u, v = U.astype(np.float64) - (128 << s), V.astype(np.float64) - (128 << s)
        for ch, val in ((0, y + fbu * u), (1, y - fgu * u - fgv * v), (2, y + frv * v)):
            want = np.clip(np.floor(val / (1 << s) + 0.5), 0, 255).astype(np.int16)
            diff = np.abs(got[..., ch].astype(np.int16) - want)
            worst[ch] = max(worst[ch], int(diff.max()))
            differing[ch] += int((diff != 0).sum())
        total += Y.size
    return {name: (worst[ch], differing[ch] / total) for ch, name in enumerate("BGR")}


# A value can differ from float64 only where the exact result lies within the constants' rounding error of a rounding boundary: six
# constants rounded to 1/65536 move a channel by at most 3 x 0.5/65536 x 255 = 0.006 code values, so for equidistributed fractions
# at most 1.2 % of the values can sit that close to a boundary on either side.  The measured shares are in profiles/yuv_ex_parity.json.
SHARE_CAP = 0.012


@pytest.mark.parametrize("matrix,full_range", cases.COMBOS)
@pytest.mark.parametrize("depth", [10, 12])
def test_within_one_code_value_of_float64(depth, matrix, full_range):
    for name, (worst, share) in _parity(depth, matrix, full_range).items():
        print(f"depth {depth} {matrix} {'full' if full_range else 'limited'} {name}: max diff {worst}, differing {100 * share:.4f} %")
        assert worst <= 1, (depth, matrix, full_range, name)
        assert share < SHARE_CAP, (depth, matrix, full_range, name, share)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_every_sum_fits_int32(depth):
    """The extremes of Y, U and V under both matrices and both ranges: every intermediate sum evaluated in int64 lies inside int32,
    and the int64 result equals yuv_frame_bgr_ex's int32 one."""
    s, top = depth - 8, (1 << depth) - 1
    e = np.array([0, top], np.int64)
    Y, U, V = (a.reshape(1, -1) for a in np.meshgrid(e, e, e, indexing="ij"))
    for matrix, full in cases.COMBOS:
        cy, oy, crv, cbu, cgu, cgv = (np.int64(c) for c in sampling.yuv_coefficients(matrix, full))
        y = cy * (Y - (oy << s)) + (1 << (15 + s))
        u, v = U - (128 << s), V - (128 << s)
        sums = {"r": y + crv * v, "g": y - cgu * u - cgv * v, "b": y + cbu * u}
        parts = [y, crv * v, cgu * u, cgv * v, cbu * u, y - cgu * u] + list(sums.values())
        assert all(int(np.abs(p).max()) < 2 ** 31 for p in parts), (depth, matrix, full)
        want = np.stack([np.clip(sums[c], 0, (1 << (24 + s)) - 1) >> (16 + s) for c in "bgr"], axis=-1)
        got = sampling.yuv_frame_bgr_ex(Y, U, V, depth, matrix=matrix, full_range=full)
        assert np.array_equal(got, want.astype(np.uint8)) and want.max() <= 255
    with pytest.raises(ValueError, match="14"):
        sampling.yuv_frame_bgr_ex(Y, U, V, 14)


def test_garbage_bits_do_not_change_the_output():
    rng = np.random.default_rng(77)
    W, H = 34, 18
    for name, garbage in (("yuv420p10le", 0xFC00), ("yuv422p10le", 0xFC00), ("yuv444p12le", 0xF000), ("p010le", 0x003F)):
        fmt, _ = cases.fmt(name)
        t, p = sampling.yuv_format_info(fmt), sampling.yuv_plan_ex(fmt, H, W)
        y, u, v = (rng.integers(0, 1 << t["depth"], s) for s in ((H, W), (p["ch"], p["cw"]), (p["ch"], p["cw"])))
        clean = cases.pack_frame(name, y, u, v)
        dirty = (clean.view("<u2") | (rng.integers(0, 65536, clean.size // 2).astype(np.uint16) & garbage)).view(np.uint8)
        assert not np.array_equal(clean, dirty)
        assert np.array_equal(cases.host_bgr(clean, name, H, W), cases.host_bgr(dirty, name, H, W))


@pytest.mark.parametrize("name,W,H,n,framerate", [("yuv420p10le", 48, 32, 60, 25), ("uyvy422", 33, 17, 31, 30), ("yuv410p", 34, 18, 31, 2.5)])
def test_load_clip_extended_equals_the_per_frame_statement(tmp_path, name, W, H, n, framerate):
    path = str(tmp_path / "v.yuv")
    frames = cases.random_frames(name, H, W, n, 19)
    frames.tofile(path)
    assert sampling.yuv_frame_count(path, W, H, name, extended=True) == n
    _, _, pairs = sampling.sampled_frame_indices(n, sampling.frame_interval(framerate))
    clip = sampling.load_clip_from_yuv(path, W, H, name, framerate, extended=True)
    assert clip.shape == (len(pairs), 2, H, W, 3) and len(pairs) >= 2
    for t, (a, b) in enumerate(pairs):
        assert np.array_equal(clip[t, 0], cases.host_bgr(frames[a], name, H, W)) and np.array_equal(clip[t, 1], cases.host_bgr(frames[b], name, H, W))
    got = sampling.load_frames_from_yuv(path, W, H, name, [0, n - 1], extended=True)
    assert np.array_equal(got[1], cases.host_bgr(frames[n - 1], name, H, W))
    with pytest.raises(ValueError, match=re.escape(repr(name))):              # without the keyword: refused by name, as before
        sampling.load_clip_from_yuv(path, W, H, name, framerate)
    fb = cases.frame_bytes(name, H, W)
    with open(path, "ab") as f:
        f.write(b"\0" * 5)
    with pytest.raises(ValueError, match=rf"{n} frames and 5 bytes over"):
        sampling.load_clip_from_yuv(path, W, H, name, framerate, extended=True)
    assert os.path.getsize(path) == n * fb + 5


def test_sanitizer_program_walks_every_format_clean():
    """csrc/yuv_ex_host.cpp (yuv_core.h's RELAX_YUVF_* half with its own main) under AddressSanitizer + UBSan: a plain child process.
    Its plan lines equal sampling.yuv_plan_ex, the layout yuv_samples reads by."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no AddressSanitizer")
    subprocess.run(["make", "-C", CSRC, "sanitize_yuv_ex"], check=True, capture_output=True)
    res = subprocess.run([os.path.join(CSRC, "yuv_ex_san")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.strip().endswith("ok") and "MISMATCH" not in res.stdout
    assert res.stderr == "", res.stderr
    keys = ("frame_bytes", "sb", "depth", "shift", "hshift", "vshift", "packing", "cw", "ch", "y_off", "y_step", "y_stride", "u_off", "v_off",
            "c_step", "c_stride", "units", "fast")
    plans = re.findall(r"plan (\d+) (\d+) (\d+) : " + " ".join(rf"{k} (\d+)" for k in keys), res.stdout)
    seen = set()
    for row in plans:
        fmt, H, W = map(int, row[:3])
        got = dict(zip(keys, map(int, row[3:])))
        t, p = sampling.yuv_format_info(fmt), sampling.yuv_plan_ex(fmt, H, W)
        for k in ("frame_bytes", "cw", "ch", "y_off", "y_step", "y_stride", "u_off", "v_off", "c_step", "c_stride"):
            assert got[k] == p[k], (row, k)
        assert (got["sb"], got["depth"], got["shift"], got["hshift"], got["vshift"], got["packing"]) == \
            (t["sample_bytes"], t["depth"], t["shift"], t["hshift"], t["vshift"], t["packing"])
        assert got["units"] == -(-H // (1 << t["vshift"])) * ((W + 15) // 16) and got["fast"] == (W % 16 == 0)
        seen.add((fmt, H, W))
    for fmt in range(16):
        for W, H in cases.CPU_SIZES + [(16, 2), (64, 32), (97, 131)]:
            assert (fmt, H, W) in seen, (fmt, H, W)


if __name__ == "__main__":
    out = {"what": "sampling.yuv_frame_bgr_ex (the integer formula of relax_yuv_to_bgr_ex) against the float64 BT.601 / BT.709 conversion "
                   "rounded to 8 bits: largest difference in code values and share of differing values per channel",
           "grid": {"10": "every Y x every 4th U and V plus 0 and 1023", "12": "every 16th of Y, U and V plus the ends"}, "cases": []}
    for depth in (10, 12):
        for matrix, full in cases.COMBOS:
            r = _parity(depth, matrix, full)
            out["cases"].append({"depth": depth, "matrix": matrix, "full_range": full,
                                 "max_diff": {k: v[0] for k, v in r.items()}, "share_differing": {k: round(v[1], 7) for k, v in r.items()}})
    with open(os.path.join(ROOT, "profiles", "yuv_ex_parity.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
