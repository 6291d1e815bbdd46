"""The f16x2 streaming attention (csrc/attention_stream_h2.hip) without a GPU: its plan as host logic (csrc/host_logic.cpp:
att_stream_h2_plan) and its arithmetic restated in numpy - fp16 hi / lo planes at h2_scale_for(max), three partial products for both
contractions, the fma'd exponent argument, the tile-wise online softmax and probability planes of e * 2^14 - against fp64 and against
torch-CPU fp32's own distance from fp64.  numpy's summation order is not the MFMA's: this pins the arithmetic, the device tests
(tests/test_gpu_attention_stream_h2.py) pin the kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import h2_restated, vit_patch8_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
FIELDS = ("key_tile", "qblock", "qblocks", "key_tiles", "lds_bytes", "wgs_per_cu", "items")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    return C.CDLL(str(out))


def _plan(lib, n_img, heads, ntok):
    out, err = (C.c_int * len(FIELDS))(), C.create_string_buffer(256)
    rc = lib.relax_host_att_stream_h2_plan(n_img, heads, ntok, out, err, 256)
    return dict(zip(FIELDS, out)) if rc == 0 else err.value.decode()


def _tile(lib):
    return _plan(lib, 1, 1, 1)["key_tile"]


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["1", "tile-1", "tile", "tile+1", "197", "785", "4097"])
def test_plan_invariants(host_lib, which):
    tile = _tile(host_lib)
    ntok = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}.get(which) or int(which)
    for n_img, heads in ((1, 1), (3, 12), (256, 12)):
        p = _plan(host_lib, n_img, heads, ntok)
        assert isinstance(p, dict), p
        assert p["key_tile"] in (32, 64) and p["qblock"] > 0 and p["qblock"] % 32 == 0
        # every query is in exactly one block: the blocks [b qblock, min(ntok, (b + 1) qblock)) are non-empty, disjoint and cover [0, ntok)
        covered = np.zeros(ntok, dtype=np.int64)
        for b in range(p["qblocks"]):
            lo, hi = b * p["qblock"], min(ntok, (b + 1) * p["qblock"])
            assert lo < hi, f"query block {b} of {p['qblocks']} is empty at ntok={ntok}"
            covered[lo:hi] += 1
        assert (covered == 1).all()
        assert p["key_tiles"] == -(-ntok // p["key_tile"])
        assert p["wgs_per_cu"] >= 1 and 0 < p["lds_bytes"] and p["lds_bytes"] * p["wgs_per_cu"] <= LDS_PER_CU
        assert p["items"] == n_img * heads * p["qblocks"]


def test_plan_refusals_name_their_values(host_lib):
    for n_img, heads, ntok in ((0, 12, 785), (2, 0, 785), (2, 12, 0), (-1, 12, 785)):
        msg = _plan(host_lib, n_img, heads, ntok)
        assert isinstance(msg, str) and f"Nimg={n_img}" in msg and f"heads={heads}" in msg and f"ntok={ntok}" in msg, msg
    tile = _tile(host_lib)
    # an image's plane rows: (ntok + one tile) rows of 3 * dim * 4 bytes must stay below 2^31
    heads = 700
    limit = (2 ** 31 - 1) // (heads * 64 * 3 * 4) - tile      # the largest ntok that fits
    assert isinstance(_plan(host_lib, 1, heads, limit), dict)
    msg = _plan(host_lib, 1, heads, limit + 1)
    assert isinstance(msg, str) and "2^31 bytes" in msg and str(limit + 1) in msg and str(heads) in msg, msg
    # items
    ok = _plan(host_lib, 2 ** 20, 12, 1500)
    assert isinstance(ok, dict) and ok["items"] == 2 ** 20 * 12 * ok["qblocks"]
    msg = _plan(host_lib, 2 ** 24, 12, 1500)
    assert isinstance(msg, str) and str(2 ** 24 * 12 * ok["qblocks"]) in msg and "items" in msg, msg


def test_the_bf16x6_plan_still_refuses_other_arithmetics(host_lib):
    out, err = (C.c_int * 5)(), C.create_string_buffer(256)
    assert host_lib.relax_host_att_stream_plan(1, 3, 785, 2, out, err, 256) != 0


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------
def _planes(x, s):
    """fp32 x -> (hi, lo) as fp32 arrays holding fp16 values of x s"""
    hi, lo = h2_restated.split2(x, s)
    return hi.view(np.float16).astype(np.float32), lo.view(np.float16).astype(np.float32)


def _round_f16(x):
    """fp32 -> the nearest fp16 value (ties to even, subnormals included), as fp32: x rounded to a multiple of max(2^(e - 11), 2^-24) for
    |x| in [2^(e-1), 2^e).  numpy's own cast is the same function (test_round_f16_is_numpys_cast) but takes a slow path for every result
    in fp16's subnormal range, which most probabilities of a row with logits of +-60 fall into.  |x| < 65504 here."""
    _, e = np.frexp(x)
    q = np.ldexp(np.float32(1), np.maximum(e - 11, -24)).astype(np.float32)
    return (np.rint(x / q) * q).astype(np.float32)


def _planes_fast(x):
    """_planes(x, 1) through _round_f16"""
    hi = _round_f16(x)
    return hi, _round_f16(x - hi)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; one rounding to fp32 at the end (up to a double rounding)"""
    return (np.asarray(a, dtype=np.float64) * np.float64(b) + np.float64(c)).astype(np.float32)


def emulate(qkv, n_img, ntok, heads, tile):
    """csrc/attention_stream_h2.hip through its operator entry, in numpy: one scale from the tensor's maximum; per (image, head) the key
    tiles in order; products smallest first; fp32 everywhere the kernel has fp32."""
    x = qkv.numpy().reshape(n_img, ntok, 3, heads, 64)
    s = np.float32(h2_restated.pow2_scale(np.abs(x).max(), 15))
    alpha = np.float32(0.125 * 1.44269504088896341 / (float(s) * float(s)))
    out_mul = np.float32(1.0 / 16384.0)            # output scale s / (s 2^14)
    hi, lo = _planes(x, s)
    out = np.empty((n_img, ntok, heads, 64), dtype=np.float32)
    key_tiles = -(-ntok // tile)
    for n in range(n_img):
        for h in range(heads):
            qh, ql = hi[n, :, 0, h], lo[n, :, 0, h]
            m = np.full(ntok, -np.inf, dtype=np.float32)
            l, m_shift = np.zeros(ntok, dtype=np.float32), np.zeros(ntok, dtype=np.float32)
            o = np.zeros((ntok, 64), dtype=np.float32)
            for kt in range(key_tiles):
                k0, k1 = kt * tile, min(ntok, (kt + 1) * tile)       # (padding keys: -inf before the maximum = left out)
                kh, kl, vh, vl = hi[n, k0:k1, 1, h], lo[n, k0:k1, 1, h], hi[n, k0:k1, 2, h], lo[n, k0:k1, 2, h]
                sc = ((qh @ kl.T + ql @ kh.T) + qh @ kh.T).astype(np.float32)
                m_new = np.maximum(m, sc.max(axis=1))
                shift = (-m_new * alpha).astype(np.float32)
                with np.errstate(invalid="ignore"):     # the rescale: the difference of the two ROUNDED shifts; 0 on the first tile
                    d = (shift - m_shift).astype(np.float32)
                    a = np.where(np.isneginf(m) | (d < -126.0), np.float32(0), np.exp2(np.maximum(d, np.float32(-126.0)))).astype(np.float32)
                m_shift = shift
                arg = _fma(sc, alpha, shift[:, None])
                e = np.where(arg < -126.0, np.float32(0), np.exp2(np.maximum(arg, np.float32(-126.0)))).astype(np.float32)   # v_exp_f32 gives no denormals
                l = (l * a + e.sum(axis=1, dtype=np.float32)).astype(np.float32)
                m = m_new
                ph, pl = _planes_fast(e * np.float32(16384.0))
                o = (o * a[:, None] + ((ph @ vl + pl @ vh) + ph @ vh)).astype(np.float32)
            assert float(np.abs(o).max()) < 2.0 ** 42
            scaled = (o * (out_mul / l)[:, None]).astype(np.float32)             # the output * s
            oh, ol = _planes(scaled, np.float32(1.0))
            out[n, :, h] = (oh + ol) * np.float32(1.0 / s)
    return torch.from_numpy(out.reshape(n_img * ntok, heads * 64))


def _norm_rel(got, ref64):
    return float(torch.linalg.norm(got.double() - ref64) / torch.linalg.norm(ref64))


def test_round_f16_is_numpys_cast(host_lib):
    """(a helper of the emulation below; it runs where the plan exists)"""
    assert _tile(host_lib) > 0
    g = np.random.default_rng(3)
    x = (g.standard_normal(200000) * np.exp2(g.uniform(-30, 12, 200000))).astype(np.float32)
    x = np.concatenate([x, np.float32([0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 16384.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])])
    assert np.array_equal(_round_f16(x), x.astype(np.float16).astype(np.float32))
    hi, lo = _planes(x, np.float32(1.0))
    fh, fl = _planes_fast(x)
    assert np.array_equal(hi, fh) and np.array_equal(lo, fl)


# the emulation runs at the key tile the kernel is built with, read from the plan (at 32 the same cases measured 0.79 .. 2.23)


def _references(qkv, n_img, ntok, heads):
    """vit_patch8_cases.attention_cpu in fp64 and fp32, one (image, head) at a time: the same inputs and the same torch operations as
    vit_patch8_cases.case, without its [images, heads, ntok, ntok] fp64 intermediates (1 GB at 6 x 12 x 785)"""
    x = qkv.reshape(n_img, ntok, 3, heads, 64)
    out = {torch.float64: torch.empty((n_img, ntok, heads, 64), dtype=torch.float64), torch.float32: torch.empty((n_img, ntok, heads, 64))}
    for n in range(n_img):
        for h in range(heads):
            one = x[n, :, :, h].reshape(ntok, 192)
            for dtype, o in out.items():
                o[n, :, h] = cases.attention_cpu(one, 1, ntok, 1, dtype)
    return out[torch.float64].reshape(n_img * ntok, heads * 64), out[torch.float32].reshape(n_img * ntok, heads * 64)


def _random_cases(tile):
    return cases.CASES + [(tile + 1, 1, 3), (4097, 1, 2)]


@pytest.mark.parametrize("scale", cases.SCALES)
def test_emulated_arithmetic_on_random_cases(host_lib, scale):
    tile = _tile(host_lib)
    for ntok, n_img, heads in _random_cases(tile):
        qkv = cases.random_qkv(ntok, n_img, heads, scale)
        ref64, cpu32 = _references(qkv, n_img, ntok, heads)
        got = emulate(qkv, n_img, ntok, heads, tile)
        rel, ratio = _norm_rel(got, ref64), cases.parity_ratio(got, ref64, cpu32)
        print(f"\nemulated f16x2 streaming attention ntok={ntok} {n_img}x{heads} scale {scale} tile {tile}: norm-rel {rel:.3e}, "
              f"x torch-CPU fp32's distance from fp64 {ratio:.3f}")
        assert rel < 1e-3, (ntok, n_img, heads, scale, rel)
        assert ratio <= cases.PARITY_CAP, (ntok, n_img, heads, scale, ratio)


@pytest.mark.parametrize("order", cases.KEY_ORDERS)
def test_emulated_arithmetic_on_constructed_key_orders(host_lib, order):
    tile = _tile(host_lib)
    qkv = cases.ordered_qkv(order)
    ref64, cpu32 = _references(qkv, 1, 785, 3)
    got = emulate(qkv, 1, 785, 3, tile)
    rel, ratio = _norm_rel(got, ref64), cases.parity_ratio(got, ref64, cpu32)
    print(f"\nemulated f16x2 streaming attention 785 keys {order} tile {tile}: norm-rel {rel:.3e}, ratio {ratio:.3f}")
    assert rel < 1e-3 and ratio <= cases.PARITY_CAP, (order, rel, ratio)
