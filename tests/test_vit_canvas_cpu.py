"""The ViT on any canvas, without a GPU: the restatement tests/vit_canvas_ref.forward_canvas against what the reference's own class
computed (tests/golden/vit_canvas.npz, tools/make_vit_canvas_golden.py), host::vit_canvas_geometry and host::pos_interp_taps through a
host build of csrc/host_logic.cpp, and the ctypes table."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import relax_vqa_amd  # noqa: F401
from tests import vit_canvas_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (case of the fixture, patch, grid)
GOLDEN_CASES = [("p16_96x160", 16, (6, 10)), ("p16_230x250", 16, (14, 15)), ("p16_112x448", 16, (7, 28)), ("p16_16x16", 16, (1, 1)),
                ("p8_64x40", 8, (8, 5))]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    return C.CDLL(str(out))


# ---- the restatement against the reference's class -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,patch,grid", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_restatement_matches_the_reference_class(golden_dir, name, patch, grid):
    """tolerance: the one tests/test_oracle_vit.py holds oracle.vit_ref to its ViT goldens with (rtol = atol = 1e-4)"""
    z = np.load(os.path.join(golden_dir, "vit_canvas.npz"))
    img = vit_canvas_ref.golden_input(z[f"{name}.shape"], z[f"{name}.seed"])
    assert int(img.sum(dtype=np.int64)) == int(z[f"{name}.sum"]), "the seeded input is not the recorded one"
    assert (img.shape[1] // patch, img.shape[2] // patch) == grid
    sd = vit_canvas_ref.golden_state_dict(z, patch)
    cls, tokens, attn = vit_canvas_ref.forward_canvas(sd, vit_canvas_ref.preprocess_bgr_u8(img), 1, patch)
    ntok = grid[0] * grid[1] + 1
    assert tuple(tokens.shape) == (1, ntok - 1, 64) and tuple(attn.shape) == (1, 1, ntok, ntok)
    np.testing.assert_allclose(cls.numpy(), z[f"{name}.cls"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(tokens.numpy(), z[f"{name}.tokens"], rtol=1e-4, atol=1e-4)
    attn = attn.numpy()
    if f"{name}.attn_rows" in z.files:
        attn = attn[:, :, z[f"{name}.attn_rows"]]
    np.testing.assert_allclose(attn, z[f"{name}.attn"], rtol=1e-4, atol=1e-4)


# ---- vit_canvas_geometry ---------------------------------------------------------------------------------------------------------------
def _canvas(lib, patch, Hc, Wc):
    out, err = (C.c_int * 5)(), C.create_string_buffer(512)
    rc = lib.relax_host_vit_canvas_geometry(patch, Hc, Wc, out, err, 512)
    return dict(zip(("gh", "gw", "npatch", "ntok", "identity"), out)) if rc == 0 else err.value.decode()


def test_canvas_geometry_floors_and_identity(host_lib):
    assert _canvas(host_lib, 16, 230, 250) == dict(gh=14, gw=15, npatch=210, ntok=211, identity=0)      # trailing 6 and 10 pixels ignored
    assert _canvas(host_lib, 16, 224, 224) == dict(gh=14, gw=14, npatch=196, ntok=197, identity=1)
    assert _canvas(host_lib, 16, 239, 225) == dict(gh=14, gw=14, npatch=196, ntok=197, identity=1)      # the grid decides, not the pixels
    assert _canvas(host_lib, 8, 224, 224) == dict(gh=28, gw=28, npatch=784, ntok=785, identity=1)
    assert _canvas(host_lib, 8, 112, 112) == dict(gh=14, gw=14, npatch=196, ntok=197, identity=0)       # 14 x 14 is not patch 8's table
    assert _canvas(host_lib, 16, 112, 448) == dict(gh=7, gw=28, npatch=196, ntok=197, identity=0)       # 196 patches, another grid
    assert _canvas(host_lib, 16, 448, 448) == dict(gh=28, gw=28, npatch=784, ntok=785, identity=0)
    assert _canvas(host_lib, 16, 270, 480) == dict(gh=16, gw=30, npatch=480, ntok=481, identity=0)
    assert _canvas(host_lib, 16, 16, 16) == dict(gh=1, gw=1, npatch=1, ntok=2, identity=0)
    for Hc in range(16, 80):
        for Wc in (16, 47, 48, 100):
            g = _canvas(host_lib, 16, Hc, Wc)
            assert (g["gh"], g["gw"], g["npatch"], g["ntok"]) == (Hc // 16, Wc // 16, (Hc // 16) * (Wc // 16), (Hc // 16) * (Wc // 16) + 1)


def test_canvas_geometry_refusals(host_lib):
    msg = _canvas(host_lib, 16, 15, 300)
    assert isinstance(msg, str) and re.search(r"\b15\b", msg) and "height" in msg, msg
    msg = _canvas(host_lib, 16, 300, 9)
    assert isinstance(msg, str) and re.search(r"\b9\b", msg) and "width" in msg, msg
    msg = _canvas(host_lib, 8, 7, 7)
    assert isinstance(msg, str) and re.search(r"\b7\b", msg), msg
    # the limit counts PATCHES: 4096 of them (4097 tokens with the class token), and the message says so
    assert _canvas(host_lib, 16, 1024, 1024) == dict(gh=64, gw=64, npatch=4096, ntok=4097, identity=0)
    assert _canvas(host_lib, 8, 512, 512) == dict(gh=64, gw=64, npatch=4096, ntok=4097, identity=0)
    msg = _canvas(host_lib, 16, 1040, 1040)
    assert isinstance(msg, str) and msg.count("1040") >= 2 and "4225 patches" in msg and "4096 patches" in msg and "4097 tokens" in msg, msg
    msg = _canvas(host_lib, 16, 1024, 1040)          # 64 x 65 = 4160
    assert isinstance(msg, str) and "1024" in msg and "1040" in msg and "4160 patches" in msg, msg
    msg = _canvas(host_lib, 8, 520, 512)
    assert isinstance(msg, str) and "520" in msg and "512" in msg, msg
    for p in (7, 32, 0):
        msg = _canvas(host_lib, p, 224, 224)
        assert isinstance(msg, str) and "8 or 16" in msg, msg
    assert isinstance(_canvas(host_lib, 16, 2 ** 30, 2 ** 30), str)     # no overflow on the way to the refusal


# ---- pos_interp_taps -------------------------------------------------------------------------------------------------------------------
def _taps(lib, side, g):
    idx, w = np.zeros(4 * g, dtype=np.int32), np.zeros(4 * g, dtype=np.float32)
    lib.relax_host_pos_interp_taps(side, g, idx.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
    return idx.reshape(g, 4), w.reshape(g, 4)


def _torch_interp(table, gh, gw, dtype):
    """table [side, side, d] numpy -> torch's [gh, gw, d] in `dtype`, called as the reference calls it"""
    side = table.shape[0]
    t = torch.from_numpy(table).to(dtype).permute(2, 0, 1)[None]
    out = F.interpolate(t, scale_factor=((gh + 0.1) / side, (gw + 0.1) / side), mode="bicubic")
    assert tuple(out.shape[-2:]) == (gh, gw)
    return out[0].permute(1, 2, 0).double().numpy()


INTERP_GRIDS = [1, 3, 5, 14, 15, 20, 28, 64]


@pytest.mark.parametrize("side", [14, 28])
def test_host_taps_reproduce_torch_fp32(host_lib, side):
    """The host taps applied in fp64 (rows with gh's taps, columns with gw's: the two axes are independent) against F.interpolate in fp32.
    Yardstick of a case: the distance between torch's own fp32 and fp64 results, which is the effect of evaluating the source coordinate
    in fp32.  Taps that round the coordinate as torch does reproduce the fp32 result to accumulation rounding - they must sit within HALF
    the yardstick of fp32; taps from exact coordinates would sit at the yardstick (at the fp64 result)."""
    table = np.random.default_rng(side).standard_normal((side, side, 8)).astype(np.float32)
    pairs = [(g, g) for g in INTERP_GRIDS] + [(3, 64), (15, 5), (28, 1), (7, 28)]
    for gh, gw in pairs:
        (iy, wy), (ix, wx) = _taps(host_lib, side, gh), _taps(host_lib, side, gw)
        assert iy.min() >= 0 and iy.max() <= side - 1 and ix.min() >= 0 and ix.max() <= side - 1
        t64 = table.astype(np.float64)
        rows = np.einsum("ya,yaxd->yxd", wy.astype(np.float64), t64[iy])                    # [gh, side, d]
        got = np.einsum("xb,yxbd->yxd", wx.astype(np.float64), rows[:, ix])                 # [gh, gw, d]
        f32, f64 = _torch_interp(table, gh, gw, torch.float32), _torch_interp(table, gh, gw, torch.float64)
        yard = np.abs(f32 - f64).max()
        err = np.abs(got - f32).max()
        print(f"side {side} grid {gh} x {gw}: |taps - torch fp32| {err:.3e}, yardstick |torch fp32 - fp64| {yard:.3e}")
        assert err <= 0.5 * yard, (side, gh, gw, err, yard)


def _fma32(a, b, c):
    """one fp32 fused multiply-add (the product of two fp32 values is exact in fp64; the sum is rounded once more, to fp32)"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _expected_taps(side, g):
    """host::pos_interp_taps restated in numpy fp32, rounding for rounding: fused coordinate, the cubics' Horner steps fused except the last
    step of each (a product rounded on its own, then the sum)"""
    f = np.float32
    A = f(-0.75)
    scale = f(1.0 / ((g + 0.1) / side))

    def conv1(x):
        return f(f(f(_fma32(A + f(2), x, -(A + f(3))) * x) * x) + f(1))

    def conv2(x):
        return f(f(_fma32(_fma32(A, x, f(-5) * A), x, f(8) * A) * x) - f(4) * A)

    idx, w = np.zeros((g, 4), dtype=np.int32), np.zeros((g, 4), dtype=np.float32)
    for i in range(g):
        real = _fma32(scale, f(i) + f(0.5), f(-0.5))
        fl = np.floor(real)
        t = f(min(max(f(real - fl), f(0)), f(1)))
        x2 = f(1) - t
        w[i] = [conv2(t + f(1)), conv1(t), conv1(x2), conv2(x2 + f(1))]
        idx[i] = [min(max(int(fl) - 1 + k, 0), side - 1) for k in range(4)]
    return idx, w


@pytest.mark.parametrize("side", [14, 28])
def test_host_taps_exactly(host_lib, side):
    """Indices and weights bit for bit against the numpy restatement, on every grid of the tests - the clamped border taps among them."""
    for g in INTERP_GRIDS + [7, 16, 30, 33, 60]:
        idx, w = _taps(host_lib, side, g)
        want_idx, want_w = _expected_taps(side, g)
        assert np.array_equal(idx, want_idx), (side, g)
        assert np.array_equal(w.view(np.uint32), want_w.view(np.uint32)), (side, g, np.abs(w - want_w).max())
        np.testing.assert_allclose(w.sum(axis=1), 1.0, atol=1e-6)          # cubic convolution weights sum to 1
        assert (w[:, 1:3] >= 0).all() and (w[:, [0, 3]] <= 0).all()        # A = -0.75: the inner taps positive, the outer ones negative
    # g = 1: one output in the middle of the table, nothing clamped
    assert _taps(host_lib, side, 1)[0].tolist() == [{14: [4, 5, 6, 7], 28: [11, 12, 13, 14]}[side]]
    # g = 64 (finer than the table): the first output sits at coordinate side / 64.1 / 2 - 0.5 < 0, floor -1: taps -2, -1, 0, 1 clamp to
    # 0, 0, 0, 1; the last one at 63.5 side / 64.1 - 0.5 = 13.37 / 27.24, floor side - 1: taps side - 2 .. side + 1 clamp the last two to side - 1
    idx, w = _taps(host_lib, side, 64)
    assert idx[0].tolist() == [0, 0, 0, 1] and idx[-1].tolist() == [side - 2, side - 1, side - 1, side - 1]
    t0 = np.float64(np.float32(1.0 / (64.1 / side))) * 0.5 - 0.5 + 1.0                     # the first output's fraction
    cubic = [((-0.75 * x + 3.75) * x - 6.0) * x + 3.0 for x in (t0 + 1, 2 - t0)], [(1.25 * x - 2.25) * x * x + 1 for x in (t0, 1 - t0)]
    np.testing.assert_allclose(w[0], [cubic[0][0], cubic[1][0], cubic[1][1], cubic[0][1]], atol=3e-7)


@pytest.mark.parametrize("side", [14, 28])
def test_host_weights_are_this_torch_builds_weights(host_lib, side):
    """Read torch's own fp32 weights off F.interpolate: a one-hot table (channel k = 1 at row k) resampled along the rows alone gives
    out[i, k] = the weight output i puts on row k.  On every output whose four taps lie inside the table the host weights equal them BIT FOR
    BIT with torch 2.10's x86-64 build; on a clamped output, where several taps share a row, their fp32 sum in tap order does.  Which fp32 operations a torch build fuses is its compiler's choice: if this assertion fails under
    another torch while test_host_taps_reproduce_torch_fp32 holds, the builds differ by an ulp or two of a weight - restate the roundings
    of the new build in host::pos_interp_taps and _expected_taps, or keep these and relax this test to that distance, saying so."""
    for g in INTERP_GRIDS:
        eye = torch.eye(side, dtype=torch.float32)[None, :, :, None].expand(1, side, side, 2).contiguous()
        out = F.interpolate(eye, scale_factor=((g + 0.1) / side, 1.0), mode="bicubic")[0, :, :, 0].T.numpy()       # [g, side]
        idx, w = _taps(host_lib, side, g)
        inside = 0
        for i in range(g):
            if len(set(idx[i].tolist())) == 4:                       # nothing clamped: each tap has a column of its own
                inside += 1
                assert np.array_equal(out[i, idx[i]].view(np.uint32), w[i].view(np.uint32)), (side, g, i, out[i, idx[i]] - w[i])
            else:                                                    # clamped: torch adds the weights that share a column, in tap order, in fp32
                for k in set(idx[i].tolist()):
                    acc = np.float32(0)
                    for a in range(4):
                        if idx[i, a] == k:
                            acc = np.float32(acc + w[i, a])
                    assert out[i, k].view(np.uint32) == acc.view(np.uint32), (side, g, i, k, out[i, k], acc)
            assert np.count_nonzero(out[i]) <= 4 and set(np.nonzero(out[i])[0].tolist()) <= set(idx[i].tolist())
        assert inside >= max(1, g - 16) and (g < 20 or inside < g), "no clamped row was checked at a fine grid"


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def test_ctypes_table_lists_the_canvas_entry_points():
    from relax_vqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "relax_hip.h")).read()
    assert re.search(r"#define RELAX_ABI_VERSION 1\b", header)
    ctype_of = {"relax_handle*": C.c_void_p, "const uint8_t*": C.c_void_p, "float*": C.c_void_p, "relax_stream": C.c_void_p, "int": C.c_int,
                "int*": C.POINTER(C.c_int)}
    for name in ("relax_vit_features_canvas", "relax_vit_pos_embed", "relax_vit_canvas_geometry"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in relax_hip.h"
        params = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and argtypes == [ctype_of[p] for p in params], (name, params)
    assert len(_lib.PROTOTYPES["relax_vit_features_canvas"][1]) == len(_lib.PROTOTYPES["relax_vit_features_ex"][1]) + 2
