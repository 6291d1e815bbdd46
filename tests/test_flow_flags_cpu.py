"""The two flag bits of relax_optical_flow_flags, the part that needs no GPU: the definitions of tests/flow_flag_ref.py against
scipy.ndimage.correlate1d and exact area integration, relax_flow_gauss_window and relax_flow_area_table against them, every refusal of the new
entry naming its value (the rules are checked before the handle is looked at), the host code under AddressSanitizer + UBSan as a stand-alone
program, and the input conditions of tests/test_gpu_flow_flags.py: every gated case is well posed and every initial field matters."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import _lib
from tests import flow_cases as fc
from tests import flow_flag_cases as gc
from tests import flow_flag_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")
INVALID = -1      # RELAX_ERR_INVALID
WINDOWS = list(range(3, 64, 2))
AREA_PAIRS = [(131, 66), (131, 33), (264, 33), (97, 48), (97, 78), (131, 105)]      # the pairs the definitions were tried on
AREA_GRID = AREA_PAIRS + [(97, 97), (256, 32), (16, 16), (2200, 16), (2160, 68), (1920, 60), (1080, 34), (97, 40), (131, 54), (97, 35), (131, 47),
                          (2200, 2090), (33, 32), (1001, 1000), (2199, 1100)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_window_is_scipys_correlate1d_with_nearest_borders_on_the_same_taps(dtype):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(5)
    for ws, (h, w) in [(3, (16, 23)), (9, (17, 65)), (15, (40, 31)), (33, (16, 70)), (63, (20, 37)), (63, (97, 131))]:
        M = g.normal(0, 50, (h, w, 5)).astype(np.float32)
        half = fr.gauss_window(ws).astype(np.float64)
        full = np.concatenate([half[:0:-1], half])
        want = ndimage.correlate1d(ndimage.correlate1d(M.astype(np.float64), full, axis=0, mode="nearest"), full, axis=1, mode="nearest")
        got = fr.gauss_window_planes(M, ws, dtype)
        assert got.dtype == dtype
        tol = 1e-11 if dtype == np.float64 else 2.0 ** -23 * (ws + 4)      # float passes: 2 m + 1 roundings of a sum bounded by max |M|
        assert np.abs(got - want).max() <= tol * np.abs(M).max(), (ws, h, w, np.abs(got - want).max())


def test_the_window_taps_are_as_stated():
    for ws in WINDOWS:
        k = fr.gauss_window(ws).astype(np.float64)
        assert abs(k[0] + 2 * k[1:].sum() - 1) < 1e-6 and (np.diff(k) < 0).all() and k[-1] > 0
    k = fr.gauss_window(63).astype(np.float64)
    assert abs(k[-1] / k[0] - np.exp(-31 * 31 / (2 * 9.3 * 9.3))) < 1e-6 and 3.8e-3 < k[-1] / k[0] < 4.0e-3     # the outermost tap still counts


@pytest.mark.parametrize("src,dst", AREA_PAIRS, ids=[f"{s}to{d}" for s, d in AREA_PAIRS])
def test_the_area_table_is_exact_area_integration(src, dst):
    """To 1e-14 against the area integral in float64; against the same integral from integer arithmetic the bound is what d * S in double
    allows, src * 2^-52 (measured: 1.1e-14 at 131 -> 105, so 1e-14 does not hold against that one)."""
    A = fr.area_table(src, dst)
    err, err_exact = np.abs(A - fr.area_integration_matrix(src, dst)).max(), np.abs(A - fr.exact_area_matrix(src, dst)).max()
    print(f"{src} -> {dst}: {err:.2e} from the float64 integral, {err_exact:.2e} from the integer one")
    assert err < 1e-14 and np.abs(A.sum(axis=1) - 1).max() < 1e-14
    assert err_exact < src * 2.0 ** -52


def test_the_area_table_with_equal_sizes_is_a_copy_and_resize_area_averages_blocks():
    assert np.array_equal(fr.area_table(97, 97), np.eye(97))
    g = np.random.default_rng(1)
    img = g.normal(0, 3, (256, 264, 2))
    want = img.reshape(32, 8, 33, 8, 2).mean(axis=(1, 3))
    assert np.abs(fr.resize_area(img, 32, 33) - want).max() < 1e-13


def test_farneback_flags_without_flags_is_the_oracle():
    from oracle import flow_ref
    a, b = fc.make_pair(gc.pc.pair_case(gc.SMALL, gc.SMOOTH))
    ga, gb = flow_ref.bgr2gray(a), flow_ref.bgr2gray(b)
    assert np.array_equal(fr.farneback_flags(ga, gb), flow_ref.farneback(ga, gb))


# ---- the host entries --------------------------------------------------------------------------------------------------------------------
def test_relax_flow_gauss_window_is_within_one_ulp_of_the_numpy_taps(lib):
    for ws in WINDOWS:
        want = fr.gauss_window(ws)
        got = np.full(ws // 2 + 2, -7.0, np.float32)
        assert lib.relax_flow_gauss_window(ws, got.ctypes.data_as(C.c_void_p)) == 0
        assert got[-1] == -7.0                                                       # winsize / 2 + 1 floats written, no more
        assert (np.abs(got[:-1] - want) <= np.spacing(want)).all(), (ws, got[:-1], want)
    buf = np.zeros(40, np.float32)
    for bad in (1, 2, 14, 65, 0, -3):
        assert lib.relax_flow_gauss_window(bad, buf.ctypes.data_as(C.c_void_p)) == INVALID
        assert f"winsize={bad}" in lib.relax_last_error(None).decode()
    assert lib.relax_flow_gauss_window(15, None) == INVALID and "NULL" in lib.relax_last_error(None).decode()


def _c_table(lib, src, dst):
    taps = src // dst + 2
    first, count = np.full(dst, -1, np.int32), np.full(dst, -1, np.int32)
    weights = np.full((dst, taps), np.nan)
    rc = lib.relax_flow_area_table(src, dst, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.relax_last_error(None).decode()
    return first, count, weights


@pytest.mark.parametrize("src,dst", AREA_GRID, ids=[f"{s}to{d}" for s, d in AREA_GRID])
def test_relax_flow_area_table_equals_the_numpy_table(lib, src, dst):
    first, count, weights = _c_table(lib, src, dst)
    wf, wc, ww = fr.area_table_sparse(src, dst)
    assert np.array_equal(first, wf) and np.array_equal(count, wc)
    assert (count >= 1).all() and (first >= 0).all() and (first + count <= src).all() and (count <= src // dst + 2).all()
    for d in range(dst):
        assert np.abs(weights[d, :count[d]] - ww[d, :count[d]]).max() <= 1e-15, d
    if dst == src:
        assert (count == 1).all() and np.array_equal(first, np.arange(src)) and (weights[:, 0] == 1.0).all()


def test_relax_flow_area_table_refusals(lib):
    i, d = np.zeros(64, np.int32), np.zeros(256)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for src, dst in [(16, 17), (16, 0), (0, 0), (16, -1)]:
        assert lib.relax_flow_area_table(src, dst, p(i), p(i), p(d)) == INVALID
        msg = lib.relax_last_error(None).decode()
        assert f"src={src}" in msg and f"dst={dst}" in msg, msg
    assert lib.relax_flow_area_table(16, 16, None, p(i), p(d)) == INVALID and "NULL" in lib.relax_last_error(None).decode()


# ---- the refusals of the new entry -------------------------------------------------------------------------------------------------------
LITERALS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)
RULES = [
    ({"winsize": 14}, ["winsize=14", "even"]), ({"winsize": 65}, ["winsize=65", "3..63"]), ({"winsize": 1}, ["winsize=1"]),
    ({"poly_n": 6}, ["poly_n=6"]), ({"poly_n": 9}, ["poly_n=9"]),
    ({"pyr_scale": 0.49}, ["pyr_scale=0.49"]), ({"pyr_scale": 1.0}, ["pyr_scale=1"]), ({"pyr_scale": float("nan")}, ["pyr_scale=nan"]),
    ({"iterations": 0}, ["iterations=0"]), ({"iterations": 11}, ["iterations=11"]),
    ({"levels": 9}, ["levels=9"]), ({"levels": -1}, ["levels=-1"]),
    ({"poly_sigma": 0.0}, ["poly_sigma=0"]), ({"poly_sigma": float("nan")}, ["poly_sigma=nan"]), ({"poly_sigma": -1.0}, ["poly_sigma=-1"]),
    ({"flags": 1}, ["flags=1"]), ({"flags": 2}, ["flags=2"]), ({"flags": 8}, ["flags=8"]), ({"flags": 261}, ["flags=261"]),
    ({"flags": 512}, ["flags=512"]), ({"flags": 264}, ["flags=264"]), ({"flags": -1}, ["flags=-1"]),
]
SOME_FIELD = C.c_void_p(64)        # a non-NULL init_flow: never read, the rules come first


def _flags_without_handle(lib, p, init=None):
    return lib.relax_optical_flow_flags(None, None, None, 0, 1, 64, 64, p["pyr_scale"], p["levels"], p["winsize"], p["iterations"], p["poly_n"],
                                        p["poly_sigma"], p["flags"], init, None, None, None)


@pytest.mark.parametrize("bad,words", RULES, ids=[f"{k}={v}" for b, _ in RULES for k, v in b.items()])
@pytest.mark.parametrize("base_flags", [0, 256], ids=["box", "gauss"])
def test_every_refusal_names_its_value(lib, base_flags, bad, words):
    assert _flags_without_handle(lib, {**LITERALS, "flags": base_flags, **bad}) == INVALID
    msg = lib.relax_last_error(None).decode()
    assert msg.startswith("relax_optical_flow_flags: ") and all(w in msg for w in words), msg
    if "flags" in bad:
        assert "not to an OpenCV build" in msg, msg


def test_the_parameter_rules_have_the_wording_of_the_ex_entry(lib):
    for bad, _ in RULES:
        if "flags" in bad:
            continue
        p = {**LITERALS, **bad}
        assert _flags_without_handle(lib, {**p, "flags": 260}, SOME_FIELD) == INVALID
        new = lib.relax_last_error(None).decode()
        assert lib.relax_optical_flow_ex(None, None, None, 0, 1, 64, 64, p["pyr_scale"], p["levels"], p["winsize"], p["iterations"], p["poly_n"],
                                         p["poly_sigma"], 0, None, None, None) == INVALID
        old = lib.relax_last_error(None).decode()
        assert new.split(": ", 1)[1] == old.split(": ", 1)[1], (new, old)


def test_a_missing_and_a_surplus_initial_flow_are_refused_by_name(lib):
    for flags in (4, 260):
        assert _flags_without_handle(lib, {**LITERALS, "flags": flags}, None) == INVALID
        msg = lib.relax_last_error(None).decode()
        assert f"flags={flags}" in msg and "init_flow is NULL" in msg and "OPTFLOW_USE_INITIAL_FLOW" in msg, msg
    for flags in (0, 256):
        assert _flags_without_handle(lib, {**LITERALS, "flags": flags}, SOME_FIELD) == INVALID
        msg = lib.relax_last_error(None).decode()
        assert f"flags={flags}" in msg and "init_flow is given" in msg and "OPTFLOW_USE_INITIAL_FLOW" in msg, msg


def test_accepted_sets_stop_at_the_missing_handle(lib):
    sets = [p for p, _ in gc.SETS.values()] + [{**LITERALS, "flags": f} for f in (0, 4, 256, 260)]
    sets.append(dict(pyr_scale=0.95, levels=8, winsize=63, iterations=10, poly_n=7, poly_sigma=1e-3, flags=260))
    for p in sets:
        assert _flags_without_handle(lib, p, SOME_FIELD if p["flags"] & 4 else None) == INVALID
        assert lib.relax_last_error(None).decode() == "relax_optical_flow_flags: the handle is NULL", p


def test_the_old_entry_still_refuses_both_bits_and_the_header_says_what_pins_the_modes(lib):
    for flags, word in [(4, "OPTFLOW_USE_INITIAL_FLOW"), (256, "OPTFLOW_FARNEBACK_GAUSSIAN"), (260, "OPTFLOW_FARNEBACK_GAUSSIAN")]:
        assert lib.relax_optical_flow_ex(None, None, None, 0, 1, 64, 64, 0.5, 3, 15, 3, 5, 1.2, flags, None, None, None) == INVALID
        assert word in lib.relax_last_error(None).decode()
    assert lib.relax_abi_version() == 1
    text = open(os.path.join(ROOT, "include", "relax_hip.h")).read()
    assert "#define RELAX_FLOW_GAUSSIAN 256" in text and "#define RELAX_FLOW_USE_INITIAL 4" in text
    assert "NOT TO AN OPENCV BUILD" in text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "relax_optical_flow_flags" in readme and "not to an OpenCV build" in readme


def test_gauss_window_area_table_and_flag_rules_under_address_and_ub_sanitizers():
    """host_logic.cpp with its own main (make flow_flags_san): every window and a grid of area tables into heap arrays of exactly the stated
    sizes."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no AddressSanitizer")
    subprocess.run(["make", "-C", CSRC, "flow_flags_san"], check=True, capture_output=True)
    res = subprocess.run([os.path.join(CSRC, "flow_flags_san")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.startswith("flow_flags ok") and "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- the inputs of the GPU parity gates ----------------------------------------------------------------------------------------------------
GATED = gc.gated_cases()


@pytest.mark.parametrize("item", GATED, ids=[gc.gated_id(i) for i in GATED])
def test_every_gated_case_meets_its_posedness_rule(item):
    """Cases gated in full: max |reference fp32 - reference fp64| < 1e-3 (flow_param_cases.WELL_POSED).  The one case gated on the mean term
    alone (gauss15, smooth, 256 x 264: max 5.2e-3): at most one component in a thousand beyond 1e-3 and a mean distance under 1e-5."""
    name, case, kind = item
    f64, f32 = gc.reference(name, case)
    d = np.abs(f32.astype(np.float64) - f64)
    print(f"{gc.gated_id(item)}: max |fp32 - fp64| {d.max():.2e}, mean {d.mean():.2e}, share past 1e-3 {(d >= gc.WELL_POSED).mean():.2e}, "
          f"max |flow| {np.abs(f64).max():.1f}")
    assert np.isfinite(f64).all() and np.isfinite(f32).all()
    if kind == "mean":
        assert float((d >= gc.WELL_POSED).mean()) <= gc.OUTLIER_SHARE and d.mean() < 1e-5, (float((d >= gc.WELL_POSED).mean()), d.mean())
    else:
        assert d.max() < gc.WELL_POSED, d.max()


@pytest.mark.parametrize("name", gc.INIT_SETS)
def test_every_initial_field_matters_on_at_least_one_gated_case(name):
    """The float64 reference differs from the same parameters without the initial flow by a mean of 0.1 px or more on at least one gated case
    (the iterations converge a starting point away: the smooth pair is poor evidence, the noise pair carries it)."""
    effects = {}
    for n, case, _ in GATED:
        if n == name:
            with_init = gc.reference(name, case)[0]
            without = gc.reference(name, case, flags=gc.SETS[name][0]["flags"] & ~4)[0]
            effects[fc.case_id(case)] = float(np.abs(with_init - without).mean())
            field = gc.initial_field(name, case)
            assert np.ptp(field[..., 0]) >= 2 * gc.AMPLITUDE - 1e-3 and np.ptp(field[..., 1]) >= 2 * gc.AMPLITUDE - 1e-3
    print(name, effects)
    assert max(effects.values()) >= gc.INIT_EFFECT, effects


def test_the_wrong_mode_references_are_far_from_the_right_ones():
    """What the GPU sensitivity check relies on: the box reference at gauss33's six parameters, and a reference without its initial flow, are
    far from the right reference in units of the float32 reference's own distance."""
    case = gc.pc.pair_case(gc.SMALL, gc.SMOOTH)
    f64, f32 = gc.reference("gauss33", case)
    b64, b32 = gc.reference("gauss33", case, flags=0)
    assert fc.parity_ratio(f32, b64, b32) > 64 * fc.PARITY_CAP
    case = gc.pc.pair_case(gc.SMALL, gc.SECOND)
    for name in ("init_lit", "init_l0"):
        f64, f32 = gc.reference(name, case)
        z64, z32 = gc.reference(name, case, flags=0)
        assert fc.parity_ratio(f32, z64, z32) > 64 * fc.PARITY_CAP, name


def test_parity_gate_follows_the_recorded_worst_ratio():
    gate = gc.parity_gate()
    assert gate in (1.0, 2.0, 4.0, 8.0) and gate <= fc.PARITY_CAP
