"""The gate of tests/fp32_grade.py on synthetic data (no GPU): it accepts fp32 rounding noise and a faithful numpy model of the
f16x2 arithmetic, and rejects the defects it exists to catch - one dropped cross product, a scale off by 2^-16 on some rows."""
import numpy as np
import pytest

from tests import fp32_grade


def _dot64(X, Y):
    """X [M, K] . Y [N, K]^T in float64 by numpy's own summation loops (einsum without BLAS): the same bits on every host, and no
    BLAS thread pool started by this test."""
    return np.einsum("mk,nk->mn", np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64))


def _fp32_chain(A, W):
    """An fp32 dot-product chain: every partial sum rounded to fp32, one k at a time."""
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc + np.outer(A[:, k], W[:, k]).astype(np.float32)).astype(np.float32)
    return acc


def _planes(X):
    """csrc/h2.h per row: s = the power of two that puts the row maximum into [2^14, 2^15); hi = fp16(x s), lo = fp16(x s - hi)."""
    amax = np.abs(X).max(axis=1, keepdims=True)
    _, ex = np.frexp(amax)
    s = np.where(amax > 0, np.exp2((15 - ex).astype(np.float64)), 1.0).astype(np.float32)
    v = (X * s).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), s.astype(np.float64)


def _f16x2(A, W, drop_al_bh=False, row_scale_error=None):
    """The four partial products of each 32-k chunk summed exactly (fp16 x fp16 products are exact in fp32) and the fp32 accumulator
    rounded once per chunk - the MFMA's behaviour; then the power-of-two inverse scales."""
    ah, al, sa = _planes(A)
    bh, bl, sb = _planes(W)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, A.shape[1], 32):
        c = slice(k0, k0 + 32)
        part = _dot64(al[:, c], bl[:, c]) + _dot64(ah[:, c], bl[:, c]) + _dot64(ah[:, c], bh[:, c])
        if not drop_al_bh:
            part = part + _dot64(al[:, c], bh[:, c])
        acc = (acc.astype(np.float64) + part).astype(np.float32)
    rs = 1.0 / sa
    if row_scale_error is not None:
        rs = rs * row_scale_error[:, None]
    return (acc.astype(np.float64) * rs * (1.0 / sb).T).astype(np.float32)


def _problem(seed, M=96, N=64, K=512, row_spread=True):
    g = np.random.default_rng(seed)
    A = g.standard_normal((M, K)).astype(np.float32)
    if row_spread:
        A *= np.exp2(g.integers(-6, 7, (M, 1))).astype(np.float32)    # rows of different size: per-row scales matter
    W = (g.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    return A, W, _dot64(A, W), _dot64(np.abs(A), np.abs(W))


@pytest.mark.parametrize("seed", [0, 1])
def test_gate_accepts_fp32_rounding_noise_and_a_faithful_f16x2_model(seed):
    A, W, ref, mag = _problem(seed)
    chain = _fp32_chain(A, W)
    assert fp32_grade.normalised_error(chain, ref, mag).max() > 0           # (the chain does round: the comparison is not vacuous)
    fp32_grade.check(chain, chain, ref, mag, "the fp32 chain against itself")
    fp32_grade.check(ref.astype(np.float32), chain, ref, mag, "fp64 rounded once to fp32")
    mean_ratio, max_ratio, _ = fp32_grade.check(_f16x2(A, W), chain, ref, mag, "numpy model of f16x2")
    assert mean_ratio < 1.0 and max_ratio < 1.0


@pytest.mark.parametrize("seed", [0, 1])
def test_gate_rejects_a_dropped_cross_product(seed):
    """Without al.bh every product is off by about 2^-12 of itself: inside the 1e-3 norm-relative bar of the features, far outside
    the gate."""
    A, W, ref, mag = _problem(seed, row_spread=False)
    bad = _f16x2(A, W, drop_al_bh=True)
    assert np.linalg.norm(bad - ref) / np.linalg.norm(ref) < 1e-3
    with pytest.raises(AssertionError):
        fp32_grade.check(bad, _fp32_chain(A, W), ref, mag, "f16x2 without al.bh")


def test_gate_rejects_a_row_scale_off_by_2_pow_minus_16_on_a_few_rows():
    """The size of a tail-tile defect: 1 + 2^-16 on 8 of 96 rows (the rest exact)."""
    A, W, ref, mag = _problem(3)
    err = np.ones(A.shape[0])
    err[-8:] = 1.0 + 2.0 ** -16
    bad = _f16x2(A, W, row_scale_error=err)
    with pytest.raises(AssertionError, match="above"):
        fp32_grade.check(bad, _fp32_chain(A, W), ref, mag, "scale off on the tail rows")


def test_gate_rejects_nonzero_output_where_every_term_is_zero():
    A, W, ref, mag = _problem(4, M=8)
    A[3] = 0
    ref, mag = _dot64(A, W), _dot64(np.abs(A), np.abs(W))
    chain = _fp32_chain(A, W)
    fp32_grade.check(chain, chain, ref, mag, "zero row")
    bad = chain.copy()
    bad[3, 5] = 1e-30
    with pytest.raises(AssertionError, match="non-finite output, or a nonzero"):
        fp32_grade.check(bad, chain, ref, mag, "zero row, one stray value")


def test_gemm_mag_adds_bias_and_residual_magnitudes():
    A, W = np.array([[1.0, -2.0]]), np.array([[3.0, 4.0], [-1.0, 0.5]])
    got = fp32_grade.gemm_mag(A, W, bias=np.array([-1.0, 2.0]), residual=np.array([[0.5, -0.25]]))
    assert np.array_equal(got, [[1 * 3 + 2 * 4 + 1 + 0.5, 1 * 1 + 2 * 0.5 + 2 + 0.25]])


def test_attention_mag_layout():
    v_max = np.array([[1.0, 2.0], [3.0, 4.0]])
    m = fp32_grade.attention_mag(v_max, rows_per_img=3, head_dim=2)
    assert m.shape == (6, 4)
    assert (m[:3, :2] == 1).all() and (m[:3, 2:] == 2).all() and (m[3:, :2] == 3).all() and (m[3:, 2:] == 4).all()
