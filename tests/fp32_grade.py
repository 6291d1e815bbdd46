"""The fp32-grade gate of the contraction kernels (numpy only).

The claim (include/relax_hip.h, README's accuracy row): against an fp64 reference, the split-operand arithmetics (f16x2, bf16x6) are
no further away than the exact-fp32 path - an fp32 FMA chain - run on the SAME inputs.  An element's error is measured against the
sum of the magnitudes that went into it,

    e = |got - ref| / mag,     mag = |A| @ |W|^T + |bias| + |residual|     (a convolution: conv(|x|, |w|) + |bias| + |residual|),

the scale every rounding of a dot product is proportional to: an output that cancels to near zero keeps the absolute error of its
large terms, and an rtol on it means nothing.  Three bounds, all of which must hold:

    max e  <= 2^-20                                   (absolute: the 1e-6 of test_rows_of_very_different_size_and_sparse_rows)
    mean e <= C_MEAN * mean e32 + SLACK
    max e  <= C_MAX  * max e32  + SLACK

Why these catch a wrong kernel that an rtol of 1e-3 lets through: a dropped cross product of f16x2 (al bh), a dropped product of
bf16x6, or a scale off by 2^-16 leaves an error of 2^-12 .. 2^-16 of the products - 2^8 .. 2^12 times the 2^-24 per-product error
the fp32 chain (and a correct kernel) leaves, and far above 2^-20.

The constants.  A correct f16x2 kernel holds each operand to 22 bits (relative error <= 2^-23 each) and rounds its fp32 accumulator
once per 32 products; the fp32 chain rounds once per product.  At K >= 32 the chain's error is the larger one; the ratios measured on
random shapes are printed by tests/test_gpu_h2_random.py.  C_MEAN = 1.25 and C_MAX = 2.5 leave room for the noise of small outputs (a mean over
256 elements, a maximum over a few hundred), and stay 2^6 below what the defects above produce.  C_MAX was 2 at first; a 3x3
convolution with a single output pixel (64 outputs) measured 2.16: the maximum of 64 errors is a small-sample statistic on both
sides, and 2.5 keeps every mutant of the issue failing.

Two properties of the f16x2 FORMAT (not defects; measured on random shapes, and the bounds below are what holds):

  * Short K.  Each operand keeps 22 bits (relative error <= 2^-23), so one product carries up to 2^-22 of itself where the fp32 chain
    rounds it once (2^-24); over K products these errors add like a random walk, about 2^-23 / sqrt(K) of mag.  The fp32 chain's own
    error does not shrink with K, so at K >= 256 this term is far below it, but at K = 16 - or in an output that is ONE product (a
    single-nonzero row: K_eff = 1) - the chain has almost no accumulation error to compare with (measured: mean e 1.57 x the chain's
    at K = 16, max e 3.2 x on single products).  `h2_slack(K)` = 2^-23 / sqrt(K) is added to both bounds of an f16x2 contraction:
    1.2e-7 for a single product, 3e-8 at K = 16, 4.3e-9 at K = 768 - the defects above sit at 1e-6 and more.
  * Values far below their row's maximum.  A value below 2^-17 of the maximum of its row (image, tensor: whatever shares its scale)
    falls under the fp16 subnormal lo plane and keeps an ABSOLUTE error of 2^-39 of that maximum, not 22 bits of itself.  In a dense
    dot product mag hides it; an output made of one such product alone (a single-nonzero row of A against a tiny weight) does not.
    `h2_floor(row_max_a, row_max_w)` = 2^-17 |max a| |max w| added to mag states that bound (2^-22 of it): for a dense row it moves
    mag by 2^-15 of itself or less.

Attention has no sum of magnitudes of a single contraction: normalise by the maximum |v| of each (image, head) instead
(`attention_mag`) - an output row is a convex combination of V rows.  There is no absolute bound for it: the softmax multiplies the
logits' own rounding (2^-24 of |q . k| / 8, logits of hundreds at scale 5) into the output, in every fp32 arithmetic - the exact-fp32
path itself is 2.4e-6 of max |v| away at scale 3 - so only the comparison with that path is meaningful there.
"""
import numpy as np

MAX_ABS = 2.0 ** -20
C_MEAN = 1.25
C_MAX = 2.5
SLACK = 2.0 ** -30


def h2_slack(K):
    """The mean-bound allowance for the 22-bit operands of f16x2 over a contraction of length K (module docstring)."""
    return 2.0 ** -23 / np.sqrt(K)


def h2_floor(row_max_a, row_max_w):
    """[M] and [N] row maxima -> the [M, N] term 2^-17 |max a_m| |max w_n| added to mag for f16x2 (module docstring)."""
    return 2.0 ** -17 * np.outer(np.abs(np.asarray(row_max_a, dtype=np.float64)), np.abs(np.asarray(row_max_w, dtype=np.float64)))


def normalised_error(got, ref, mag):
    """|got - ref| / mag elementwise in float64.  Where mag == 0 every input term is zero, so the only right answer is ref itself
    (exactly 0): e is 0 there if got equals it and inf otherwise.  Non-finite outputs give inf."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    mag = np.broadcast_to(np.asarray(mag, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    pos = mag > 0
    return np.where(pos, err / np.where(pos, mag, 1.0), np.where(err == 0, 0.0, np.inf))


def gemm_mag(A, W, bias=None, residual=None):
    """|A| @ |W|^T + |bias| + |residual| in float64 (numpy arrays, A [M, K], W [N, K])."""
    mag = np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(np.asarray(W, dtype=np.float64)).T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    if residual is not None:
        mag = mag + np.abs(np.asarray(residual, dtype=np.float64))
    return mag


def attention_mag(v_max, rows_per_img, head_dim=64):
    """v_max [n_img, heads] (max |v| of each image and head) -> the per-element normaliser of the attention output
    [n_img * rows_per_img, heads * head_dim]."""
    v_max = np.asarray(v_max, dtype=np.float64)
    n_img, heads = v_max.shape
    return np.repeat(np.repeat(v_max, rows_per_img, axis=0), head_dim, axis=1).reshape(n_img * rows_per_img, heads * head_dim)


def check(got, got32, ref, mag, what, c_mean=C_MEAN, c_max=C_MAX, slack=SLACK, max_abs=MAX_ABS):
    """Asserts the three bounds for `got` (the kernel under test) against `got32` (the exact-fp32 path on the same inputs); `ref` the
    fp64 result, `mag` its sum of magnitudes (broadcastable); max_abs None: no absolute bound (attention).  Returns (mean e / mean e32, max e / max e32, max e) for the record
    (a ratio is 0 where both errors are 0)."""
    e = normalised_error(got, ref, mag)
    e32 = normalised_error(got32, ref, mag)
    assert np.isfinite(e32).all(), f"{what}: the exact-fp32 path itself is non-finite or wrong where mag == 0"
    assert np.isfinite(e).all(), f"{what}: non-finite output, or a nonzero where every input term is zero"
    me, me32, xe, xe32 = float(e.mean()), float(e32.mean()), float(e.max()), float(e32.max())
    detail = f"{what}: mean e {me:.3e} (fp32 {me32:.3e}), max e {xe:.3e} (fp32 {xe32:.3e}) at {np.unravel_index(int(e.argmax()), e.shape)}"
    assert max_abs is None or xe <= max_abs, f"{detail}: above the absolute bound {max_abs:.3e}"
    assert me <= c_mean * me32 + slack, f"{detail}: mean above {c_mean} x the fp32 path's"
    assert xe <= c_max * xe32 + slack, f"{detail}: max above {c_max} x the fp32 path's"
    return (me / me32 if me32 > 0 else 0.0), (xe / xe32 if xe32 > 0 else 0.0), xe
