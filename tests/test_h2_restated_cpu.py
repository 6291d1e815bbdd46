"""The numpy restatement of split2_pair (tests/h2_restated.py) against the bound csrc/h2.h states for the format: relative error
<= 2^-22 where |x s| >= 2^-3, absolute error <= 2^-25 / s below that - the anchor of the restatement the GPU tests of the plane
outputs compare the kernels with, independent of any kernel."""
import numpy as np
import pytest

from tests import h2_restated


def _values(seed):
    g = np.random.default_rng(seed)
    # |x s| from 2^-30 up to fp16's largest finite value, dense in every binade, plus the edges of the two regimes
    mag = np.exp2(g.uniform(-30, np.log2(65504.0), 200_000))
    xs = (mag * g.choice([-1.0, 1.0], mag.size)).astype(np.float32)
    edges = np.array([0.0, -0.0, 2.0 ** -3, np.nextafter(np.float32(2.0 ** -3), np.float32(0)), 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 65504.0,
                      1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -12, 2048.5, 16384.0, 32767.998], dtype=np.float32)
    return np.concatenate([xs, edges, -edges])


@pytest.mark.parametrize("log2_s", [-20, -1, 0, 7, 30])
def test_split2_keeps_the_bound_of_the_format(log2_s):
    s = np.float32(2.0 ** log2_s)
    x = (_values(log2_s + 100) / s).astype(np.float32)           # exact: a power of two, far from fp32's own limits
    hi, lo = h2_restated.split2(x, s)
    assert np.isfinite(hi.view(np.float16)).all() and np.isfinite(lo.view(np.float16)).all()
    back = (hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)) / float(s)
    err = np.abs(back - x.astype(np.float64))
    big = np.abs(x.astype(np.float64) * float(s)) >= 2.0 ** -3
    assert big.any() and (~big).any()
    assert (err[big] <= 2.0 ** -22 * np.abs(x[big].astype(np.float64))).all(), "relative bound 2^-22 missed at |x s| >= 2^-3"
    assert (err[~big] <= 2.0 ** -25 / float(s)).all(), "absolute bound 2^-25 / s missed below 2^-3"
    # the fp32 value the planes stand for is what join2 returns, and the sign of a zero survives in hi
    assert np.array_equal(h2_restated.join2(hi, lo, np.float32(1.0) / s).astype(np.float64), back)
    z = h2_restated.split2(np.array([0.0, -0.0], dtype=np.float32), s)
    assert z[0].tolist() == [0x0000, 0x8000] and z[1].tolist() == [0x0000, 0x0000]


def test_row_layout_round_trips():
    g = np.random.default_rng(5)
    hi = g.integers(0, 2 ** 16, (7, 64)).astype(np.uint16)
    lo = g.integers(0, 2 ** 16, (7, 64)).astype(np.uint16)
    rows = h2_restated.to_rows(hi, lo)
    assert rows.shape == (7, 128)
    assert np.array_equal(rows[:, :16], hi[:, :16]) and np.array_equal(rows[:, 16:32], lo[:, :16]) and np.array_equal(rows[:, 32:48], hi[:, 16:32])
    h2, l2 = h2_restated.from_rows(rows)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)


def test_pow2_scale_window():
    amax = np.array([0.0, 1.0, 0.999, 3.0, 2.0 ** -40, 12345.678])
    s = h2_restated.pow2_scale(amax, 14)
    assert s[0] == 1.0
    v = amax[1:] * s[1:]
    assert ((v >= 2.0 ** 13) & (v < 2.0 ** 14)).all() and (np.log2(s) == np.round(np.log2(s))).all()
