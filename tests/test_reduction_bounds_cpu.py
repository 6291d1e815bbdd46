"""The gates of tests/reduction_bounds.py against numpy fp32 replays of the kernels' summation orders, on the case list the GPU test
runs (tests/reduction_cases.py): every correct replay is inside its gate, and each of five wrong replays - the slips these kernels can
have - is at least 8 x over its gate on at least one listed case, so the inputs separate right from wrong.  No GPU.

The replays keep the kernels' order operation for operation (numpy's fp32 element-wise operations round like the device's); the device
may contract `q += dv * dv` into a fused multiply-add, which takes one rounding out and stays inside the same gate.

  M1  gap_partial: per = HW / S instead of the ceiling (the pixels past S * per are dropped)
  M2  vit_token_stats: variance divided by count - 1
  M3  vit_token_stats: the squared-deviation loop stops at count - 1
  M4  rn_pool_stats: sqrtf(red[0] / (float)(D - 1))
  M5  rn_pool_stats: thread 255 leaves its last element out of the squared deviations
"""
import numpy as np
import pytest

from tests import reduction_bounds as RB
from tests import reduction_cases as RC

F = np.float32
SEPARATION = 8.0


# ---- replays ------------------------------------------------------------------------------------------------------------------------
def replay_gap(x, floor_per=False):
    """x fp32 [HW, C] -> the means [C] as gap_partial + gap_finish form them"""
    hw, c = x.shape
    s, per = RB.gap_split(hw)
    if floor_per:
        per = hw // s
    t = np.zeros(c, F)
    for sp in range(s):
        lo = sp * per
        hi = min(lo + per, hw)
        a = np.zeros((16, c), F)                       # the 16 lane groups stride the pixels
        for p0 in range(lo, hi, 16):
            rows = x[p0:min(p0 + 16, hi)]
            a[:len(rows)] += rows
        part = a[0].copy()                             # lanes 0..15 add the group sums in order
        for g in range(1, 16):
            part += a[g]
        t += part                                      # gap_finish: the partials in split order
    return t / F(hw)


def replay_gap_groups(x, group):
    """x fp32 [HW, C] -> the means as the epilogues' group sums + gap_groups_finish form them (rows of a group in order, groups in order)"""
    hw, c = x.shape
    sums = np.zeros((hw // group, c), F)
    for r in range(group):
        sums += x[r::group]
    t = np.zeros(c, F)
    for g in range(hw // group):
        t += sums[g]
    return t / F(hw)


def _four_groups(x):
    """the sums of tokens grp, grp + 4, ... per group, in order -> ((r0 + r1) + (r2 + r3))"""
    count, dim = x.shape
    r = np.zeros((4, dim), F)
    for p0 in range(0, count, 4):
        rows = x[p0:p0 + 4]
        r[:len(rows)] += rows
    return (r[0] + r[1]) + (r[2] + r[3])


def replay_token_stats(x, bessel=False, short_loop=False):
    """x fp32 [count, dim] -> (mean, max, std) [dim] as vit_token_stats forms them"""
    count = x.shape[0]
    mean = _four_groups(x) / F(count)
    dv = x - mean
    if short_loop:
        dv = dv[:count - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = _four_groups(dv * dv) / F(count - 1 if bessel else count)
        return mean, x.max(axis=0), np.sqrt(var)


def _tree256(vals):
    """vals fp32 [n, 256, D/256] -> red[0] [n]: a thread's elements in order onto 0.f, then the 8 levels of the LDS tree"""
    red = np.zeros(vals.shape[:2], F)
    for j in range(vals.shape[2]):
        red += vals[:, :, j]
    w = 128
    while w >= 1:
        red[:, :w] += red[:, w:2 * w]
        w >>= 1
    return red[:, 0]


def replay_pool_stats(v, bessel=False, drop_last=False):
    """v fp32 [n, D] -> (mean, max, std) [n] as rn_pool_stats<D> forms them"""
    n, dim = v.shape
    vals = v.reshape(n, dim // 256, 256).transpose(0, 2, 1)       # vals[t][j] = v[t + 256 j]
    mean = _tree256(vals) / F(dim)
    dv = vals - mean[:, None, None]
    q = dv * dv
    if drop_last:
        q[:, 255, -1] = 0
    return mean, v.max(axis=1), np.sqrt(_tree256(q) / F(dim - 1 if bessel else dim))


# ---- worst err / gate of a replay over one case ---------------------------------------------------------------------------------------
def gap_worst(hw, c, **mutant):
    x, _ = RC.gap_input(hw, c)
    got = np.stack([replay_gap(img, **mutant) for img in x])
    return float(RB.mean_ratio(got, x, 1, RB.l_gap(hw)).max())


def token_ratios(count, dim, **mutant):
    """-> err / gate of the means and of the stds, [image, channel]"""
    x, _ = RC.token_input(count, dim)
    L = RB.l_token_stats(count)
    mean, mx, std = (np.stack(t) for t in zip(*(replay_token_stats(img, **mutant) for img in x)))
    assert np.array_equal(mx, x.max(axis=1))
    return RB.mean_ratio(mean, x, 1, L), RB.std_ratio(std, x, 1, L)


def token_worst(count, dim, **mutant):
    mean, std = token_ratios(count, dim, **mutant)
    return float(mean.max()), float(std.max())


def pool_worst(dim, n, **mutant):
    v, _ = RC.pool_input(dim, n)
    L = RB.l_pool_stats(dim)
    mean, mx, std = replay_pool_stats(v, **mutant)
    assert np.array_equal(mx, v.max(axis=1))
    return float(RB.mean_ratio(mean, v, 1, L).max()), float(RB.std_ratio(std, v, 1, L).max())


# ---- the counts and the case list -------------------------------------------------------------------------------------------------------
def test_the_counts():
    assert [RB.gap_split(hw) for hw in RC.GAP_HW] == [(1, 1), (1, 17), (1, 49), (1, 135), (1, 391), (2, 196), (2, 197), (3, 197), (16, 197),
                                                     (16, 784)]
    assert RB.l_gap(49) == 4 + 15 + 1 + 1 and RB.l_gap(12544) == 49 + 15 + 16 + 1 and RB.l_gap(393) == 13 + 15 + 2 + 1
    assert RB.l_token_stats(1) == 4 and RB.l_token_stats(784) == 199 and RB.l_token_stats(5) == 5
    assert RB.l_pool_stats(2048) == 17 and RB.l_pool_stats(4096) == 25
    assert RB.l_gap_groups(3136, 16) == 16 + 196 + 1 and RB.l_gap_groups(196, 4) == 4 + 49 + 1
    assert RB.l_feature_mean(3136, "fp32") == RB.l_gap(3136) == 13 + 15 + 16 + 1
    assert RB.l_feature_mean(3136, "f16x2") == 4 + 784 + 1 and RB.l_feature_mean(33 * 34, "bf16x6") == RB.l_gap(33 * 34)


def test_the_inputs_are_what_the_cases_say():
    x, kinds = RC.gap_input(393, 64)
    assert x.shape == (2, 393, 64) and x.dtype == np.float32 and not np.array_equal(x[0], x[1])
    assert kinds[0] == "negative" and (x[:, :, 0] < 0).all() and kinds[1] == "constant" and (x[:, :, 1] == 1.5).all()
    assert [k[1] for k in kinds if k[0] == "planted"] == [0, 196, 197, 392] == RC.gap_planted(393)
    c = kinds.index(("planted", 392))
    off, spread = RC.PAIRS[c % 6]
    assert (x[:, 392, c] == np.float32(off + 64 * spread)).all()
    assert len(RC.gap_planted(12544)) == 32 and RC.gap_planted(1) == [0]
    v, kinds = RC.pool_input(2048, 300)
    assert v.shape == (300, 2048) and kinds[:3] == [("planted", 2047), "negative", "constant"] and (v[1] < 0).all() and (v[2] == 1.5).all()
    assert {k[1] for k in kinds if k[0] == "planted"} == {0, 255, 1792, 2047}
    assert len(RC.GAP_CASES) == 20 and len(RC.TOKEN_CASES) == 25 and len(RC.POOL_CASES) == 6


# ---- correct replays are inside the gates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,c", RC.GAP_CASES)
def test_gap_replay_is_inside_the_gate(hw, c):
    assert gap_worst(hw, c) <= 1.0
    x, kinds = RC.gap_input(hw, c)
    got = replay_gap(x[0])
    assert got[1] == np.float32(1.5)


@pytest.mark.parametrize("hw,group", [(3136, 16), (784, 16), (196, 4), (12544, 16), (12544, 4)])
def test_group_sum_replay_is_inside_its_gate(hw, group):
    x, _ = RC.columns(2, hw, 64, RC.gap_planted(hw), seed=hw + group)
    got = np.stack([replay_gap_groups(img, group) for img in x])
    assert RB.mean_ratio(got, x, 1, RB.l_gap_groups(hw, group)).max() <= 1.0


@pytest.mark.parametrize("count,dim", RC.TOKEN_CASES)
def test_token_stats_replay_is_inside_the_gates(count, dim):
    mean, std = token_worst(count, dim)
    assert mean <= 1.0 and std <= 1.0, (mean, std)
    x, _ = RC.token_input(count, dim)
    m, mx, s = replay_token_stats(x[0])
    assert m[1] == mx[1] == np.float32(1.5) and s[1] == 0
    if count == 1:
        assert np.array_equal(m, mx) and (s == 0).all()


@pytest.mark.parametrize("dim,n", RC.POOL_CASES)
def test_pool_stats_replay_is_inside_the_gates(dim, n):
    mean, std = pool_worst(dim, n)
    assert mean <= 1.0 and std <= 1.0, (mean, std)
    if n >= 3:
        m, mx, s = replay_pool_stats(RC.pool_input(dim, n)[0])
        assert m[2] == mx[2] == np.float32(1.5) and s[2] == 0 and mx[1] < 0


# ---- the five wrong replays are far outside -----------------------------------------------------------------------------------------------
def test_m1_floor_instead_of_ceil_in_gap_partial():
    over = {(hw, c): gap_worst(hw, c, floor_per=True) for hw, c in RC.GAP_CASES}
    print({k: f"{v:.3g}" for k, v in over.items()})
    assert max(over.values()) >= SEPARATION
    for (hw, c), r in over.items():            # every ragged map sees it; a map that divides by its split is the same computation
        s, _ = RB.gap_split(hw)
        assert (r >= SEPARATION) == (hw % s != 0), (hw, c, r)


def test_m2_variance_over_count_minus_one():
    over = {case: token_worst(*case, bessel=True)[1] for case in RC.TOKEN_CASES}
    print({k: f"{v:.3g}" for k, v in over.items()})
    # (count 1: 0 / 0, not finite.  At 4096 tokens the slip is 1.2e-4 of the std and the gate, with L = 1027, 6e-5: the large counts are
    # in the list for the loops and the planted tokens, the small ones for the divisor)
    assert all(r >= SEPARATION for (count, _), r in over.items() if count <= 784), over
    for count, dim in RC.TOKEN_CASES:      # the divisor is one expression for every count; where the gate is tight every channel sees it
        if 2 <= count <= 196:
            std = token_ratios(count, dim, bessel=True)[1]
            # (channel 1 is the constant one: its std is 0 either way.  The worst-conditioned channels, -30 +- 0.01, are 19 x over at 196 tokens)
            assert np.delete(std, 1, axis=1).min() >= SEPARATION, (count, dim)


def test_m3_squared_deviation_loop_one_token_short():
    over = {case: token_worst(*case, short_loop=True)[1] for case in RC.TOKEN_CASES if case[0] > 1}
    print({k: f"{v:.3g}" for k, v in over.items()})
    assert all(r >= SEPARATION for r in over.values()), over


def test_m4_pool_std_over_d_minus_one():
    over = {case: pool_worst(*case, bessel=True)[1] for case in RC.POOL_CASES}
    print({k: f"{v:.3g}" for k, v in over.items()})
    assert all(r >= SEPARATION for r in over.values()), over


def test_m5_pool_std_without_the_last_element():
    over = {case: pool_worst(*case, drop_last=True)[1] for case in RC.POOL_CASES}
    print({k: f"{v:.3g}" for k, v in over.items()})
    assert all(r >= SEPARATION for r in over.values()), over
