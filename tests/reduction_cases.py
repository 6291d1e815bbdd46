"""The cases and inputs of the reduction gates, shared by tests/test_reduction_bounds_cpu.py (numpy replays of the kernels' summation
orders) and tests/test_gpu_reductions.py (the kernels): numpy only.

Inputs.  A channel is offset + spread * N(0, 1); the (offset, spread) pairs cycle over the channels through PAIRS: centred, a mean of the
order of the spread, means 2 and 100 spreads away (the std's two-pass form must not cancel), a tight channel far from zero and a small
one.  Special channels: channel 0 all negative (a max that starts from 0 instead of -inf shows), channel 1 constant at 1.5 (partial sums
exact: mean and max are exactly 1.5, the std exactly 0), and from channel 2 on one channel per PLANTED position of the reduced axis, whose
element there is offset + 64 * spread - an element a kernel drops moves that channel's mean by 64 spread / count and its std far more.
Two images per call, with different data.
"""
import numpy as np

from tests import reduction_bounds as RB

PAIRS = ((0.0, 1.0), (0.3, 1.0), (2.0, 1.0), (100.0, 1.0), (-30.0, 0.01), (0.0, 1e-3))
PLANT = 64.0
CONSTANT = 1.5
N_IMG = 2

GAP_HW = (1, 17, 49, 135, 391, 392, 393, 589, 3137, 12544)      # every split count transition (S = 1 | 2 | 3 | 16) and ragged per
GAP_CASES = [(hw, c) for hw in GAP_HW for c in (64, 128)]
TOKEN_CASES = [(count, dim) for count in (1, 2, 3, 4, 5, 7, 196, 784) for dim in (64, 192, 768)] + [(4096, 192)]
POOL_CASES = [(dim, n) for dim in (2048, 4096) for n in (1, 3, 300)]


def gap_planted(hw):
    """first and last pixel of the map and of every split"""
    s, per = RB.gap_split(hw)
    pos = {0, hw - 1}
    for sp in range(s):
        if sp * per < hw:
            pos |= {sp * per, min((sp + 1) * per, hw) - 1}
    return sorted(pos)


def token_planted(count):
    return sorted({0, count - 1})


def pool_planted(dim):
    return [0, 255, dim - 256, dim - 1]


def columns(n_img, count, channels, planted, seed):
    """-> (x fp32 [n_img, count, channels], reduced over axis 1; kinds: per channel "negative" | "constant" | ("planted", position) | "plain")"""
    assert 2 + len(planted) <= channels, (planted, channels)
    rng = np.random.RandomState(seed)
    off = np.array([PAIRS[c % len(PAIRS)][0] for c in range(channels)])
    spread = np.array([PAIRS[c % len(PAIRS)][1] for c in range(channels)])
    x = off + spread * rng.standard_normal((n_img, count, channels))
    x[:, :, 0] = -0.5 - np.abs(rng.standard_normal((n_img, count)))
    x[:, :, 1] = CONSTANT
    kinds = ["negative", "constant"]
    for k, pos in enumerate(planted):
        x[:, pos, 2 + k] = off[2 + k] + PLANT * spread[2 + k]
        kinds.append(("planted", pos))
    kinds += ["plain"] * (channels - len(kinds))
    return np.ascontiguousarray(x.astype(np.float32)), kinds


def gap_input(hw, c):
    return columns(N_IMG, hw, c, gap_planted(hw), seed=100003 * hw + c)


def token_input(count, dim):
    return columns(N_IMG, count, dim, token_planted(count), seed=7 + 100019 * count + dim)


# pool vectors: the rows take the kinds below in order, so n = 1 is the vector with its last element planted, n = 3 adds the all-negative
# and the constant vector, and n = 300 runs every kind many times over
def pool_row_kinds(dim):
    p = pool_planted(dim)
    return ([("planted", p[3]), "negative", "constant", ("plain", 3), ("planted", p[0]), ("planted", p[1]), ("planted", p[2])]
            + [("plain", k) for k in (0, 1, 2, 4, 5)])


def pool_input(dim, n):
    """-> (v fp32 [n, dim], kinds per row)"""
    rng = np.random.RandomState(31 * dim + n)
    table = pool_row_kinds(dim)
    v = np.empty((n, dim), dtype=np.float64)
    kinds = []
    for i in range(n):
        kind = table[i % len(table)]
        off, spread = PAIRS[kind[1] if kind[0] == "plain" else i % len(PAIRS)]
        v[i] = off + spread * rng.standard_normal(dim)
        if kind == "negative":
            v[i] = -0.5 - np.abs(rng.standard_normal(dim))
        elif kind == "constant":
            v[i] = CONSTANT
        elif kind[0] == "planted":
            v[i, kind[1]] = off + PLANT * spread
        kinds.append(kind if kind[0] != "plain" else "plain")
    return np.ascontiguousarray(v.astype(np.float32)), kinds
