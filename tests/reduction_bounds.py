"""The fp32 rounding gates of the kernels that turn activations into the numbers a user receives: spatial means (gap_partial + gap_finish,
the fused group sums + gap_groups_finish: csrc/layers.hip), token statistics (vit_token_stats: csrc/vit.hip) and the pool vectors' tail
(rn_pool_stats<2048|4096>: csrc/resnet50.hip).  numpy only; tests/test_reduction_bounds_cpu.py holds the gates against replays of the
kernels' summation orders, tests/test_gpu_reductions.py holds the kernels against the gates.

The gates, u = 2^-24, ref = numpy fp64 on the same fp32 inputs.  L of an output = the fp32 additions on the longest path into it, + 1 for
the division (an addition onto the 0.f an accumulator starts from is exact, yet counted: the counts below are upper bounds).

  mean              |got - ref| <= L u (1 + L u) mean_i |x_i|
                    (every x_i passes through at most L roundings of relative size u: the first-order bound of any summation order, with
                    the factor that covers the second-order terms)
  population std    sigma = ref > 0:  |got - sigma| <= (L + 4) u sigma + (L u mean|x|)^2 / sigma
                    (two-pass form.  With the computed mean m = mu + d: sum (x - m)^2 = N sigma^2 + N d^2, so the mean's own error moves the
                    std by at most d^2 / (2 sigma), |d| <= L u mean|x| - the second term; subtraction, square, the L - 1 additions, the
                    division and the square root move it by less than (L + 4) u relative - the first.)
                    sigma = 0 (all x_i equal c): x_i - m = -d exactly, so got = |d| (1 + ...) <= L u (1 + (L + 4) u) |c|; where c has exact
                    partial sums (c = 1.5) d = 0 and the tests ask for exactly 0.
  max, copies       bit for bit.

L, recounted from the kernels:

  gap_partial + gap_finish    S = clamp(HW // 196, 1, 16) splits, per = ceil(HW / S) pixels each (launch_gap_ws).  A lane group adds its
                              pixels lo + grp, lo + grp + 16, ...: ceil(per / 16) additions; lane 0..15 adds the 16 group sums in order: 15;
                              gap_finish adds the S partials onto 0.f: S; the division: 1.   L = ceil(per / 16) + 15 + S + 1
  fused group sums            the epilogues (conv1_x6.hip, gemm_x6.hip, gemm_h2.hip) add the `group` = 16 or 4 rows of an aligned group in order
  + gap_groups_finish         onto 0.f: at most `group` (the stem adds 8 + 1 across two lanes: fewer); gap_groups_finish adds the HW / group sums
                              of an image in order onto 0.f; the division: 1.           L = group + HW / group + 1
  vit_token_stats             a thread adds tokens grp, grp + 4, ...: ceil(count / 4); (r0 + r1) + (r2 + r3): 2; the division: 1.
                                                                                        L = ceil(count / 4) + 2 + 1
                              (the squared deviations run through the same tree: the same L in the std gate)
  rn_pool_stats<D>            a thread adds its D / 256 elements onto 0.f; the LDS tree has 8 levels (128 .. 1); the division: 1.
                                                                                        L = D / 256 + 8 + 1   (17 and 25)
"""
import numpy as np

U = 2.0 ** -24
GAP_MAX_SPLIT = 16


def gap_split(hw):
    """-> (S, per) of launch_gap_ws: the split depends on the map alone"""
    s = min(max(hw // 196, 1), GAP_MAX_SPLIT)
    return s, -(-hw // s)


def l_gap(hw):
    s, per = gap_split(hw)
    return -(-per // 16) + 15 + s + 1


def l_gap_groups(hw, group):
    assert group in (4, 16) and hw % group == 0, (hw, group)
    return group + hw // group + 1


def l_token_stats(count):
    return -(-count // 4) + 2 + 1


def l_pool_stats(dim):
    assert dim in (2048, 4096), dim
    return dim // 256 + 8 + 1


def l_feature_mean(hw, precision):
    """L of one layer-stack block of a forward: the largest over the forms that can serve a tap of hw pixels under `precision`.
    fp32: gap_partial + gap_finish, always.  bf16x6 / f16x2: that form, or - where the producing launch fuses the mean - the group sums
    of 16 rows (hw % 16 == 0) or of 4 (hw % 4 == 0) finished by gap_groups_finish:
        max(l_gap(hw), 16 + hw / 16 + 1 if hw % 16 == 0, 4 + hw / 4 + 1 if hw % 4 == 0)."""
    forms = [l_gap(hw)]
    if precision != "fp32":
        forms += [l_gap_groups(hw, g) for g in (16, 4) if hw % g == 0]
    return max(forms)


def mean_gate(L, abs_mean):
    """abs_mean: mean_i |x_i| of the output's inputs (fp64)"""
    return L * U * (1.0 + L * U) * np.asarray(abs_mean, dtype=np.float64)


def std_gate(L, sigma, abs_mean):
    sigma, abs_mean = np.asarray(sigma, dtype=np.float64), np.asarray(abs_mean, dtype=np.float64)
    d = L * U * abs_mean
    with np.errstate(divide="ignore", invalid="ignore"):
        positive = (L + 4) * U * sigma + d * d / sigma
    return np.where(sigma > 0, positive, d * (1.0 + (L + 4) * U))


def ratio(got, ref, gate):
    """err / gate per output; 0 where the output is exact, inf where it is not finite or off at a gate of 0"""
    got, ref, gate = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(gate, dtype=np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / gate)
    return np.where(np.isfinite(got), r, np.inf)


def reference(x, axis):
    """fp64 on the fp32 inputs -> (mean, max, population std, mean |x|) over `axis`"""
    x64 = np.asarray(x).astype(np.float64)
    return x64.mean(axis=axis), x64.max(axis=axis), x64.std(axis=axis), np.abs(x64).mean(axis=axis)


def mean_ratio(got, x, axis, L):
    mean, _, _, am = reference(x, axis)
    return ratio(got, mean, mean_gate(L, am))


def std_ratio(got, x, axis, L):
    _, _, sigma, am = reference(x, axis)
    return ratio(got, sigma, std_gate(L, sigma, am))
