"""-m gpu: the kernels that turn activations into the numbers a user receives, at fp32 rounding: spatial means (gap_partial + gap_finish,
the fused group sums + gap_groups_finish), token statistics (vit_token_stats) and the pool vectors' tail (rn_pool_stats<2048|4096>).

Reference: numpy fp64 on the same fp32 inputs.  Gates: tests/reduction_bounds.py - derived from the number of fp32 roundings on the longest
path into an output, not from what a kernel returns; max and copied elements bit for bit.  Cases and inputs: tests/reduction_cases.py, the
list tests/test_reduction_bounds_cpu.py replays on the CPU (correct replays inside the gates, five wrong ones at least 8 x outside).

The operator tests drive op_gap, op_token_stats and op_pool_stats.  The feature tests need no reference network: a layer-stack block must
be the spatial mean of the tap the SAME call exported, and the tail of a pool vector the statistics of the vector in front of it, under
every arithmetic.  L of a block: reduction_bounds.l_feature_mean, the largest over the forms that can serve the tap -
    max(ceil(per / 16) + 15 + S + 1,  16 + HW / 16 + 1 if HW % 16 == 0,  4 + HW / 4 + 1 if HW % 4 == 0)      (fp32: the first alone).

The largest err / gate seen per kernel and case goes to the file RELAX_REDUCTION_PARITY_OUT names (profiles/reduction_parity.json).
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fragment_ref, pooling_ref
from relax_vqa_amd import engine as engine_module
from tests import reduction_bounds as RB
from tests import reduction_cases as RC
from tests.gpu_common import engine, rn50_weights, synth

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
SEEN = {}
_state = {}


def _see(kernel, case, what, ratios):
    worst = float(np.max(ratios))
    print(f"{kernel} {case}: {what} err / gate {worst:.3g}")
    seen = SEEN.setdefault(kernel, {}).setdefault(case, {})
    seen[what] = max(seen.get(what, 0.0), worst)
    return worst


@pytest.fixture(scope="module", autouse=True)
def _record_parity():
    yield
    out = os.environ.get("RELAX_REDUCTION_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "largest err / gate per kernel and case: the reductions on the device against numpy fp64 on the same fp32 inputs "
                               "(tests/test_gpu_reductions.py; gates and L: tests/reduction_bounds.py; max and copies are compared bit for bit)",
                       "gate": 1.0, "seen": SEEN}, f, indent=1, sort_keys=True)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the operators ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,c", RC.GAP_CASES)
def test_op_gap(hw, c):
    x, kinds = RC.gap_input(hw, c)
    out = torch.full((RC.N_IMG, c + 5), SENTINEL, dtype=torch.float32, device="cuda")       # out_stride > C
    engine().op_gap(_cu(x), out=out)
    got = out.cpu().numpy()
    assert (got[:, c:] == np.float32(SENTINEL)).all(), "written past the C means of a row"
    worst = _see("op_gap", f"hw={hw},c={c}", "mean", RB.mean_ratio(got[:, :c], x, 1, RB.l_gap(hw)))
    assert worst <= 1.0, f"HW={hw} C={c}: mean err / gate {worst:.3g}"
    assert (got[:, kinds.index("constant")] == np.float32(RC.CONSTANT)).all()


@pytest.mark.parametrize("count,dim", RC.TOKEN_CASES)
def test_op_token_stats(count, dim):
    x, kinds = RC.token_input(count, dim)
    got = engine().op_token_stats(_cu(x)).cpu().numpy()
    mean, mx, std = got[:, :dim], got[:, dim:2 * dim], got[:, 2 * dim:]
    L = RB.l_token_stats(count)
    case = f"count={count},dim={dim}"
    w_mean = _see("op_token_stats", case, "mean", RB.mean_ratio(mean, x, 1, L))
    w_std = _see("op_token_stats", case, "std", RB.std_ratio(std, x, 1, L))
    assert np.array_equal(mx, x.max(axis=1)), "max is not bit-exact"
    assert w_mean <= 1.0 and w_std <= 1.0, f"{case}: mean err / gate {w_mean:.3g}, std err / gate {w_std:.3g}"
    k = kinds.index("constant")
    assert (mean[:, k] == np.float32(RC.CONSTANT)).all() and (std[:, k] == 0).all()
    assert (mx[:, kinds.index("negative")] < 0).all()
    if count == 1:
        assert (std == 0).all() and np.array_equal(mean.view(np.int32), mx.view(np.int32))


@pytest.mark.parametrize("dim,n", RC.POOL_CASES)
def test_op_pool_stats(dim, n):
    v, kinds = RC.pool_input(dim, n)
    vp = np.full((n, dim + 7), 1e30, dtype=np.float32)          # v_stride > dim: a read past a row's dim elements shows in every statistic
    vp[:, :dim] = v
    out = torch.full((n, dim + 3 + 5), SENTINEL, dtype=torch.float32, device="cuda")     # out_stride > dim + 3
    engine().op_pool_stats(_cu(vp), dim, out=out)
    got = out.cpu().numpy()
    assert (got[:, dim + 3:] == np.float32(SENTINEL)).all(), "written past the dim + 3 outputs of a row"
    assert np.array_equal(got[:, :dim].view(np.int32), v.view(np.int32)), "out[:dim] is not the vector"
    L = RB.l_pool_stats(dim)
    case = f"dim={dim},n={n}"
    w_mean = _see("op_pool_stats", case, "mean", RB.mean_ratio(got[:, dim], v, 1, L))
    w_std = _see("op_pool_stats", case, "std", RB.std_ratio(got[:, dim + 2], v, 1, L))
    assert np.array_equal(got[:, dim + 1], v.max(axis=1)), "max is not bit-exact"
    assert w_mean <= 1.0 and w_std <= 1.0, f"{case}: mean err / gate {w_mean:.3g}, std err / gate {w_std:.3g}"
    if "constant" in kinds:
        k = kinds.index("constant")
        assert got[k, dim] == got[k, dim + 1] == np.float32(RC.CONSTANT) and got[k, dim + 2] == 0
        assert got[kinds.index("negative"), dim + 1] < 0


def test_op_pool_stats_refuses_other_widths_by_name():
    eng = engine()
    v = torch.zeros((2, 4096), dtype=torch.float32, device="cuda")
    for dim in (1024, 2049, 4095):
        with pytest.raises(RuntimeError, match=f"dim {dim} is neither 2048 nor 4096"):
            eng.op_pool_stats(v, dim)
    with pytest.raises(ValueError, match="op_pool_stats"):
        eng.op_pool_stats(v[:, :2047].contiguous(), 2048)


# ---- features as functions of the engine's own exported taps ---------------------------------------------------------------------------------
def _fragments(n):
    frs = []
    for i in range(n):
        o, nx = synth.synthetic_pair(240, 320, 900 + i)
        f = fragment_ref.fragment_pair(o, nx)
        frs.append(f["ori_frag"] if i % 2 == 0 else f["diff_frag"])
    return np.stack(frs)


def _layer_stack_is_the_mean_of_the_taps(net, ls, taps, channels, precision):
    off, worst = 0, {}
    for t, c in enumerate(channels):
        a = taps[t].cpu().numpy()
        n, ch, h, w = a.shape
        assert ch == c
        L = RB.l_feature_mean(h * w, precision)
        worst[t] = _see(net, f"{precision},block {t} ({h}x{w}x{c})", "mean", RB.mean_ratio(ls[:, off:off + c], a.reshape(n, c, h * w), 2, L))
        off += c
    assert off == ls.shape[1]
    bad = {t: f"{r:.3g}" for t, r in worst.items() if r > 1.0}
    assert not bad, f"{net} {precision}: layer-stack blocks that are not the mean of their exported tap (block: err / gate) {bad}"


def _pool_tail_is_the_statistics_of_the_vector(net, pool, dim, precision):
    v = np.ascontiguousarray(pool[:, :dim])
    L = RB.l_pool_stats(dim)
    w_mean = _see(net, f"{precision},pool tail", "mean", RB.mean_ratio(pool[:, dim], v, 1, L))
    w_std = _see(net, f"{precision},pool tail", "std", RB.std_ratio(pool[:, dim + 2], v, 1, L))
    assert np.array_equal(pool[:, dim + 1], v.max(axis=1)), f"{net}: the pool vector's max is not bit-exact"
    assert w_mean <= 1.0 and w_std <= 1.0, f"{net} {precision}: pool tail mean err / gate {w_mean:.3g}, std err / gate {w_std:.3g}"


def test_resnet50_features_are_the_statistics_of_the_exported_taps(each_precision):
    rn50_weights()
    ls, pool, taps = engine().resnet50_features(_cu(_fragments(3)), taps=range(15))
    ls, pool = ls.cpu().numpy(), pool.cpu().numpy()
    _pool_tail_is_the_statistics_of_the_vector("resnet50_224", pool, 2048, each_precision)
    _layer_stack_is_the_mean_of_the_taps("resnet50_224", ls, taps, pooling_ref.RESNET50_TAP_CHANNELS, each_precision)


def _smallest_odd_canvas(eng):
    """the smallest square canvas of the any-size rule on which the map of every stage is odd (65: 33, 17, 9, 5, 3)"""
    if "odd" not in _state:
        for side in range(64, 1025):
            shapes = eng.resnet50_canvas_geometry(side, side, any_size=True)[0]
            if all(h % 2 == 1 and w % 2 == 1 for h, w in shapes):
                _state["odd"] = side
                break
    return _state["odd"]


def test_resnet50_features_on_an_odd_canvas_are_the_statistics_of_the_exported_taps(each_precision):
    rn50_weights()
    eng = engine()
    side = _smallest_odd_canvas(eng)
    assert side == 65
    imgs = np.stack([synth.synthetic_pair(240, 320, 930 + i)[i % 2][40 * i:40 * i + side, 60 * i:60 * i + side] for i in range(3)])
    ls, pool, taps = eng.resnet50_features_canvas(_cu(imgs), taps=range(15), any_size=True)
    ls, pool = ls.cpu().numpy(), pool.cpu().numpy()
    assert [tuple(taps[t].shape[2:]) for t in (0, 1, 4, 8, 12)] == [(33, 33), (17, 17), (9, 9), (5, 5), (3, 3)]
    _pool_tail_is_the_statistics_of_the_vector("resnet50_65", pool, 2048, each_precision)
    _layer_stack_is_the_mean_of_the_taps("resnet50_65", ls, taps, pooling_ref.RESNET50_TAP_CHANNELS, each_precision)


def test_vgg16_features_are_the_statistics_of_the_exported_taps(each_precision):
    eng = engine()
    if _state.get("vgg16") is not eng:
        eng.load_vgg16(synth.vgg16_state_dict())
        _state["vgg16"] = eng
    ls, pool, taps = eng.vgg16_features(_cu(_fragments(2)), taps=range(13))
    ls, pool = ls.cpu().numpy(), pool.cpu().numpy()
    _pool_tail_is_the_statistics_of_the_vector("vgg16", pool, 4096, each_precision)
    _layer_stack_is_the_mean_of_the_taps("vgg16", ls, taps, [c for c, _ in engine_module.VGG16_TAP_SHAPES], each_precision)
