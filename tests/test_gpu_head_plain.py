"""-m gpu: the plain head (no BatchNorm; relax_head_train_init_ex with batchnorm 0, through head_train.HeadTrainer(batchnorm=False))
against the restatement of tests/head_plain_ref.py, pinned to the reference's own run by tests/golden/head_plain.npz.

The gates are those of tests/test_gpu_head_train.py and tests/test_gpu_head_train_adam.py: the yardstick is the restatement in
fp64, the bar the error of the same restatement in fp32 on the CPU, per tensor as max |t - t64| / max |t64| floored at 2^-24; the
GPU may be BOUND = 8 times as far off.  Under Adam / AdamW parameters are compared on the elements where the fp64 run's
sqrt(exp_avg_sq) is at least MASK_REL of the tensor's largest, at most MASK_CAP of a tensor off that mask (a condition on the
inputs, which tests/test_head_plain_cpu.py holds without a GPU); an element off the mask may differ by 2 lr + lr wd |w|.  Unlike
the BatchNorm head, fc1.bias has a real gradient here and is gated like every other tensor.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gpu_common
import head_plain_ref as P
from relax_vqa_amd import head_train

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_plain.npz")
BOUND = 8.0
FLOOR = 2.0 ** -24
MASK_CAP = 0.01
KINDS = ("sgd", "adam", "adamw")
SGD, ADAM = P.SGD_CFG, P.ADAM_CFG


def _err(t, ref):
    t, ref = np.asarray(t, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.isfinite(t).all()
    return float(np.abs(t - ref).max() / (np.abs(ref).max() + 1e-300))


def grade(name, got, cpu32, ref64, yard=None):
    e, e32 = _err(got, ref64 if yard is None else yard), max(_err(cpu32, ref64), FLOOR)
    ratio = e / e32
    print(f"parity {name}: gpu {e:.3e} cpu-fp32 {e32:.3e} ratio {ratio:.2f}")
    assert ratio <= BOUND, f"{name}: GPU error {e:.3e} is {ratio:.1f} x the CPU fp32 error {e32:.3e}"


def _golden():
    g = np.load(GOLD)
    return g, {k[5:]: g[k] for k in g.files if k.startswith("init/")}, {k[6:]: g[k] for k in g.files if k.startswith("final/")}


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu_common.engine().device, dtype)


def _xp(x):
    F = x.shape[1]
    return gpu_common.engine().head_train_transform(_dev(x), np.ones(F), np.zeros(F))


def _trainer(F=200, hidden=128, max_batch=64):
    return head_train.HeadTrainer(gpu_common.engine(), F, hidden, max_batch=max_batch, batchnorm=False)


def gpu_step(tr, kind, xp, y, rows, drop_rate=0.0, seed=5, step=0, want_masks=False):
    if kind == "sgd":
        return tr.step(xp, y, rows, SGD["lr"], SGD["mu"], SGD["wd"], SGD["l1_w"], SGD["rank_w"], drop_rate, seed=seed, step=step,
                       want_masks=want_masks)
    return tr.step_adam(xp, y, rows, ADAM["lr"], P.B1, P.B2, P.EPS, ADAM["wd"], kind == "adamw", ADAM["l1_w"], ADAM["rank_w"], drop_rate,
                        seed=seed, step=step, want_masks=want_masks)


def restated(kind, init, x, y, drop_rate=0.0, masks=None):
    c = SGD if kind == "sgd" else ADAM
    return P.restated_step(init, x, y, kind, c["lr"], c["wd"], c["l1_w"], c["rank_w"], drop_rate, masks, momentum=SGD["mu"])


def check_step(tag, kind, tr, ref, sel=None):
    """Every parameter, fc1.bias included, and every optimizer block against the fp64 step."""
    sel = sel or (lambda k, a: np.asarray(a))
    r32, r64 = ref["32"], ref["64"]
    got = tr.export_state()
    assert tuple(got) == P.PARAM_KEYS
    grade(f"{tag}.loss", tr.read_loss(0)[0], r32["loss"], r64["loss"])
    if kind == "sgd":
        mom = tr.export_momentum()
        for k in P.PARAM_KEYS:
            grade(f"{tag}.{k}", sel(k, got[k]), sel(k, r32["state"][k]), sel(k, r64["state"][k]))
            grade(f"{tag}.momentum.{k}", sel(k, mom[k]), sel(k, r32["mom"][k]), sel(k, r64["mom"][k]))
        return
    opt = tr.export_optimizer_state()
    assert opt["step"] == r64["step"] and set(opt["exp_avg"]) == set(opt["exp_avg_sq"]) == set(P.PARAM_KEYS)
    c = ADAM
    for k in P.PARAM_KEYS:
        for mom in ("exp_avg", "exp_avg_sq"):
            grade(f"{tag}.{mom}.{k}", sel(k, opt[mom][k]), sel(k, r32[mom][k]), sel(k, r64[mom][k]))
        g, c32, w64 = (sel(k, a).astype(np.float64) for a in (got[k], r32["state"][k], r64["state"][k]))
        mask = P.conditioned(sel(k, r64["exp_avg_sq"][k]))
        off = 1.0 - mask.mean()
        print(f"parity {tag}.{k}: {100 * off:.3f} % of the elements are off the well-conditioned mask")
        assert off <= MASK_CAP, f"{tag}.{k}: {100 * off:.2f} % of the tensor is ill-conditioned"
        grade(f"{tag}.{k}", g[mask], c32[mask], w64[mask])
        if (~mask).any():
            d = np.abs(g - w64)[~mask]
            assert (d <= 2 * c["lr"] + c["lr"] * c["wd"] * np.abs(w64[~mask])).all(), f"{tag}.{k}: off the mask by {d.max():.3e}"


# ---- steps and gates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("drop_rate", [0.0, 0.1])
def test_one_step_from_the_golden_state(drop_rate, kind):
    g, init, _ = _golden()
    b = g["batches"][0]
    tr = _trainer()
    tr.import_state(init)
    m1, m2 = gpu_step(tr, kind, _xp(g["x"]), _dev(g["y"]), b, drop_rate, want_masks=True)
    masks = (m1.cpu().numpy(), m2.cpu().numpy())
    if drop_rate == 0:
        assert masks[0].all() and masks[1].all()
    else:
        assert not masks[0].all() and set(np.unique(masks[0])) <= {0, 1}
    check_step(f"step[{kind},drop={drop_rate}]", kind, tr, restated(kind, init, g["x"][b], g["y"][b], drop_rate, masks))
    assert tr.pad_abs_sum_adam() == (0.0, 0.0, 0.0)           # F = 200 is padded to 224


def test_golden_trajectory():
    """The six recorded steps of the reference's own plain Mlp: per-step loss, the final state and the momentum buffers against the
    recorded fp32 values; the bar is the fp32 restatement's distance from the fp64 restatement of the same six steps."""
    g, init, final = _golden()
    l1_w, rank_w, lr, mu, wd = (float(v) for v in g["config"])
    tr = _trainer()
    tr.import_state(init)
    xp, y = _xp(g["x"]), _dev(g["y"])
    m64 = P.make_model(init, 0.0, torch.float64)
    o64 = P.make_sgd(m64, lr, mu, wd)
    for s, b in enumerate(g["batches"]):
        tr.step(xp, y, b, lr, mu, wd, l1_w, rank_w, 0.0, seed=0, step=s)
        loss64, _, _ = P.train_step(m64, o64, g["x"][b], g["y"][b], l1_w, rank_w)
        grade(f"trajectory.loss[{s}]", tr.read_loss(0)[0], g["losses"][s], loss64, yard=g["losses"][s])
    got, mom, s64, m64m = tr.export_state(), tr.export_momentum(), P.state_of(m64), P.momentum_of(m64, o64)
    for k in P.PARAM_KEYS:
        grade(f"trajectory.{k}", got[k], final[k], s64[k], yard=final[k])
        grade(f"trajectory.momentum.{k}", mom[k], g["momentum/" + k], m64m[k], yard=g["momentum/" + k])
    assert tr.pad_abs_sum() == (0.0, 0.0)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("B", P.SMALL_BATCHES)
def test_one_step_at_the_batch_edges(B, kind):
    """B = 2 (the minimum), 37 (odd: a ragged tail of the column sums) and 64 = max_batch, hidden 128, F = 200."""
    init, x, y, rows = P.small_case(B)
    tr = _trainer(max_batch=64)
    tr.import_state(init)
    gpu_step(tr, kind, _xp(x), _dev(y), rows)
    check_step(f"B={B}[{kind}]", kind, tr, restated(kind, init, x[rows], y[rows]))


_FULL = {}


def _full_case():
    if not _FULL:
        init, x, y, rows = P.full_width_case()
        _FULL.update(init=init, x=x, y=y, rows=rows, xp=_xp(x), yd=_dev(y))
    return _FULL


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_one_step_at_full_width(kind):
    c = _full_case()
    F = c["x"].shape[1]
    tr = _trainer(F, 256, 256)
    tr.import_state(c["init"])
    gpu_step(tr, kind, c["xp"], c["yd"], c["rows"])
    cols = np.random.RandomState(2).choice(F, 64, replace=False)
    sel = lambda k, a: np.asarray(a)[:, cols] if k == "fc1.weight" else np.asarray(a)
    check_step(f"full[{kind}]", kind, tr, restated(kind, c["init"], c["x"][c["rows"]], c["y"][c["rows"]]), sel=sel)
    assert (F + 31) // 32 * 32 - F == 29 and tr.pad_abs_sum_adam() == (0.0, 0.0, 0.0)


# ---- variant and state ----------------------------------------------------------------------------------------------------
def test_masks_equal_the_batchnorm_trainers():
    g, init, _ = _golden()
    xp, y, b = _xp(g["x"]), _dev(g["y"]), g["batches"][1]
    eng = gpu_common.engine()
    tr = _trainer()
    tr.import_state(init)
    p1, p2 = (m.cpu().numpy() for m in tr.step(xp, y, b, 1e-3, drop_rate=0.1, seed=7, step=3, want_masks=True))
    bn = head_train.HeadTrainer(eng, 200, 128, max_batch=64)
    assert bn.arch() is True
    bn.import_state(head_train.init_state_dict(200, 128, seed=1))
    q1, q2 = (m.cpu().numpy() for m in bn.step(xp, y, b, 1e-3, drop_rate=0.1, seed=7, step=3, want_masks=True))
    assert np.array_equal(p1, q1) and np.array_equal(p2, q2) and not p1.all()


def _run32(kind, read_each):
    g, init, _ = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    torch.cuda.synchronize()
    tr = _trainer()
    tr.import_state(init)
    stream = torch.cuda.Stream()
    idx = [tr._idx(g["batches"][s % 6], 48) for s in range(32)]
    with torch.cuda.stream(stream):
        for s in range(32):
            gpu_step(tr, kind if kind == "sgd" else ("adamw" if s % 2 else "adam"), xp, y, idx[s], 0.1, seed=9, step=s)
            if read_each:
                tr.read_loss(0, reset=False)
        out = (tr.export_state(), tr.export_momentum() if kind == "sgd" else tr.export_optimizer_state(), tr.read_loss(0))
    stream.synchronize()
    return out


def _same(a, b):
    if isinstance(a, dict):
        assert set(a) == set(b)
        for k in a:
            _same(a[k], b[k])
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_steps_back_to_back_equal_steps_with_a_read_each_and_a_second_run(kind):
    a, b, c = _run32(kind, False), _run32(kind, True), _run32(kind, False)
    assert a[2] == b[2] == c[2] and a[2][2] == 32
    for x, z in ((a, b), (a, c)):
        _same(x[0], z[0])
        _same(x[1], z[1])


def _raw_init(eng, F, hidden, mb, batchnorm):
    rc = (eng.lib.relax_head_train_init(eng.h, F, hidden, mb) if batchnorm is None
          else eng.lib.relax_head_train_init_ex(eng.h, F, hidden, mb, batchnorm))
    tr = object.__new__(head_train.HeadTrainer)           # the Python half around a state made by a raw call
    tr.eng, tr.lib, tr.h, tr.F, tr.H1, tr.H2, tr.max_batch, tr.Fpad = eng, eng.lib, eng.h, F, hidden, hidden // 2, mb, (F + 31) // 32 * 32
    tr.batchnorm, tr.keys = True, head_train.STATE_KEYS
    eng._head_train_generation = tr.generation = getattr(eng, "_head_train_generation", 0) + 1
    return rc, tr


def test_init_ex_with_batchnorm_equals_init_and_other_values_are_refused():
    g, _, _ = _golden()
    eng = gpu_common.engine()
    xp, y = _xp(g["x"]), _dev(g["y"])
    init = head_train.init_state_dict(200, 128, seed=2)
    runs = []
    for flag in (None, 1):
        rc, tr = _raw_init(eng, 200, 128, 64, flag)
        assert rc == 0 and tr.arch() is True
        tr.import_state(init)
        for s in range(3):
            tr.step(xp, y, g["batches"][s], 0.05, drop_rate=0.1, seed=4, step=s)
        pred = tr.evaluate(xp, y, np.arange(48)).cpu().numpy()
        runs.append((tr.export_state(), tr.export_momentum(), pred, tr.read_loss(0), tr.read_loss(1)))
    _same(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2]) and runs[0][3:] == runs[1][3:]
    assert int(runs[1][0]["bn1.num_batches_tracked"]) == 3
    rc = eng.lib.relax_head_train_init_ex(eng.h, 200, 128, 64, 2)
    assert rc != 0 and "2" in eng.lib.relax_last_error(eng.h).decode() and "batchnorm" in eng.lib.relax_last_error(eng.h).decode()
    plain = _trainer()
    assert plain.arch() is False and plain.lib.relax_head_train_export_numel(plain.h) == 128 * 200 + 128 + 64 * 128 + 64 + 64 + 1


def test_arch_without_a_state_is_refused():
    from relax_vqa_amd.engine import RelaxEngine
    eng = RelaxEngine(0)
    out = C.c_int(-1)
    assert eng.lib.relax_head_train_arch(eng.h, C.byref(out)) != 0 and eng.lib.relax_last_error(eng.h).decode()


# ---- state transfer and loading -------------------------------------------------------------------------------------------
def test_export_import_round_trip_and_a_resumed_adam_run():
    g, init, _ = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    tr = _trainer()
    tr.import_state(init)
    back = tr.export_state()
    assert tuple(back) == P.PARAM_KEYS
    _same({k: init[k].reshape(back[k].shape) for k in back}, back)
    for s in range(3):
        gpu_step(tr, "adamw", xp, y, g["batches"][s], 0.1, seed=7, step=s)
    state, opt_state = tr.export_state(), tr.export_optimizer_state()
    assert opt_state["step"] == 3 and set(opt_state["exp_avg"]) == set(P.PARAM_KEYS)
    gpu_step(tr, "adamw", xp, y, g["batches"][3], 0.1, seed=7, step=3)
    want, want_opt = tr.export_state(), tr.export_optimizer_state()
    tr2 = _trainer()
    tr2.import_state(state)
    tr2.import_optimizer_state(opt_state)
    _same(tr2.export_optimizer_state(), opt_state)
    gpu_step(tr2, "adamw", xp, y, g["batches"][3], 0.1, seed=7, step=3)
    _same(tr2.export_state(), want)
    _same(tr2.export_optimizer_state(), want_opt)
    # bn1 keys into a plain state: refused by name, nothing written
    with pytest.raises(RuntimeError, match="bn1.weight"):
        tr2.import_state(dict(state, **{"bn1.weight": np.ones(128, np.float32)}))
    bad = {m: dict(opt_state[m], **{"bn1.bias": np.zeros(128, np.float32)}) for m in ("exp_avg", "exp_avg_sq")}
    with pytest.raises(RuntimeError, match="bn1.bias"):
        tr2.import_optimizer_state(dict(bad, step=4))
    _same(tr2.export_state(), want)
    _same(tr2.export_optimizer_state(), want_opt)
    assert tr2.pad_abs_sum_adam() == (0.0, 0.0, 0.0)


def test_swa_update_bn_pass_and_the_padding():
    g, init, _ = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    tr = _trainer()
    tr.import_state(init)
    tr.copy(head_train.SWA, head_train.LIVE)
    avg = None
    for s, b in enumerate(g["batches"][:3]):
        gpu_step(tr, "sgd", xp, y, b, step=s)
        tr.swa_update()
        live = tr.export_state()
        # AveragedModel.update_parameters in fp32 on the host: the first call copies, then avg += (p - avg) / (n + 1)
        avg = ({k: v.copy() for k, v in live.items()} if avg is None
               else {k: (avg[k] + (live[k] - avg[k]) / np.float32(s + 1)).astype(np.float32) for k in avg})
    got = tr.export_state(head_train.SWA)
    assert int(got.pop("n_averaged")) == 3 and "bn1.num_batches_tracked" not in got
    for k in P.PARAM_KEYS:
        assert np.abs(got[k].astype(np.float64) - avg[k]).max() <= 2.0 ** -22 * np.abs(avg[k]).max(), k   # the division may round the other way
    before = [tr.export_state(w) for w in (head_train.LIVE, head_train.SWA, head_train.BEST)]
    tr.bn_pass(None, None, head_train.SWA, reset=True)
    tr.bn_pass(xp, g["batches"][0], head_train.SWA)
    tr.update_bn(xp, [g["batches"][1]], head_train.LIVE)
    for w, b4 in zip((head_train.LIVE, head_train.SWA, head_train.BEST), before):
        _same(tr.export_state(w), b4)
    with pytest.raises(RuntimeError):
        tr.bn_pass(xp, np.arange(1), head_train.SWA)          # validated as on a BatchNorm state: a batch of one row
    assert tr.pad_abs_sum() == (0.0, 0.0)


def test_loading_and_scoring_a_plain_dict():
    """relax_load_mlp_head + relax_mlp_head and relax_head_train_eval on a plain state dict against the fp64 forward, within the
    tolerance tests/test_gpu_head.py holds the BatchNorm head to (rtol 1e-4, atol 1e-3)."""
    g, init, final = _golden()
    eng = gpu_common.engine()
    rng = np.random.RandomState(3)
    scale, mn, stats = rng.uniform(0.5, 2.0, 200), rng.uniform(-1, 1, 200), rng.uniform(0, 1, 200)
    feats = g["x"].copy()
    feats[7, 100:120] = np.nan
    filled = np.where(np.isnan(feats), stats[None, :], feats.astype(np.float64))
    xs = (filled * scale + mn).astype(np.float32)
    want = P.eval_forward(P.make_model(final, 0.0, torch.float64), xs)
    eng.load_mlp_head({("module." + k): v for k, v in final.items()}, scale, mn, stats)
    got = eng.mlp_head(_dev(feats)).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-3)
    tr = _trainer()
    tr.import_state(final)
    pred = tr.evaluate(_dev(np.pad(xs, ((0, 0), (0, 24)))), None, np.arange(48)).cpu().numpy()
    np.testing.assert_allclose(pred, want, rtol=1e-4, atol=1e-3)
    with pytest.raises(RuntimeError, match="bn1"):             # some but not all bn1 keys: still refused
        eng.load_mlp_head(dict(final, **{"bn1.weight": np.ones(128, np.float32)}), scale, mn, stats)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _synthetic_set(n=240, F=512):
    rng = np.random.RandomState(0)
    x = rng.uniform(0, 10, size=(n, F)).astype(np.float32)
    mos = (3 + np.sin(x[:, 0] * 0.5) + 0.1 * x[:, 1] - 0.02 * x[:, 2] ** 2 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return x, mos


def test_fit_head_simple_round_trip_and_fine_tune():
    from relax_vqa_amd import metrics
    x, mos = _synthetic_set()
    eng = gpu_common.engine()
    feats = _dev(x)
    result = eng.fit_head_simple(feats, mos, dict(epochs=6, hidden_features=128, batch_size=64, seed=3))
    sd, scaler, hist = result
    assert tuple(sd) == P.PARAM_KEYS and sd["fc1.weight"].shape == (128, 512) and hist["best"] is not None
    train, val = metrics.holdout_split(240, 0.2, 42)
    assert len(hist["folds"]) == 1 and np.array_equal(hist["folds"][0][0], train) and np.array_equal(hist["folds"][0][1], val)
    assert len(val) == 48 and len(hist["train_loss"]) == 1 and len(hist["train_loss"][0]) <= 6
    eng.load_fitted_head(result)
    scores = eng.mlp_head(feats)
    assert torch.isfinite(scores).all() and hist["predictions"].shape == (240,)
    gpu_common.assert_close(scores, hist["predictions"], "mlp_head on the plain fitted head vs the training path's eval")
    tuned = eng.fine_tune_head(sd, feats, mos, dict(epochs=4, batch_size=64, initial_lr=1e-2))
    assert "n_averaged" in tuned[0] and set(tuned[0]) - {"n_averaged"} == set(P.PARAM_KEYS) and np.isfinite(tuned[0]["fc1.weight"]).all()
    eng.load_fitted_head(tuned)
    gpu_common.assert_close(eng.mlp_head(feats), tuned[2]["predictions"], "mlp_head on the fine-tuned plain head vs the training path's eval")


def test_holdout_protocol_with_the_simple_config():
    x, mos = _synthetic_set()
    cfg = dict(head_train.SIMPLE_DEFAULTS, epochs=6, hidden_features=128, batch_size=64)
    res = gpu_common.engine().holdout_protocol(_dev(x), mos, cfg, n_repeats=3)
    assert len(res["repeats"]) == 3 and tuple(res["repeats"][0]["state_dict"]) == P.PARAM_KEYS
    for key, (median, std) in res["summary"].items():
        assert np.isfinite(median) and np.isfinite(std), key
