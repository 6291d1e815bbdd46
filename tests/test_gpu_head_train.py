"""-m gpu: the head's training path (csrc/head_train.hip through RelaxEngine / head_train.py) against the restatement of
tests/head_train_ref.py.

Yardstick of every float comparison: the restatement in fp64.  Bar: the error the restatement in fp32 ON THE CPU has against
that fp64 run, per tensor, as max |t - t64| / max |t64| (floored at 2^-24, the rounding of the fp64 value to fp32 itself: a
CPU result that happens to be exact does not demand an exact GPU one).  The GPU may be BOUND times as far off as the CPU's
fp32 is.  BOUND = twice the largest ratio observed on the first GPU run, within [2, 8]; the observed ratios are in
profiles/head_train_parity.json and below.

Ratios observed on the GPU (largest eight of 84 compared tensors; profiles/head_train_parity.json is the file this module
writes when RELAX_HEAD_TRAIN_PARITY_OUT names one, unedited):
  full.bn1.bias: 5.73
  full.fc2.bias: 4.40
  trajectory.loss[0]: 3.16
  full.fc2.weight: 3.10
  step[drop=0.0].loss: 2.18
  full.bn1.running_var: 1.99
  trajectory.bn1.running_mean: 1.66
  full.bn1.weight: 1.64
Largest 5.73 (bn1.bias after one full-width step: a 256-row sum in another order than the CPU's, against a CPU error at the
2^-24 floor), the same on every run so far.  BOUND = min(8, 2 x 5.73) = 8.
fc1.bias and its momentum buffer have a zero true gradient, so a ratio of roundings says nothing about them: they are held to the
absolute bound of check 9 (lr * 2^-20 * max|dz1| * B for one step), propagated through the momentum recursion for several steps
(_b1_bounds).
"""
import json
import os

import numpy as np
import pytest
import torch

import gpu_common
import head_train_ref as R
from relax_vqa_amd import head_train, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_train.npz")
BOUND = 8.0
FLOOR = 2.0 ** -24
RATIOS = {}
TENSORS = R.PARAM_KEYS + R.BUFFER_KEYS


@pytest.fixture(scope="module", autouse=True)
def _record_ratios():
    yield
    out = os.environ.get("RELAX_HEAD_TRAIN_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"metric": "(max|gpu - yardstick| / max|yardstick|) / max(max|cpu fp32 - fp64| / max|fp64|, 2^-24) per compared tensor",
                       "largest_ratio": max(RATIOS.values()) if RATIOS else None, "bound": BOUND, "ratios": RATIOS}, f, indent=1, sort_keys=True)


def _err(t, ref):
    t, ref = np.asarray(t, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.isfinite(t).all()
    return float(np.abs(t - ref).max() / (np.abs(ref).max() + 1e-300))


def grade(name, got, cpu32, ref64, yard=None):
    """yard: what `got` is measured against (default the fp64 run); the bar is always the fp32 run's distance from the fp64 one"""
    e, e32 = _err(got, ref64 if yard is None else yard), max(_err(cpu32, ref64), FLOOR)
    ratio = e / e32
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"parity {name}: gpu {e:.3e} cpu-fp32 {e32:.3e} ratio {ratio:.2f}")
    assert ratio <= BOUND, f"{name}: GPU error {e:.3e} is {ratio:.1f} x the CPU fp32 error {e32:.3e}"


def _golden():
    g = np.load(GOLD)
    init = {k[5:]: g[k] for k in g.files if k.startswith("init/")}
    final = {k[6:]: g[k] for k in g.files if k.startswith("final/")}
    return g, init, final


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu_common.engine().device, dtype)


def _xp(x):
    F = x.shape[1]
    return gpu_common.engine().head_train_transform(_dev(x), np.ones(F), np.zeros(F))


# ---- 7. scaler fit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(48, 200), (1200, 19779), (37, 35203)])
def test_scaler_fit(n, F):
    rng = np.random.RandomState(n)
    x = (rng.standard_normal((n, F)) * rng.uniform(0.1, 30, F) + rng.uniform(-5, 5, F)).astype(np.float32)
    x[rng.randint(n, size=40), rng.randint(F, size=40)] = np.nan
    x[rng.randint(n, size=20), rng.randint(F, size=20)] = np.inf
    x[rng.randint(n, size=20), rng.randint(F, size=20)] = -np.inf
    x[:, 3] = np.nan                       # an all-NaN column
    x[:, 5] = 2.5                          # a constant column
    x[:, 7] = 1.0
    x[n // 2, 7] = np.nextafter(np.float32(1.0), np.float32(2.0))   # a range of one ulp
    eng = gpu_common.engine()
    got = eng.fit_scaler(_dev(x), want_range=True)
    want = R.fit_scaler(x)
    for k in ("data_min", "data_max", "scale", "min"):
        assert np.array_equal(got[k], want[k]), k           # min and max do not round: bit-exact
    assert got["scale"][3] == 1.0 and got["scale"][5] == 1.0 and got["min"][5] == -2.5 and got["scale"][7] == 2.0 ** 23
    zeroed = np.where(np.isfinite(x), x, 0).astype(np.float64)
    bound = n * 2.0 ** -52 * np.abs(zeroed).mean(axis=0)   # a float64 sum of n terms, in any order
    assert (np.abs(got["imputer_statistics"] - want["imputer_statistics"]) <= bound).all()
    xp = eng.head_train_transform(_dev(x), got["scale"], got["min"]).cpu().numpy()
    assert xp.shape == (n, (F + 31) // 32 * 32)
    assert np.array_equal(xp[:, :F], R.train_transform(x, want["scale"], want["min"])) and not xp[:, F:].any()


# ---- 8. criterion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 16, 255, 256])
def test_criterion(B):
    tr = head_train.HeadTrainer(gpu_common.engine(), 64, 128, max_batch=256)
    rng = np.random.RandomState(B)
    y = np.round(1 + 4 * rng.uniform(size=B), 1).astype(np.float32)       # one decimal: ties once B is large
    p = (y + rng.standard_normal(B) * 0.7).astype(np.float32)
    if B >= 16:
        y[1] = y[0]                                                        # a tie for certain
        p[2::5] = y[2::5]                                                  # predictions equal to their target
    loss, grad = tr.criterion(_dev(p), _dev(y), 0.6, 1.0)
    outs = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        pt = torch.tensor(p, dtype=dt, requires_grad=True)
        L = R.mae_rank_loss(pt, torch.tensor(y, dtype=dt), 0.6, 1.0)
        L.backward()
        outs[name] = (float(L.detach()), pt.grad.numpy())
    grade(f"criterion.loss[B={B}]", loss.cpu().numpy(), outs["32"][0], outs["64"][0])
    grade(f"criterion.grad[B={B}]", grad.cpu().numpy(), outs["32"][1], outs["64"][1])


def test_criterion_zero_gradients_are_exact():
    tr = head_train.HeadTrainer(gpu_common.engine(), 64, 128, max_batch=256)
    # a tied pair: sign 0, relu(0) = 0, no gradient from the rank term whatever the predictions are
    _, grad = tr.criterion(_dev(np.float32([0.3, 1.9])), _dev(np.float32([2.0, 2.0])), 0.0, 1.0)
    assert (grad.cpu().numpy() == 0).all()
    # an exact hit: sign(p - y) = 0, no gradient from the MAE term
    loss, grad = tr.criterion(_dev(np.float32([2.0, 3.5, 1.0])), _dev(np.float32([2.0, 3.0, 1.0])), 1.0, 0.0)
    g = grad.cpu().numpy()
    assert g[0] == 0 and g[2] == 0 and g[1] == np.float32(1.0) / np.float32(3.0)


# ---- 9. one step --------------------------------------------------------------------------------------------------------
def _restated_step(init, x, y, cfg, drop_rate, masks):
    out = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        m = R.make_model(init, drop_rate, dt)
        opt = R.make_sgd(m, cfg["lr"], cfg["mu"], cfg["wd"])
        loss, pred, grads = R.train_step(m, opt, x, y, cfg["l1_w"], cfg["rank_w"], masks)
        out[name] = dict(state=R.state_of(m), mom=R.momentum_of(m, opt), loss=loss, model=m, opt=opt)
    return out


def _dz1_eps(model64, x, y, cfg, masks=None):
    """2^-20 * max|dz1| * B for the step `model64` (fp64) is about to take: fc1.bias has a zero gradient behind the BatchNorm
    (db1 = sum_b dz1 = 0 in exact arithmetic), so what an fp32 implementation adds into it is the rounding of a B-term sum of
    values up to max|dz1| - the bound of the issue, without its lr factor."""
    import copy
    mc = copy.deepcopy(model64)
    mc.train()
    mc.masks = masks
    z = mc.fc1(torch.as_tensor(x, dtype=torch.float64))
    z.retain_grad()
    h = mc._drop(torch.nn.functional.gelu(mc.bn1(z)), 0)
    h = mc._drop(torch.nn.functional.gelu(mc.fc2(h)), 1)
    R.mae_rank_loss(mc.fc3(h).reshape(-1), torch.as_tensor(y, dtype=torch.float64), cfg["l1_w"], cfg["rank_w"]).backward()
    return 2.0 ** -20 * float(z.grad.abs().max()) * len(y)


def _b1_bounds(eps, cfg, b_max, m_max):
    """Worst-case propagation of the per-step gradient errors eps[k] through m = mu m + g, b -= lr m, plus the fp32 roundings
    of the two stored values (2^-22 max|m| and 2^-23 max|b| per step): [(bound on fc1.bias, bound on its momentum)] after each
    step.  After one step from m = 0 the first is lr * eps[0] (+ the rounding of b), the bound check 9 names."""
    out, eb, em = [], 0.0, 0.0
    for e in eps:
        em = cfg["mu"] * em + e + 2.0 ** -22 * m_max
        eb = eb + cfg["lr"] * em + 2.0 ** -23 * b_max
        out.append((eb, em))
    return out


def check_b1(name, got_b, got_m, want_b, want_m, bounds, slack=1.0):
    eb, em = bounds
    db = float(np.abs(np.asarray(got_b, np.float64) - np.asarray(want_b, np.float64)).max())
    print(f"parity {name}: fc1.bias off by {db:.3e} (bound {slack * eb:.3e})")
    assert db <= slack * eb, f"{name}: fc1.bias off by {db:.3e}, bound {slack * eb:.3e}"
    if got_m is not None:
        dm = float(np.abs(np.asarray(got_m, np.float64) - np.asarray(want_m, np.float64)).max())
        print(f"parity {name}: fc1.bias momentum off by {dm:.3e} (bound {slack * em:.3e})")
        assert dm <= slack * em, f"{name}: momentum of fc1.bias off by {dm:.3e}, bound {slack * em:.3e}"


CFG = dict(lr=0.1, mu=0.9, wd=0.005, l1_w=0.6, rank_w=1.0)


@pytest.mark.parametrize("drop_rate", [0.0, 0.1])
def test_one_step_from_the_golden_state(drop_rate):
    g, init, _ = _golden()
    b = g["batches"][0]
    tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
    tr.import_state(init)
    m1, m2 = tr.step(_xp(g["x"]), _dev(g["y"]), b, CFG["lr"], CFG["mu"], CFG["wd"], CFG["l1_w"], CFG["rank_w"], drop_rate, seed=5, step=0,
                     want_masks=True)
    masks = (m1.cpu().numpy(), m2.cpu().numpy())
    if drop_rate == 0:
        assert masks[0].all() and masks[1].all()
    ref = _restated_step(init, g["x"][b], g["y"][b], CFG, drop_rate, masks)
    got, mom = tr.export_state(), tr.export_momentum()
    tag = f"step[drop={drop_rate}]"
    grade(f"{tag}.loss", tr.read_loss(0)[0], ref["32"]["loss"], ref["64"]["loss"])
    for k in TENSORS:
        if k == "fc1.bias":
            continue
        grade(f"{tag}.{k}", got[k], ref["32"]["state"][k], ref["64"]["state"][k])
    for k in R.PARAM_KEYS:
        if k != "fc1.bias":
            grade(f"{tag}.momentum.{k}", mom[k], ref["32"]["mom"][k], ref["64"]["mom"][k])
    eps = _dz1_eps(R.make_model(init, drop_rate, torch.float64), g["x"][b], g["y"][b], CFG, masks)
    s64, m64 = ref["64"]["state"]["fc1.bias"], ref["64"]["mom"]["fc1.bias"]
    check_b1(tag, got["fc1.bias"], mom["fc1.bias"], s64, m64, _b1_bounds([eps], CFG, np.abs(s64).max(), np.abs(m64).max())[0])
    assert int(got["bn1.num_batches_tracked"]) == 1


def test_one_step_at_full_width():
    F, H1, B = 35203, 256, 256
    init = synth.mlp_head_state_dict()
    rng = np.random.RandomState(11)
    x = rng.uniform(0, 1, size=(B + 8, F)).astype(np.float32)
    y = (1 + 4 * rng.uniform(size=B + 8)).astype(np.float32)
    rows = rng.permutation(B + 8)[:B]
    tr = head_train.HeadTrainer(gpu_common.engine(), F, H1, max_batch=256)
    tr.import_state(init)
    tr.step(_xp(x), _dev(y), rows, CFG["lr"], CFG["mu"], CFG["wd"], CFG["l1_w"], CFG["rank_w"], 0.0, seed=1, step=0)
    ref = _restated_step(init, x[rows], y[rows], CFG, 0.0, None)
    got = tr.export_state()
    cols = np.random.RandomState(2).choice(F, 64, replace=False)
    grade("full.loss", tr.read_loss(0)[0], ref["32"]["loss"], ref["64"]["loss"])
    grade("full.fc1.weight[64 columns]", got["fc1.weight"][:, cols], ref["32"]["state"]["fc1.weight"][:, cols],
          ref["64"]["state"]["fc1.weight"][:, cols])
    for k in TENSORS:
        if k not in ("fc1.weight", "fc1.bias"):
            grade(f"full.{k}", got[k], ref["32"]["state"][k], ref["64"]["state"][k])
    eps = _dz1_eps(R.make_model(init, 0.0, torch.float64), x[rows], y[rows], CFG)
    s64, m64 = ref["64"]["state"]["fc1.bias"], ref["64"]["mom"]["fc1.bias"]
    check_b1("full", got["fc1.bias"], tr.export_momentum()["fc1.bias"], s64, m64,
             _b1_bounds([eps], CFG, np.abs(s64).max(), np.abs(m64).max())[0])
    # the 29 padded columns of W1 and of its momentum, read back from the device block itself: exactly 0
    assert (F + 31) // 32 * 32 - F == 29
    assert tr.pad_abs_sum() == (0.0, 0.0)


# ---- 10. the golden trajectory ------------------------------------------------------------------------------------------
def test_golden_trajectory():
    """The six recorded steps: per-step loss and the final state against the REFERENCE's recorded values (fp32, its own
    classes); the bar is the fp32 restatement's distance from the fp64 restatement of the same six steps."""
    g, init, final = _golden()
    l1_w, rank_w, lr, mu, wd = (float(v) for v in g["config"])
    tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
    tr.import_state(init)
    xp, y = _xp(g["x"]), _dev(g["y"])
    m64 = R.make_model(init, 0.0, torch.float64)
    o64 = R.make_sgd(m64, lr, mu, wd)
    cfg = dict(lr=lr, mu=mu, wd=wd, l1_w=l1_w, rank_w=rank_w)
    eps = []
    for s, b in enumerate(g["batches"]):
        tr.step(xp, y, b, lr, mu, wd, l1_w, rank_w, 0.0, seed=0, step=s)
        eps.append(_dz1_eps(m64, g["x"][b], g["y"][b], cfg))
        loss64, _, _ = R.train_step(m64, o64, g["x"][b], g["y"][b], l1_w, rank_w)
        grade(f"trajectory.loss[{s}]", tr.read_loss(0)[0], g["losses"][s], loss64, yard=g["losses"][s])
    got, s64 = tr.export_state(), R.state_of(m64)
    for k in TENSORS:
        if k != "fc1.bias":
            grade(f"trajectory.{k}", got[k], final[k], s64[k], yard=final[k])
    assert int(got["bn1.num_batches_tracked"]) == int(final["bn1.num_batches_tracked"]) == 6
    # fc1.bias and its momentum buffer after six steps (the mu * m path of the update): against the fp64 run within the propagated
    # rounding bound, and against the reference's recorded fp32 values within twice it (each side may use the bound once)
    mom, m64m = tr.export_momentum(), R.momentum_of(m64, o64)
    bounds = _b1_bounds(eps, cfg, np.abs(s64["fc1.bias"]).max(), np.abs(m64m["fc1.bias"]).max())[-1]
    check_b1("trajectory", got["fc1.bias"], mom["fc1.bias"], s64["fc1.bias"], m64m["fc1.bias"], bounds)
    check_b1("trajectory vs recorded", got["fc1.bias"], mom["fc1.bias"], final["fc1.bias"], g["momentum/fc1.bias"], bounds, slack=2.0)
    for k in R.PARAM_KEYS:
        if k != "fc1.bias":
            grade(f"trajectory.momentum.{k}", mom[k], g["momentum/" + k], m64m[k], yard=g["momentum/" + k])
    assert tr.pad_abs_sum() == (0.0, 0.0)                # F = 200 is padded to 224


# ---- 11. dropout --------------------------------------------------------------------------------------------------------
def test_dropout_masks():
    rng = np.random.RandomState(4)
    x = rng.uniform(size=(256, 64)).astype(np.float32)
    y = rng.uniform(1, 5, size=256).astype(np.float32)
    tr = head_train.HeadTrainer(gpu_common.engine(), 64, 256, max_batch=256)
    tr.import_state(head_train.init_state_dict(64, 256, seed=1))
    xp, yd, rows = _xp(x), _dev(y), np.arange(256)

    def masks(seed, step, rate=0.1):
        m1, m2 = tr.step(xp, yd, rows, 1e-3, 0.9, 0.0, 0.6, 1.0, rate, seed=seed, step=step, want_masks=True)
        return m1.cpu().numpy(), m2.cpu().numpy()
    a, b, c, d = masks(7, 3), masks(7, 3), masks(7, 4), masks(8, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])            # the same key, the same masks
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], d[0])    # another step, another seed
    assert not np.array_equal(a[0].reshape(-1)[:256 * 128], a[1].reshape(-1))   # another layer: the same element numbers, other bits
    assert a[0].shape == (256, 256) and set(np.unique(a[0])) <= {0, 1}
    keep, n, p = int(a[0].sum()), 65536, 0.9
    assert abs(keep - n * p) <= 5 * np.sqrt(n * p * (1 - p)), keep
    z = masks(7, 3, rate=0.0)
    assert z[0].all() and z[1].all()


# ---- 12. SWA and the BatchNorm refresh ----------------------------------------------------------------------------------
def test_swa_update_and_bn_refresh():
    from torch.optim.swa_utils import AveragedModel, update_bn
    g, init, _ = _golden()
    tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
    tr.import_state(init)
    tr.copy(head_train.SWA, head_train.LIVE)
    xp, y = _xp(g["x"]), _dev(g["y"])
    ref = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        m = R.make_model(init, 0.0, dt)
        ref[name] = (m, R.make_sgd(m, CFG["lr"], CFG["mu"], CFG["wd"]), AveragedModel(m))
    eps = []
    for s, b in enumerate(g["batches"][:3]):
        tr.step(xp, y, b, CFG["lr"], CFG["mu"], CFG["wd"], CFG["l1_w"], CFG["rank_w"], 0.0, seed=0, step=s)
        tr.swa_update()
        eps.append(_dz1_eps(ref["64"][0], g["x"][b], g["y"][b], CFG))
        for m, opt, avg in ref.values():
            R.train_step(m, opt, g["x"][b], g["y"][b], CFG["l1_w"], CFG["rank_w"])
            avg.update_parameters(m)
    got = tr.export_state(head_train.SWA)
    assert int(got["n_averaged"]) == int(ref["64"][2].n_averaged) == 3
    assert int(got["bn1.num_batches_tracked"]) == 0         # buffers are not averaged: still those of the copy
    assert np.array_equal(got["bn1.running_mean"], init["bn1.running_mean"])
    s32, s64 = R.state_of(ref["32"][2].module), R.state_of(ref["64"][2].module)
    for k in R.PARAM_KEYS:
        if k != "fc1.bias":
            grade(f"swa.{k}", got[k], s32[k], s64[k])
    # the average of fc1.bias over the three steps: no further than the live value may be after the third, plus the average's own rounding
    m64m = R.momentum_of(ref["64"][0], ref["64"][1])["fc1.bias"]
    eb, _ = _b1_bounds(eps, CFG, np.abs(s64["fc1.bias"]).max(), np.abs(m64m).max())[-1]
    check_b1("swa", got["fc1.bias"], None, s64["fc1.bias"], None, (eb + 3 * 2.0 ** -23 * np.abs(s64["fc1.bias"]).max(), None))
    batches = [b for b in g["batches"][3:6]]
    tr.update_bn(xp, batches, head_train.SWA)
    for name, (m, opt, avg) in ref.items():
        dt = torch.float32 if name == "32" else torch.float64
        update_bn([torch.as_tensor(g["x"][b]).to(dt) for b in batches], avg)
    got = tr.export_state(head_train.SWA)
    s32, s64 = R.state_of(ref["32"][2].module), R.state_of(ref["64"][2].module)
    assert int(got["bn1.num_batches_tracked"]) == int(s64["bn1.num_batches_tracked"]) == 3
    for k in R.BUFFER_KEYS:
        grade(f"update_bn.{k}", got[k], s32[k], s64[k])
    pred = tr.evaluate(xp, None, np.arange(48), head_train.SWA).cpu().numpy()
    grade("swa.eval_predictions", pred, R.eval_forward(ref["32"][2].module, g["x"]), R.eval_forward(ref["64"][2].module, g["x"]))


# ---- 13. round trip -----------------------------------------------------------------------------------------------------
def test_fit_head_round_trip():
    rng = np.random.RandomState(0)
    n, F = 240, 200
    x = rng.uniform(0, 10, size=(n, F)).astype(np.float32)
    mos = (3 + np.sin(x[:, 0] * 0.5) + 0.1 * x[:, 1] - 0.02 * x[:, 2] ** 2 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    eng = gpu_common.engine()
    feats = _dev(x)
    result = eng.fit_head(feats, mos, dict(n_splits=3, epochs=12, hidden_features=128, batch_size=64, seed=3))
    sd, scaler, hist = result
    assert sd["fc3.weight"].shape == (1, 64) and sd["fc1.weight"].shape == (128, F)
    for fold_losses in hist["train_loss"]:
        assert fold_losses[-1] < fold_losses[0], fold_losses
    eng.load_fitted_head(result)
    scores = eng.mlp_head(feats)
    own = hist["predictions"]
    assert torch.isfinite(scores).all() and own.shape == (n,)
    gpu_common.assert_close(scores, own, "mlp_head on the fitted head vs the training path's eval")
    tuned = eng.fine_tune_head(sd, feats, mos, dict(epochs=4, batch_size=64, initial_lr=1e-2))
    assert np.isfinite(tuned[0]["fc1.weight"]).all() and "n_averaged" in tuned[0]
    eng.load_fitted_head(tuned)
    gpu_common.assert_close(eng.mlp_head(feats), tuned[2]["predictions"], "mlp_head on the fine-tuned head vs the training path's eval")


def test_a_replaced_trainer_and_bad_inputs_are_refused():
    eng = gpu_common.engine()
    old = head_train.HeadTrainer(eng, 64, 128, max_batch=16)
    xp_old = _xp(np.zeros((4, 64), np.float32))
    new = head_train.HeadTrainer(eng, 200, 128, max_batch=16)
    with pytest.raises(RuntimeError):
        old.evaluate(xp_old, None, np.arange(4))              # the state now strides by 224 columns
    with pytest.raises(ValueError):
        new.evaluate(xp_old, None, np.arange(4))              # a matrix of another width
    with pytest.raises(IndexError):
        new.evaluate(_xp(np.zeros((4, 200), np.float32)), None, np.array([0, 4]))


# ---- 14. a step does not synchronise ------------------------------------------------------------------------------------
def test_steps_back_to_back_equal_steps_with_a_read_each():
    g, init, _ = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    torch.cuda.synchronize()
    states = []
    for read_each in (False, True):
        tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
        tr.import_state(init)
        stream = torch.cuda.Stream()
        idx = [tr._idx(g["batches"][s % 6], 48) for s in range(32)]
        with torch.cuda.stream(stream):
            for s in range(32):
                tr.step(xp, y, idx[s], 0.05, 0.9, 0.005, 0.6, 1.0, 0.1, seed=9, step=s)
                if read_each:
                    tr.read_loss(0, reset=False)
            total = tr.read_loss(0)
            states.append((tr.export_state(), tr.export_momentum(), total))
        stream.synchronize()
    (a, am, at), (b, bm, bt) = states
    assert at == bt and at[2] == 32
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in am:
        assert np.array_equal(am[k], bm[k]), k
