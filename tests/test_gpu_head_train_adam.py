"""-m gpu: the Adam / AdamW step of the head's training path (relax_head_train_step_adam and the optimizer-state entries, through
head_train.HeadTrainer) against torch.optim.Adam / AdamW on the restatement of tests/head_train_ref.py.

The scheme of tests/test_gpu_head_train.py: the yardstick is the restatement in fp64, the bar the error of the same restatement in
fp32 on the CPU, per tensor as max |t - t64| / max |t64| floored at 2^-24; the GPU may be BOUND = 8 times as far off.  Adam needs
three additions, because it divides a gradient by its own magnitude:
  * an element whose gradient is within rounding of zero moves by about +-lr per step with the sign of the noise, in ANY fp32
    implementation.  Parameters are therefore graded on the well-conditioned elements - those where the fp64 run's sqrt(exp_avg_sq)
    after the step is at least 1e-4 of the tensor's largest - which must be at least 99 % of every tensor; an element off that mask
    may differ from the fp64 run by 2 lr + lr wd |w| at most (both took a full step in opposite directions).  The moments are linear
    and quadratic in the gradient and graded whole.
  * fc1.bias sits in front of a BatchNorm: its gradient is rounding noise alone, so it, its moments and (over several steps)
    bn1.running_mean, which contains it, have no ratio gate.  It has the textbook bound on an Adam step instead (check 5).
  * what the ratio cannot pin for such elements, self-consistency does (check 2): from the device's own w before the step and its
    own exp_avg, exp_avg_sq and step count after it, torch's formula in fp64 gives every w after it within 2^-21 max(|w|, lr).

Ratios observed on the GPU (largest eight of 409 compared tensors; profiles/head_train_adam_parity.json is the file this module
writes when RELAX_HEAD_TRAIN_PARITY_OUT names one, unedited):
  full.exp_avg_sq.fc3.bias: 7.42
  full.exp_avg.bn1.bias: 5.83
  full.exp_avg.fc3.bias: 5.58
  full.exp_avg_sq.fc2.bias: 5.10
  full.exp_avg_sq.bn1.bias: 4.72
  full.fc1.weight: 4.47
  full.exp_avg.fc2.bias: 3.97
  free.loss[6]: 3.57
The largest are the moments of the bias gradients after the full-width step: sums over 256 rows in another order than the CPU's,
against a CPU error at or near the 2^-24 floor (exp_avg_sq doubles the gradient's relative error) - the gradients the SGD step
computes with the same kernels, where the same sums gave 5.73.  Off the full-width step nothing is above 2.7.  The mask leaves out
0.12 - 0.44 % of fc1.weight and fc2.weight on a first step, nothing of the other tensors, and nothing from the second step on.
Check 2 sits at 0.63 x 2^-21 max(|w|, lr) at most.
"""
import json
import os

import numpy as np
import pytest
import torch

import gpu_common
import head_train_ref as R
from relax_vqa_amd import head_train, synth
from relax_vqa_amd.engine import RelaxEngine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_train.npz")
BOUND = 8.0
FLOOR = 2.0 ** -24
MASK_REL = 1e-4          # well-conditioned: sqrt(exp_avg_sq) of the fp64 run >= MASK_REL x the tensor's largest
MASK_CAP = 0.01          # at most this share of a tensor may be off the mask
RATIOS = {}
B1, B2, EPS = 0.9, 0.999, 1e-8
CFG = dict(lr=1e-2, wd=5e-4, l1_w=0.6, rank_w=1.0)
GATED = tuple(k for k in R.PARAM_KEYS if k != "fc1.bias")


@pytest.fixture(scope="module", autouse=True)
def _record_ratios():
    yield
    out = os.environ.get("RELAX_HEAD_TRAIN_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"metric": "(max|gpu - fp64| / max|fp64|) / max(max|cpu fp32 - fp64| / max|fp64|, 2^-24) per compared tensor; "
                                 "parameters on the elements where the fp64 run's sqrt(exp_avg_sq) >= 1e-4 of the tensor's largest",
                       "largest_ratio": max(RATIOS.values()) if RATIOS else None, "bound": BOUND, "ratios": RATIOS}, f, indent=1, sort_keys=True)


def _err(t, ref):
    t, ref = np.asarray(t, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert np.isfinite(t).all()
    return float(np.abs(t - ref).max() / (np.abs(ref).max() + 1e-300))


def grade(name, got, cpu32, ref64):
    e, e32 = _err(got, ref64), max(_err(cpu32, ref64), FLOOR)
    ratio = e / e32
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"parity {name}: gpu {e:.3e} cpu-fp32 {e32:.3e} ratio {ratio:.2f}")
    assert ratio <= BOUND, f"{name}: GPU error {e:.3e} is {ratio:.1f} x the CPU fp32 error {e32:.3e}"


def _golden():
    g = np.load(GOLD)
    return g, {k[5:]: g[k] for k in g.files if k.startswith("init/")}


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(gpu_common.engine().device, dtype)


def _xp(x):
    F = x.shape[1]
    return gpu_common.engine().head_train_transform(_dev(x), np.ones(F), np.zeros(F))


# ---- torch's optimizers on the restatement ----------------------------------------------------------------------------------
def make_adam(model, decoupled, lr, wd):
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return cls(model.parameters(), lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)


def moments_of(model, opt):
    """({key: exp_avg}, {key: exp_avg_sq}, step) of an optimizer that has stepped."""
    named = list(model.named_parameters())
    steps = {int(opt.state[p]["step"]) for _, p in named}
    assert len(steps) == 1                      # torch's per-parameter counts are all equal: the device keeps one
    return ({k: opt.state[p]["exp_avg"].detach().numpy().copy() for k, p in named},
            {k: opt.state[p]["exp_avg_sq"].detach().numpy().copy() for k, p in named}, steps.pop())


def load_moments(model, opt, state):
    for k, p in model.named_parameters():
        opt.state[p] = {"step": torch.tensor(float(state["step"])),
                        "exp_avg": torch.as_tensor(np.asarray(state["exp_avg"][k])).to(p.dtype).reshape(p.shape).clone(),
                        "exp_avg_sq": torch.as_tensor(np.asarray(state["exp_avg_sq"][k])).to(p.dtype).reshape(p.shape).clone()}


def rounded(state, opt_state=None):
    """An fp64 run's tensors as the fp32 values an import carries."""
    f = lambda d: {k: (np.asarray(v).astype(np.float32) if np.asarray(v).dtype.kind == "f" else v) for k, v in d.items()}
    if opt_state is None:
        return f(state)
    return f(state), {"exp_avg": f(opt_state["exp_avg"]), "exp_avg_sq": f(opt_state["exp_avg_sq"]), "step": opt_state["step"]}


def restated_step(state, opt_state, x, y, decoupled, drop_rate=0.0, masks=None, cfg=CFG):
    """One Adam / AdamW step from `state` (and `opt_state`, None for a fresh optimizer) in fp32 and in fp64."""
    out = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        m = R.make_model(state, drop_rate, dt)
        opt = make_adam(m, decoupled, cfg["lr"], cfg["wd"])
        if opt_state is not None and opt_state["step"] > 0:
            load_moments(m, opt, opt_state)
        loss, _, _ = R.train_step(m, opt, x, y, cfg["l1_w"], cfg["rank_w"], masks)
        avg, sq, t = moments_of(m, opt)
        out[name] = dict(state=R.state_of(m), exp_avg=avg, exp_avg_sq=sq, step=t, loss=loss)
    return out


def conditioned(sq64):
    """The well-conditioned elements of a tensor, from the fp64 run's exp_avg_sq after the step."""
    r = np.sqrt(np.asarray(sq64, np.float64))
    return r >= MASK_REL * r.max()


# ---- checks 1 and 2 on one step ---------------------------------------------------------------------------------------------
def check_step(tag, ref, loss, got, opt, cfg=CFG, sel=None, buffers=R.BUFFER_KEYS):
    """Check 1.  `sel`: maps a key's array to the part that is compared (the full-width test looks at 64 columns of fc1.weight)."""
    sel = sel or (lambda k, a: np.asarray(a))
    r32, r64 = ref["32"], ref["64"]
    grade(f"{tag}.loss", loss, r32["loss"], r64["loss"])
    assert opt["step"] == r64["step"]
    for k in buffers:
        grade(f"{tag}.{k}", got[k], r32["state"][k], r64["state"][k])
    for k in GATED:
        for mom in ("exp_avg", "exp_avg_sq"):
            grade(f"{tag}.{mom}.{k}", sel(k, opt[mom][k]), sel(k, r32[mom][k]), sel(k, r64[mom][k]))
        g, c32, w64 = (sel(k, a).astype(np.float64) for a in (got[k], r32["state"][k], r64["state"][k]))
        mask = conditioned(sel(k, r64["exp_avg_sq"][k]))
        off = 1.0 - mask.mean()
        print(f"parity {tag}.{k}: {100 * off:.3f} % of the elements are off the well-conditioned mask")
        assert off <= MASK_CAP, f"{tag}.{k}: {100 * off:.2f} % of the tensor is ill-conditioned"
        grade(f"{tag}.{k}", g[mask], c32[mask], w64[mask])
        if (~mask).any():
            d = np.abs(g - w64)[~mask]
            assert (d <= 2 * cfg["lr"] + cfg["lr"] * cfg["wd"] * np.abs(w64[~mask])).all(), f"{tag}.{k}: off the mask by {d.max():.3e}"


def check_update(tag, before, got, opt, decoupled, lr=CFG["lr"], wd=CFG["wd"], sel=None):
    """Check 2: torch's parameter update in fp64 from the device's own w before the step and its own moments and step count after it."""
    sel = sel or (lambda k, a: np.asarray(a))
    t = opt["step"]
    step_size, bc2_sqrt = lr / (1 - B1 ** t), np.sqrt(1 - B2 ** t)
    for k in R.PARAM_KEYS:
        w0, m, v, w1 = (sel(k, a).astype(np.float64) for a in (before[k], opt["exp_avg"][k], opt["exp_avg_sq"][k], got[k]))
        want = (w0 * (1 - lr * wd) if decoupled else w0) - step_size * m / (np.sqrt(v) / bc2_sqrt + EPS)
        d = np.abs(w1 - want) / np.maximum(np.abs(want), lr)
        print(f"parity {tag}.update.{k}: off torch's formula by {d.max() * 2 ** 21:.3f} x 2^-21 max(|w|, lr)")
        assert np.isfinite(w1).all() and (d <= 2.0 ** -21).all(), f"{tag}: {k} is {d.max() * 2 ** 21:.2f} x 2^-21 max(|w|, lr) off the update formula"


def gpu_step(tr, xp, y, rows, decoupled, drop_rate=0.0, seed=5, step=0, want_masks=False, cfg=CFG):
    return tr.step_adam(xp, y, rows, cfg["lr"], B1, B2, EPS, cfg["wd"], decoupled, cfg["l1_w"], cfg["rank_w"], drop_rate, seed=seed,
                        step=step, want_masks=want_masks)


# ---- 1, 2. one step from the golden state -----------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("drop_rate", [0.0, 0.1])
def test_one_step_from_the_golden_state(drop_rate, decoupled):
    g, init = _golden()
    b = g["batches"][0]
    tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
    tr.import_state(init)
    assert tr.export_optimizer_state()["step"] == 0
    m1, m2 = gpu_step(tr, _xp(g["x"]), _dev(g["y"]), b, decoupled, drop_rate, want_masks=True)
    masks = (m1.cpu().numpy(), m2.cpu().numpy())
    ref = restated_step(init, None, g["x"][b], g["y"][b], decoupled, drop_rate, masks)
    got, opt = tr.export_state(), tr.export_optimizer_state()
    tag = f"step[{'adamw' if decoupled else 'adam'},drop={drop_rate}]"
    assert opt["step"] == 1 and int(got["bn1.num_batches_tracked"]) == 1
    assert set(opt["exp_avg"]) == set(opt["exp_avg_sq"]) == set(R.PARAM_KEYS)
    check_step(tag, ref, tr.read_loss(0)[0], got, opt)
    check_update(tag, init, got, opt, decoupled)
    assert tr.pad_abs_sum_adam() == (0.0, 0.0, 0.0)           # F = 200 is padded to 224


# ---- 3. six teacher-forced steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_six_teacher_forced_steps(decoupled):
    """Before each golden batch the device takes over the fp64 run's parameters, buffers, moments and step count (rounded to fp32), so
    every step starts from non-zero moments and its own t, and one step's noise does not reach the next."""
    g, init = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
    m64 = R.make_model(init, 0.0, torch.float64)
    o64 = make_adam(m64, decoupled, CFG["lr"], CFG["wd"])
    name = "adamw" if decoupled else "adam"
    for s, b in enumerate(g["batches"]):
        state, opt_state = R.state_of(m64), None
        if s:
            avg, sq, t = moments_of(m64, o64)
            assert t == s
            opt_state = {"exp_avg": avg, "exp_avg_sq": sq, "step": t}
            state, opt_state = rounded(state, opt_state)
        else:
            state = rounded(state)
        tr.import_state(state)
        if opt_state is not None:
            tr.import_optimizer_state(opt_state)
            back, back_opt = tr.export_state(), tr.export_optimizer_state()     # an export right after an import: bit for bit
            assert back_opt["step"] == s
            for k in R.PARAM_KEYS + R.BUFFER_KEYS:
                assert np.array_equal(back[k], state[k].reshape(back[k].shape)), k
            for k in R.PARAM_KEYS:
                assert np.array_equal(back_opt["exp_avg"][k], opt_state["exp_avg"][k].reshape(back_opt["exp_avg"][k].shape)), k
                assert np.array_equal(back_opt["exp_avg_sq"][k], opt_state["exp_avg_sq"][k].reshape(back_opt["exp_avg_sq"][k].shape)), k
        gpu_step(tr, xp, y, b, decoupled, step=s)
        ref = restated_step(state, opt_state, g["x"][b], g["y"][b], decoupled)
        got, opt = tr.export_state(), tr.export_optimizer_state()
        assert opt["step"] == s + 1 and int(got["bn1.num_batches_tracked"]) == s + 1
        check_step(f"forced[{name}][{s}]", ref, tr.read_loss(0)[0], got, opt)
        check_update(f"forced[{name}][{s}]", state, got, opt, decoupled)
        R.train_step(m64, o64, g["x"][b], g["y"][b], CFG["l1_w"], CFG["rank_w"])
    assert tr.pad_abs_sum_adam() == (0.0, 0.0, 0.0)


# ---- 4. full width ------------------------------------------------------------------------------------------------------------
def test_one_adamw_step_at_full_width():
    F, H1, B = 35203, 256, 256
    init = synth.mlp_head_state_dict()
    rng = np.random.RandomState(11)
    x = rng.uniform(0, 1, size=(B + 8, F)).astype(np.float32)
    y = (1 + 4 * rng.uniform(size=B + 8)).astype(np.float32)
    rows = rng.permutation(B + 8)[:B]
    tr = head_train.HeadTrainer(gpu_common.engine(), F, H1, max_batch=256)
    tr.import_state(init)
    gpu_step(tr, _xp(x), _dev(y), rows, True)
    ref = restated_step(init, None, x[rows], y[rows], True)
    cols = np.random.RandomState(2).choice(F, 64, replace=False)
    sel = lambda k, a: np.asarray(a)[:, cols] if k == "fc1.weight" else np.asarray(a)
    got, opt = tr.export_state(), tr.export_optimizer_state()
    check_step("full", ref, tr.read_loss(0)[0], got, opt, sel=sel)
    check_update("full", init, got, opt, True, sel=sel)
    # the 29 padded columns of W1 and of both moments, read back from the device blocks themselves: exactly 0
    assert (F + 31) // 32 * 32 - F == 29
    assert tr.pad_abs_sum_adam() == (0.0, 0.0, 0.0)


# ---- 5, 6. free-running ---------------------------------------------------------------------------------------------------------
def test_six_free_running_steps_and_fc1_bias():
    g, init = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    lr, wd = CFG["lr"], CFG["wd"]
    tr = head_train.HeadTrainer(gpu_common.engine(), 200, 128, max_batch=256)
    tr.import_state(init)
    ref = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        m = R.make_model(init, 0.0, dt)
        ref[name] = (m, make_adam(m, False, lr, wd))
    before, drift = tr.export_state(), 0.0
    for s, b in enumerate(g["batches"]):
        gpu_step(tr, xp, y, b, False, step=s)
        got, opt = tr.export_state(), tr.export_optimizer_state()
        assert np.isfinite(tr.read_loss(0)[0]) and opt["step"] == s + 1
        check_update(f"free[{s}]", before, got, opt, False)
        drift = drift + lr * wd * np.abs(before["fc1.bias"].astype(np.float64))
        before = got
        for m, o in ref.values():
            R.train_step(m, o, g["x"][b], g["y"][b], CFG["l1_w"], CFG["rank_w"])
    # check 5: an Adam step moves an element by lr (1 - b1) / sqrt(1 - b2) at most (Kingma & Ba 2015, section 2.1), whatever its
    # gradient is - here rounding noise; the L2 term's own pull is lr wd |b| per step
    b1 = before["fc1.bias"].astype(np.float64)
    moved = np.abs(b1 - init["fc1.bias"].astype(np.float64))
    bound = 6 * lr * (1 - B1) / np.sqrt(1 - B2) + drift
    print(f"parity free.fc1.bias: moved by {moved.max():.3e} at most (bound {bound.min():.3e})")
    assert np.isfinite(b1).all() and (moved <= bound).all()
    # a bias in front of a train-mode BatchNorm cannot change the loss: the seventh step's is as close to the fp64 run's as fp32 gets
    b = g["batches"][0]
    gpu_step(tr, xp, y, b, False, step=6)
    losses = {n: R.train_step(m, o, g["x"][b], g["y"][b], CFG["l1_w"], CFG["rank_w"])[0] for n, (m, o) in ref.items()}
    grade("free.loss[6]", tr.read_loss(0)[0], losses["32"], losses["64"])


def test_adam_steps_back_to_back_equal_steps_with_a_read_each():
    g, init = _golden()
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
                tr.step_adam(xp, y, idx[s], 1e-3, B1, B2, EPS, 0.005, bool(s % 2), 0.6, 1.0, 0.1, seed=9, step=s)
                if read_each:
                    tr.read_loss(0, reset=False)
            total = tr.read_loss(0)
            states.append((tr.export_state(), tr.export_optimizer_state(), total))
        stream.synchronize()
    (a, ao, at), (b, bo, bt) = states
    assert at == bt and at[2] == 32 and ao["step"] == bo["step"] == 32
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for mom in ("exp_avg", "exp_avg_sq"):
        for k in ao[mom]:
            assert np.array_equal(ao[mom][k], bo[mom][k]), (mom, k)


# ---- 7. SGD is untouched --------------------------------------------------------------------------------------------------------
def test_sgd_after_adam_equals_sgd_on_an_engine_that_never_ran_adam():
    g, init = _golden()
    results = []
    for eng, adam_first in ((gpu_common.engine(), True), (RelaxEngine(0), False)):
        F = g["x"].shape[1]
        xp = eng.head_train_transform(_dev(g["x"]), np.ones(F), np.zeros(F))
        y = _dev(g["y"])
        if adam_first:
            tr = head_train.HeadTrainer(eng, 200, 128, max_batch=256)
            tr.import_state(init)
            for s in range(3):
                tr.step_adam(xp, y, g["batches"][s], 1e-2, decoupled=bool(s % 2), step=s)
            assert tr.export_optimizer_state()["step"] == 3
        tr = head_train.HeadTrainer(eng, 200, 128, max_batch=256)
        tr.import_state(init)
        for s, b in enumerate(g["batches"]):
            tr.step(xp, y, b, 0.1, 0.9, 0.005, 0.6, 1.0, 0.1, seed=2, step=s)
        results.append((tr.export_state(), tr.export_momentum(), tr.read_loss(0)))
        if adam_first:                       # SGD never writes the second moments, and the import zeroed them and the step count
            opt = tr.export_optimizer_state()
            assert opt["step"] == 0 and all(not v.any() for v in opt["exp_avg_sq"].values())
    (a, am, al), (b, bm, bl) = results
    assert al == bl
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in am:
        assert np.array_equal(am[k], bm[k]), k


# ---- 8. round trip ----------------------------------------------------------------------------------------------------------------
def _synthetic_set():
    rng = np.random.RandomState(0)
    n, F = 240, 200
    x = rng.uniform(0, 10, size=(n, F)).astype(np.float32)
    mos = (3 + np.sin(x[:, 0] * 0.5) + 0.1 * x[:, 1] - 0.02 * x[:, 2] ** 2 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return x, mos


def test_fit_head_round_trip_under_adam():
    x, mos = _synthetic_set()
    eng = gpu_common.engine()
    feats = _dev(x)
    cfg = dict(optimizer_type="adam", initial_lr=1e-3, n_splits=3, epochs=12, hidden_features=128, batch_size=64, seed=3)
    result = eng.fit_head(feats, mos, cfg)
    sd, scaler, hist = result
    assert sd["fc3.weight"].shape == (1, 64) and sd["fc1.weight"].shape == (128, x.shape[1])
    for fold_losses in hist["train_loss"]:
        assert fold_losses[-1] < fold_losses[0], fold_losses
    assert hist["lr"] == head_train.lr_schedule(12, 1e-3, int(12 * 0.7), True, scheduler="step", step_size=2, gamma=0.95)
    eng.load_fitted_head(result)
    scores = eng.mlp_head(feats)
    assert torch.isfinite(scores).all() and hist["predictions"].shape == (240,)
    gpu_common.assert_close(scores, hist["predictions"], "mlp_head on the Adam-fitted head vs the training path's eval")
    # the hold-out protocol hands the configuration through to fit_head
    res = eng.holdout_protocol(feats, mos, dict(cfg, epochs=2), n_repeats=1)
    assert res["repeats"][0]["state_dict"]["fc1.weight"].shape == (128, x.shape[1]) and np.isfinite(res["SRCC_test"]).all()


def test_fine_tune_head_runs_adamw():
    """One epoch of one batch, no SWA: the returned model is the live one after exactly one step, so torch's AdamW formula on the
    starting weights and the device's exported moments must give it (check 2) - and Adam's, without the decay, must not."""
    x, mos = _synthetic_set()
    eng = gpu_common.engine()
    start = head_train.init_state_dict(x.shape[1], 128, seed=4)
    lr, wd = 1e-2, 0.1
    cfg = dict(optimizer_type="adam", initial_lr=lr, weight_decay=wd, epochs=1, batch_size=240, use_swa=False, drop_rate=0.0)
    tuned, _, hist = eng.fine_tune_head(start, _dev(x), mos, cfg)
    assert hist["lr"] == [lr, lr]
    opt = hist["optimizer_state"]
    assert opt["step"] == 1
    check_update("fine_tune", start, tuned, opt, True, lr=lr, wd=wd)
    with pytest.raises(AssertionError):
        check_update("fine_tune as Adam", start, tuned, opt, False, lr=lr, wd=wd)


def test_resuming_from_an_exported_optimizer_state():
    g, init = _golden()
    xp, y = _xp(g["x"]), _dev(g["y"])
    eng = gpu_common.engine()
    tr = head_train.HeadTrainer(eng, 200, 128, max_batch=256)
    tr.import_state(init)
    for s in range(3):
        gpu_step(tr, xp, y, g["batches"][s], True, 0.1, seed=7, step=s)
    state, opt_state = tr.export_state(), tr.export_optimizer_state()
    gpu_step(tr, xp, y, g["batches"][3], True, 0.1, seed=7, step=3)
    want, want_opt = tr.export_state(), tr.export_optimizer_state()
    tr2 = head_train.HeadTrainer(eng, 200, 128, max_batch=256)
    tr2.import_state(state)
    tr2.import_optimizer_state(opt_state)
    gpu_step(tr2, xp, y, g["batches"][3], True, 0.1, seed=7, step=3)
    got, got_opt = tr2.export_state(), tr2.export_optimizer_state()
    assert got_opt["step"] == want_opt["step"] == 4
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for mom in ("exp_avg", "exp_avg_sq"):
        for k in want_opt[mom]:
            assert np.array_equal(got_opt[mom][k], want_opt[mom][k]), (mom, k)
    short = dict(opt_state["exp_avg"], **{"fc2.bias": np.zeros(3, np.float32)})
    with pytest.raises(RuntimeError):                                            # a tensor of another size: refused, nothing written
        tr2.import_optimizer_state({"exp_avg": short, "exp_avg_sq": short, "step": 3})
    with pytest.raises(ValueError):
        tr2.import_optimizer_state({"exp_avg": short, "exp_avg_sq": opt_state["exp_avg_sq"], "step": 3})
    after = tr2.export_optimizer_state()
    assert after["step"] == 4 and np.array_equal(after["exp_avg"]["fc2.bias"], want_opt["exp_avg"]["fc2.bias"])
