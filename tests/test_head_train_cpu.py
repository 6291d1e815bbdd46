"""CPU checks of the head's training path: the restatement the GPU tests compare against is pinned to a recorded run of the
reference's own classes (tests/golden/head_train.npz), and the host arithmetic of head_train.py (learning-rate chain, fold
indices, Kendall tau-b) against torch / sklearn / scipy."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import _lib, head_train

import head_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "head_train.npz")
MARGIN = 2e-4


def _golden():
    g = np.load(GOLD)
    init = {k[5:]: g[k] for k in g.files if k.startswith("init/")}
    final = {k[6:]: g[k] for k in g.files if k.startswith("final/")}
    return g, init, final


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max() / (np.abs(np.asarray(want, np.float64)).max() + 1e-30))


def test_restatement_replays_the_reference_run():
    """The fp32 restatement on the recorded inputs gives the reference's recorded losses, predictions, first-step gradients,
    final parameters, BatchNorm buffers and momentum buffers to 1e-6 relative (of each tensor's largest magnitude).  Observed
    with the generating torch (2.10): 0 on every tensor - the same CPU ops in the same order."""
    g, init, final = _golden()
    l1_w, rank_w, lr, mu, wd = g["config"]
    model = R.make_model(init)
    opt = R.make_sgd(model, lr, mu, wd)
    for s, b in enumerate(g["batches"]):
        loss, pred, grads = R.train_step(model, opt, g["x"][b], g["y"][b], l1_w, rank_w)
        assert abs(loss - g["losses"][s]) <= 1e-6 * abs(g["losses"][s]), (s, loss, g["losses"][s])
        assert _rel(pred, g["preds"][s]) <= 1e-6, s
        if s == 0:
            for k, v in grads.items():
                assert _rel(v, g["grad0/" + k]) <= 1e-6, k
    got = R.state_of(model)
    for k, v in final.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v) == len(g["batches"])
        else:
            assert _rel(got[k], v) <= 1e-6, k
    for k, v in R.momentum_of(model, opt).items():
        assert _rel(v, g["momentum/" + k]) <= 1e-6, k


def test_fixture_stays_away_from_the_criterions_kinks():
    """Every step of the fixture (none is left out anywhere) keeps |p - y| and, for pairs with unequal targets,
    |td - sign(td) pd| at least 2e-4: hundreds of fp32 roundings of a prediction of the fixture's magnitude (at most 5.2)."""
    g, _, _ = _golden()
    assert len(g["batches"]) == 6
    for s, b in enumerate(g["batches"]):
        m1, m2 = R.kink_margins(g["preds"][s], g["y"][b])
        assert m1 >= MARGIN and m2 >= MARGIN, (s, m1, m2)
        assert np.abs(g["preds"][s]).max() < 8     # one fp32 ulp below 8 is 4.8e-7: the margin is 400 of them


@pytest.mark.parametrize("epochs", [20, 120])
@pytest.mark.parametrize("initial_lr", [1e-1, 1e-2])
@pytest.mark.parametrize("swa_frac", [0.7, 0.75])
def test_learning_rate_equals_torchs_chained_schedulers(epochs, initial_lr, swa_frac):
    from torch.optim.lr_scheduler import CosineAnnealingLR
    from torch.optim.swa_utils import SWALR
    import warnings
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=initial_lr, momentum=0.9)
    sched = CosineAnnealingLR(opt, T_max=epochs, eta_min=1e-5)
    swa = SWALR(opt, swa_lr=initial_lr, anneal_strategy="cos")
    swa_start = int(epochs * swa_frac)
    want = [opt.param_groups[0]["lr"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for epoch in range(epochs):
            opt.step()
            sched.step()
            if epoch >= swa_start:
                swa.step()
            want.append(opt.param_groups[0]["lr"])
    got = head_train.lr_schedule(epochs, initial_lr, swa_start)
    assert len(got) == epochs + 1
    for e, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-12 * abs(b), (e, a, b)


def test_fold_indices_equal_sklearns_kfold():
    g, _, _ = _golden()
    try:
        from sklearn.model_selection import KFold
    except Exception:
        KFold = None
    recorded = [k for k in g.files if k.startswith("kfold/")]
    if KFold is not None:
        for n, k in ((53, 5), (240, 3), (960, 10)):
            want = list(KFold(n_splits=k, shuffle=True, random_state=42).split(np.zeros(n)))
            for (tr, va), (wtr, wva) in zip(head_train.kfold_indices(n, k), want):
                assert np.array_equal(tr, wtr) and np.array_equal(va, wva)
    # with or without sklearn here: the indices sklearn gave where the fixture was made
    assert recorded
    if True:
        for n, k in ((53, 5), (240, 3)):
            for i, (tr, va) in enumerate(head_train.kfold_indices(n, k)):
                assert np.array_equal(tr, g[f"kfold/{n}_{k}/{i}/train"]) and np.array_equal(va, g[f"kfold/{n}_{k}/{i}/val"])
    sizes = [len(va) for _, va in head_train.kfold_indices(53, 5)]
    assert sizes == [11, 11, 11, 10, 10]


def test_kendall_tau_b_equals_scipys():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.RandomState(3)
    for n in (2, 5, 24, 97):
        x = rng.normal(size=n)
        y = x + rng.normal(size=n)
        for xs, ys in ((x, y), (np.round(x), y), (np.round(x), np.round(y * 2) / 2)):
            want = stats.kendalltau(xs, ys)[0]
            got = head_train.kendall_tau_b(xs, ys)
            assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-12, (n, got, want)
    assert np.isnan(head_train.kendall_tau_b(np.ones(5), np.arange(5)))


def test_epoch_batches_keep_the_short_batch_and_skip_a_single_row():
    b = head_train.epoch_batches(40, 16, np.random.RandomState(0))
    assert [len(v) for v in b] == [16, 16, 8] and sorted(np.concatenate(b).tolist()) == list(range(40))
    with pytest.warns(UserWarning):
        b = head_train.epoch_batches(33, 16, None)
    assert [len(v) for v in b] == [16, 16]


NEW_SYMBOLS = {
    "relax_head_fit_scaler": 10, "relax_head_train_transform": 8, "relax_head_train_init": 4, "relax_head_train_import": 8,
    "relax_head_train_export_numel": 1, "relax_head_train_export": 6, "relax_head_train_copy": 4, "relax_head_criterion": 9,
    "relax_head_train_step": 17, "relax_head_train_eval": 11, "relax_head_train_bn_pass": 8, "relax_head_train_swa_update": 2,
    "relax_head_train_loss_read": 5, "relax_head_train_pad_abs_sum": 3, "relax_head_train_dw1": 7,
}


def test_new_symbols_are_exported_with_the_headers_signatures():
    text = open(os.path.join(ROOT, "include", "relax_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in relax_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"librelax_hip.so does not export {name}"
    assert lib.relax_abi_version() == 1
