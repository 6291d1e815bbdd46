"""CPU checks of the plain head (no BatchNorm; the reference's src/model_regression_simple.py): the restatement of
tests/head_plain_ref.py against the reference's own recorded run (tests/golden/head_plain.npz), the hold-out split, the
configuration, the two new C entries, and the condition the GPU tests' Adam gate puts on its inputs.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import _lib, head_train, metrics

import head_plain_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "head_plain.npz")
MARGIN = 2e-4
MASK_CAP = 0.01
NEW_SYMBOLS = {"relax_head_train_init_ex": 5, "relax_head_train_arch": 2}


def _golden():
    g = np.load(GOLD)
    init = {k[5:]: g[k] for k in g.files if k.startswith("init/")}
    final = {k[6:]: g[k] for k in g.files if k.startswith("final/")}
    return g, init, final


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max() / (np.abs(np.asarray(want, np.float64)).max() + 1e-30))


def test_restatement_replays_the_reference_run():
    """The fp32 restatement on the recorded inputs gives the reference's recorded losses, predictions, first-step gradients,
    final parameters and momentum buffers to 1e-6 relative (of each tensor's largest magnitude): fp32 rounding, the same CPU ops."""
    g, init, final = _golden()
    assert set(init) == set(final) == set(P.PARAM_KEYS)          # the reference's simple Mlp has no bn1
    l1_w, rank_w, lr, mu, wd = g["config"]
    model = P.make_model(init)
    opt = P.make_sgd(model, lr, mu, wd)
    for s, b in enumerate(g["batches"]):
        loss, pred, grads = P.train_step(model, opt, g["x"][b], g["y"][b], l1_w, rank_w)
        assert abs(loss - g["losses"][s]) <= 1e-6 * abs(g["losses"][s]), (s, loss, g["losses"][s])
        assert _rel(pred, g["preds"][s]) <= 1e-6, s
        if s == 0:
            assert set(grads) == set(P.PARAM_KEYS)
            for k, v in grads.items():
                assert _rel(v, g["grad0/" + k]) <= 1e-6, k
            assert np.abs(g["grad0/fc1.bias"]).max() > 1e-4      # unlike the BatchNorm head's, fc1.bias has a real gradient
    got = P.state_of(model)
    for k, v in final.items():
        assert _rel(got[k], v) <= 1e-6, k
    for k, v in P.momentum_of(model, opt).items():
        assert _rel(v, g["momentum/" + k]) <= 1e-6, k


def test_fixture_and_cases_stay_away_from_the_criterions_kinks():
    g, _, _ = _golden()
    assert len(g["batches"]) == 6 and g["x"].shape == (48, 200) and g["init/fc1.weight"].shape == (128, 200)
    for s, b in enumerate(g["batches"]):
        m1, m2 = P.kink_margins(g["preds"][s], g["y"][b])
        assert m1 >= MARGIN and m2 >= MARGIN, (s, m1, m2)
        assert np.abs(g["preds"][s]).max() < 8
    for B in P.SMALL_BATCHES:                      # the synthetic one-step cases of the GPU tests: the same margin in their fp64 forward
        init, x, y, rows = P.small_case(B)
        m = P.make_model(init, 0.0, torch.float64)
        m.train()
        pred = m(torch.as_tensor(x[rows], dtype=torch.float64)).detach().numpy().reshape(-1)
        m1, m2 = P.kink_margins(pred, y[rows])
        assert m1 >= MARGIN and m2 >= MARGIN, (B, m1, m2)


def test_holdout_split_equals_sklearns_train_test_split():
    g, _, _ = _golden()
    sizes = sorted({int(k.split("/")[1]) for k in g.files if k.startswith("split/")})
    assert sizes == [53, 240]
    for n in sizes:
        train, val = metrics.holdout_split(n, 0.2, 42)
        assert np.array_equal(train, g[f"split/{n}/train"]) and np.array_equal(val, g[f"split/{n}/val"]), n
        assert len(val) == int(np.ceil(0.2 * n)) and sorted(np.concatenate([train, val])) == list(range(n))


def test_config_accepts_the_variant_and_the_validation_and_refuses_other_values():
    base = head_train._config(None)
    assert base["batchnorm"] is True and base["validation"] == "kfold"
    want = dict(n_splits=10, batch_size=256, epochs=20, hidden_features=256, drop_rate=0.1, loss_type="MAERankLoss", optimizer_type="sgd",
                select_criteria="bykrcc", initial_lr=1e-1, weight_decay=0.005, patience=5, use_swa=True, l1_w=0.6, rank_w=1.0,
                momentum=0.9, seed=0, beta1=0.9, beta2=0.999, adam_eps=1e-8, lr_step_size=2, lr_gamma=0.95)
    assert {k: base[k] for k in want} == want                          # the defaults without the new keys are unchanged
    assert set(base) - set(want) == {"batchnorm", "validation", "logistic_fit"}
    cfg = head_train._config({"batchnorm": False, "validation": "holdout"})
    assert cfg["batchnorm"] is False and cfg["validation"] == "holdout" and cfg["epochs"] == 20
    for bad in ({"batchnorm": 2}, {"batchnorm": "no"}, {"batchnorm": None}, {"validation": "loo"}, {"validation": True}):
        with pytest.raises(ValueError):
            head_train._config(bad)
    simple = head_train._config(head_train.SIMPLE_DEFAULTS)
    assert (simple["batchnorm"], simple["validation"], simple["epochs"], simple["initial_lr"], simple["weight_decay"]) == (
        False, "holdout", 120, 1e-2, 5e-4)
    assert head_train.PLAIN_STATE_KEYS == P.PARAM_KEYS
    sd = head_train.init_state_dict(200, 128, seed=3, batchnorm=False)
    full = head_train.init_state_dict(200, 128, seed=3)
    assert tuple(sd) == P.PARAM_KEYS and all(np.array_equal(sd[k], full[k]) for k in sd)
    assert head_train.is_plain_state_dict({"module." + k: v for k, v in sd.items()}) and not head_train.is_plain_state_dict(full)


def test_simple_defaults_equal_the_reference_scripts_argparse_defaults():
    """tests/golden/head_plain.npz carries the defaults of model_regression_simple.py's add_argument lines as data."""
    g, _, _ = _golden()
    ref = {k[9:]: g[k].item() for k in g.files if k.startswith("argparse/")}
    assert (ref["epochs"], ref["initial_lr"], ref["weight_decay"]) == (120, 1e-2, 5e-4)
    cfg = head_train._config(head_train.SIMPLE_DEFAULTS)
    for k in ("batch_size", "epochs", "hidden_features", "drop_rate", "loss_type", "optimizer_type", "select_criteria", "initial_lr",
              "weight_decay", "patience", "use_swa", "l1_w", "rank_w"):
        assert cfg[k] == ref[k], (k, cfg[k], ref[k])
    assert set(head_train.SIMPLE_DEFAULTS) == {"batchnorm", "validation", "epochs", "initial_lr", "weight_decay"}


def test_new_symbols_are_exported_and_no_stream_prototype_is_new():
    raw = open(os.path.join(ROOT, "include", "relax_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in relax_hip.h"
        assert "relax_stream" not in m.group(1), name            # host-only entries: the variant is a property of the state
        assert len(m.group(1).split(",")) == n_args, name
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"librelax_hip.so does not export {name}"
    protos = re.findall(r"^(?:int|int64_t|const char\*)\s+(relax_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert len([n for n, p in protos if re.search(r"\brelax_stream\b", p)]) == 68       # (67 when this test was written; relax_op_pool_stats since)
    assert lib.relax_abi_version() == 1


def _off_mask_shares(init, x, y, kind, drop_rate=0.0, masks=None):
    m = P.make_model(init, drop_rate, torch.float64)
    opt = P.make_optimizer(m, kind, P.ADAM_CFG["lr"], P.ADAM_CFG["wd"])
    P.train_step(m, opt, x, y, P.ADAM_CFG["l1_w"], P.ADAM_CFG["rank_w"], masks)
    _, sq, _ = P.moments_of(m, opt)
    return {k: 1.0 - P.conditioned(v).mean() for k, v in sq.items()}


def test_the_adam_cases_keep_99_percent_of_every_tensor_on_the_mask():
    """The Adam gate compares the elements whose sqrt(exp_avg_sq) in the fp64 run is at least 1e-4 of the tensor's largest, and
    allows at most 1 % of a tensor off that mask: a condition on the inputs, held here for every case the GPU tests step under
    Adam / AdamW.  With dropout the device's own masks decide (the GPU test asserts the cap on them); a seeded Bernoulli(0.9) mask
    stands in here."""
    g, init, _ = _golden()
    b = g["batches"][0]
    rng = np.random.RandomState(0)
    masks = ((rng.uniform(size=(16, 128)) >= 0.1).astype(np.uint8), (rng.uniform(size=(16, 64)) >= 0.1).astype(np.uint8))
    cases = [("golden", init, g["x"][b], g["y"][b], 0.0, None), ("golden, dropout", init, g["x"][b], g["y"][b], 0.1, masks)]
    for B in P.SMALL_BATCHES:
        i, x, y, rows = P.small_case(B)
        cases.append((f"B={B}", i, x[rows], y[rows], 0.0, None))
    i, x, y, rows = P.full_width_case()
    cases.append(("full width", i, x[rows], y[rows], 0.0, None))
    for name, i, x, y, rate, mk in cases:
        for kind in (("adamw",) if name == "full width" else ("adam", "adamw")):
            for k, off in _off_mask_shares(i, x, y, kind, rate, mk).items():
                print(f"{name} {kind} {k}: {100 * off:.3f} % off the mask")
                assert off <= MASK_CAP, (name, kind, k, off)
