"""CPU checks of the Adam branch of the head's training path: the StepLR + SWALR learning-rate chain of head_train.lr_schedule
against torch's own schedulers stepping on one optimizer (src/model_regression.py:385-386, :408-411), the unchanged cosine default,
the accepted optimizer names, and the new C-ABI entries."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import _lib, head_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("epochs", [7, 20, 120])
@pytest.mark.parametrize("use_swa", [True, False])
@pytest.mark.parametrize("initial_lr,swa_frac", [(1e-3, 0.7), (1e-2, 0.75)])
def test_step_schedule_equals_torchs_steplr_chained_with_swalr(epochs, use_swa, initial_lr, swa_frac):
    from torch.optim.lr_scheduler import StepLR
    from torch.optim.swa_utils import SWALR
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=initial_lr, weight_decay=0.005)
    sched = StepLR(opt, step_size=2, gamma=0.95)
    swa = SWALR(opt, swa_lr=initial_lr, anneal_strategy="cos") if use_swa else None
    swa_start = int(epochs * swa_frac) if use_swa else epochs
    want = [opt.param_groups[0]["lr"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for epoch in range(epochs):          # the reference's order: the epoch's optimizer steps, scheduler.step(), then swa_scheduler.step()
            opt.step()
            sched.step()
            if use_swa and epoch >= swa_start:
                swa.step()
            want.append(opt.param_groups[0]["lr"])
    got = head_train.lr_schedule(epochs, initial_lr, swa_start, use_swa, scheduler="step", step_size=2, gamma=0.95)
    assert len(got) == epochs + 1
    for e, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-15 * abs(b), (e, a, b)
    if not use_swa:                          # plain StepLR in closed form, to the rounding of its `epochs` multiplications
        for e, a in enumerate(got):
            assert abs(a - initial_lr * 0.95 ** (e // 2)) <= epochs * 2.0 ** -52 * a
    assert got == head_train.lr_schedule(epochs, initial_lr, swa_start, use_swa, scheduler="step")   # 2 and 0.95 are the defaults


@pytest.mark.parametrize("epochs,initial_lr", [(7, 1e-1), (20, 1e-1), (120, 1e-2)])
def test_the_cosine_default_is_unchanged(epochs, initial_lr):
    for kwargs in ({}, {"swa_start": epochs // 2}, {"use_swa": False}):
        want = head_train.lr_schedule(epochs, initial_lr, **kwargs)
        assert head_train.lr_schedule(epochs, initial_lr, scheduler="cosine", **kwargs) == want
        assert head_train.lr_schedule(epochs, initial_lr, scheduler="cosine", step_size=5, gamma=0.5, **kwargs) == want
    # the closed form of CosineAnnealingLR before SWALR sets in: the default has not become the step form
    got = head_train.lr_schedule(epochs, initial_lr, use_swa=False)
    for e, a in enumerate(got):
        closed = head_train.ETA_MIN + (initial_lr - head_train.ETA_MIN) * (1 + torch.cos(torch.tensor(torch.pi * e / epochs, dtype=torch.float64))) / 2
        assert abs(a - float(closed)) <= 1e-12 * initial_lr, (e, a, float(closed))
    with pytest.raises(ValueError):
        head_train.lr_schedule(epochs, initial_lr, scheduler="exponential")


def test_config_accepts_adam_and_refuses_other_optimizers():
    cfg = head_train._config({"optimizer_type": "adam"})
    assert (cfg["beta1"], cfg["beta2"], cfg["adam_eps"], cfg["lr_step_size"], cfg["lr_gamma"]) == (0.9, 0.999, 1e-8, 2, 0.95)
    assert head_train._config(None)["optimizer_type"] == "sgd"
    for name in ("rmsprop", "adamw", "Adam", ""):
        with pytest.raises(ValueError):
            head_train._config({"optimizer_type": name})
    with pytest.raises(ValueError):
        head_train._config({"optimizer_type": "adam", "loss_type": "MSEloss"})


def test_the_schedule_follows_the_optimizer():
    sgd, adam = head_train._config({"epochs": 12}), head_train._config({"epochs": 12, "optimizer_type": "adam", "initial_lr": 1e-3})
    assert head_train._schedule(sgd, 8, True) == head_train.lr_schedule(12, 1e-1, 8, True)
    assert head_train._schedule(adam, 8, True) == head_train.lr_schedule(12, 1e-3, 8, True, scheduler="step")
    adam["lr_step_size"], adam["lr_gamma"] = 3, 0.5
    assert head_train._schedule(adam, 12, False) == [1e-3 * 0.5 ** (e // 3) for e in range(13)]


ADAM_SYMBOLS = {"relax_head_train_step_adam": 20, "relax_head_train_export_optimizer": 5, "relax_head_train_import_optimizer": 7,
                "relax_head_train_pad_abs_sum_adam": 3, "relax_head_train_dw1_adam": 10}


def test_adam_symbols_are_exported_with_the_headers_signatures():
    text = open(os.path.join(ROOT, "include", "relax_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in ADAM_SYMBOLS.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in relax_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"librelax_hip.so does not export {name}"
