"""Writes tests/golden/head_plain.npz: a short training run of the REFERENCE's own plain Mlp (src/model_regression_simple.py, bn1
commented out), MAEAndRankLoss and optim.SGD, as data.  The counterpart of tools/make_head_train_golden.py for the head without
BatchNorm.

Runs on a CPU host that has the reference checkout (its path: the first argument, or RELAX_REFERENCE).  Imports the reference's
src/model_regression_simple.py with the absent third-party modules stubbed; no reference source is copied.  Recorded: the inputs,
the initial state dict, each step's loss and predictions, the gradients of the first step, the final state dict, the momentum
buffers, the values of the script's argparse defaults that head_train.SIMPLE_DEFAULTS restates (read from its add_argument lines
as data) and - when sklearn imports - train_test_split's indices for two sizes.

    python tools/make_head_plain_golden.py REFERENCE_CHECKOUT

The run has the shape of the BatchNorm fixture: F = 200 (Fpad = 224), hidden 128, 48 rows in three fixed batches of 16, two epochs,
drop_rate 0, l1_w 0.6, rank_w 1.0, SGD(lr 0.1, momentum 0.9, weight_decay 0.005).  The seed is bumped until every step stays at
least MARGIN away from the criterion's kinks; the seed used is recorded.
"""
import ast
import importlib
import os
import re
import sys
from unittest import mock

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RELAX_REFERENCE")
if not REF:
    sys.exit("usage: make_head_plain_golden.py REFERENCE_CHECKOUT (or set RELAX_REFERENCE)")
REF_SRC = os.path.join(REF, "src")
OUT = os.path.join(ROOT, "tests", "golden", "head_plain.npz")
MARGIN = 2e-4
F_, HIDDEN, ROWS, BATCH, EPOCHS = 200, 128, 48, 16, 2
L1_W, RANK_W, LR, MOMENTUM, WD = 0.6, 1.0, 0.1, 0.9, 0.005
ARGS = ("batch_size", "epochs", "hidden_features", "drop_rate", "loss_type", "optimizer_type", "select_criteria", "initial_lr",
        "weight_decay", "patience", "use_swa", "l1_w", "rank_w", "n_repeats")


def import_reference():
    for m in ["pandas", "scipy.io", "scipy.stats", "scipy.optimize", "sklearn", "sklearn.impute", "sklearn.preprocessing", "sklearn.metrics",
              "sklearn.model_selection", "joblib", "seaborn", "matplotlib", "matplotlib.pyplot", "data_processing"]:
        try:
            importlib.import_module(m)
        except Exception:
            sys.modules[m] = mock.MagicMock()
    sys.modules["data_processing"] = mock.MagicMock()
    sys.path.insert(0, REF_SRC)
    import model_regression_simple as mrs
    return mrs


def argparse_defaults(path):
    """{name: default} of the script's add_argument lines, for the names in ARGS: values, read as data."""
    out = {}
    with open(path) as f:
        for line in f:
            m = re.search(r"add_argument\('--(\w+)'.*?default=([^,)]+)", line)
            if m and m.group(1) in ARGS:
                out[m.group(1)] = ast.literal_eval(m.group(2).strip())
    return out


def run(mrs, seed):
    from head_train_ref import kink_margins
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, size=(ROWS, F_)).astype(np.float32)
    y = (1 + 4 * rng.uniform(0, 1, size=ROWS)).astype(np.float32)
    batches = np.stack([rng.permutation(ROWS).reshape(-1, BATCH) for _ in range(EPOCHS)]).reshape(-1, BATCH).astype(np.int32)
    torch.manual_seed(seed)
    model = mrs.Mlp(input_features=F_, hidden_features=HIDDEN, drop_rate=0.0)
    assert not any(k.startswith("bn1") for k in model.state_dict()), "the reference's simple Mlp has a bn1 after all"
    crit = mrs.MAEAndRankLoss()
    crit.l1_w, crit.rank_w = L1_W, RANK_W
    opt = torch.optim.SGD(model.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=WD)
    rec = {"x": x, "y": y, "batches": batches, "seed": np.int64(seed)}
    for k, v in model.state_dict().items():
        rec["init/" + k] = v.detach().numpy().copy()
    losses, preds = [], []
    model.train()
    for s, b in enumerate(batches):
        xb, yb = torch.from_numpy(x[b]), torch.from_numpy(y[b])
        opt.zero_grad()
        out = model(xb)
        loss = crit(out, yb.view(-1, 1))
        loss.backward()
        m1, m2 = kink_margins(out.detach().numpy(), y[b])
        if min(m1, m2) < MARGIN:
            return None
        if s == 0:
            for k, p in model.named_parameters():
                rec["grad0/" + k] = p.grad.detach().numpy().copy()
        opt.step()
        losses.append(float(loss.detach()))
        preds.append(out.detach().numpy().reshape(-1).copy())
    rec["losses"] = np.asarray(losses, dtype=np.float64)
    rec["preds"] = np.stack(preds)
    for k, v in model.state_dict().items():
        rec["final/" + k] = v.detach().numpy().copy()
    for k, p in model.named_parameters():
        rec["momentum/" + k] = opt.state[p]["momentum_buffer"].detach().numpy().copy()
    return rec


def main():
    mrs = import_reference()
    seed = 0
    while True:
        rec = run(mrs, seed)
        if rec is not None:
            break
        seed += 1
    rec["torch_version"] = np.asarray(torch.__version__)
    rec["config"] = np.asarray([L1_W, RANK_W, LR, MOMENTUM, WD], dtype=np.float64)
    for k, v in argparse_defaults(os.path.join(REF_SRC, "model_regression_simple.py")).items():
        rec["argparse/" + k] = np.asarray(v)
    try:
        from sklearn.model_selection import train_test_split
        for n in (53, 240):
            tr, va = train_test_split(np.arange(n), test_size=0.2, random_state=42)
            rec[f"split/{n}/train"] = tr.astype(np.int64)
            rec[f"split/{n}/val"] = va.astype(np.int64)
    except Exception:
        print("sklearn does not import here: no train_test_split indices recorded")
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: seed {seed}, losses {rec['losses']}, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
