"""Writes tests/golden/head_train.npz: a short training run of the REFERENCE's own Mlp, MAEAndRankLoss and optim.SGD, as data.

Runs on a CPU host that has the reference checkout (its path: the first argument, or RELAX_REFERENCE).  Imports the reference's
src/model_regression.py with the absent third-party modules stubbed, the way oracle/make_golden.py imports its modules; no
reference source is copied.  Recorded: the inputs, the initial state dict, each step's loss and predictions, the gradients of
the first step, the final state dict with its BatchNorm buffers, and - when sklearn imports - KFold's indices.

    python tools/make_head_train_golden.py REFERENCE_CHECKOUT

The run: F = 200, hidden 128, 48 rows in three fixed batches of 16, two epochs, drop_rate 0, l1_w 0.6, rank_w 1.0,
SGD(lr 0.1, momentum 0.9, weight_decay 0.005).  The seed is bumped until every step stays at least MARGIN away from the
criterion's kinks (|p - y|, and |td - sign(td) pd| of every pair with unequal targets), so that no correct fp32
implementation can land on the other side of a sign or relu; the seed used is recorded.
"""
import importlib
import os
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
    sys.exit("usage: make_head_train_golden.py REFERENCE_CHECKOUT (or set RELAX_REFERENCE)")
REF_SRC = os.path.join(REF, "src")
OUT = os.path.join(ROOT, "tests", "golden", "head_train.npz")
MARGIN = 2e-4
F_, HIDDEN, ROWS, BATCH, EPOCHS = 200, 128, 48, 16, 2
L1_W, RANK_W, LR, MOMENTUM, WD = 0.6, 1.0, 0.1, 0.9, 0.005


def import_reference():
    for m in ["pandas", "scipy.io", "sklearn", "sklearn.impute", "sklearn.preprocessing", "sklearn.metrics", "sklearn.model_selection",
              "joblib", "seaborn", "matplotlib", "matplotlib.pyplot", "data_processing"]:
        try:
            importlib.import_module(m)
        except Exception:
            sys.modules[m] = mock.MagicMock()
    sys.modules["data_processing"] = mock.MagicMock()
    sys.path.insert(0, REF_SRC)
    import model_regression as mr
    return mr


def run(mr, seed):
    from head_train_ref import kink_margins
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 1, size=(ROWS, F_)).astype(np.float32)
    y = (1 + 4 * rng.uniform(0, 1, size=ROWS)).astype(np.float32)
    batches = np.stack([rng.permutation(ROWS).reshape(-1, BATCH) for _ in range(EPOCHS)]).reshape(-1, BATCH).astype(np.int32)
    torch.manual_seed(seed)
    model = mr.Mlp(input_features=F_, hidden_features=HIDDEN, drop_rate=0.0)
    crit = mr.MAEAndRankLoss()
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
    mr = import_reference()
    seed = 0
    while True:
        rec = run(mr, seed)
        if rec is not None:
            break
        seed += 1
    rec["torch_version"] = np.asarray(torch.__version__)
    rec["config"] = np.asarray([L1_W, RANK_W, LR, MOMENTUM, WD], dtype=np.float64)
    try:
        from sklearn.model_selection import KFold
        for n, k in ((53, 5), (240, 3)):
            for i, (tr, va) in enumerate(KFold(n_splits=k, shuffle=True, random_state=42).split(np.zeros(n))):
                rec[f"kfold/{n}_{k}/{i}/train"] = tr.astype(np.int64)
                rec[f"kfold/{n}_{k}/{i}/val"] = va.astype(np.int64)
    except Exception:
        print("sklearn does not import here: no KFold indices recorded")
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: seed {seed}, losses {rec['losses']}, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
