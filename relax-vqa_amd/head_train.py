"""Training of the quality head on the GPU: the host half (csrc/head_train.hip is the device half).

Follows the reference's src/model_regression.py and src/fine_tune.py:
  preprocess_data (:122-135)        RelaxEngine.fit_scaler + the training transform
  train_and_evaluate (:335-471)     fit_head: K-fold, SGD + CosineAnnealingLR or Adam + StepLR (:381-386) chained with SWALR,
                                    early stopping from swa_start, model selection by validation KRCC, update_bn on the kept model
  fine_tune_model (fine_tune.py:130-190)   fine_tune_head: one split, batches in order, swa_start = int(0.75 epochs); its 'adam'
                                    is AdamW (fine_tune.py:155)
Argument names and defaults are the reference's (model_regression.py:737-751).

What differs from the reference: the dropout masks and the initial weights come from this project's own
seeded generators, not torch's; the optimizers are 'sgd' and 'adam', the only criterion 'MAERankLoss' (the reference's MSELoss
branch never assigns its criterion, :379); plots and .mat / .csv bookkeeping are the caller's business.  The per-epoch selection
metric runs on the device (metrics.py, csrc/metrics.hip); kendall_tau_b and logistic_rmse below stay as its host yardsticks.
The four reported metrics and the 21-repeat median-model protocol of main() are in metrics.py.
"""
import ctypes as C
import math
import warnings

import numpy as np
import torch

from . import metrics as _metrics

DEFAULTS = dict(n_splits=10, batch_size=256, epochs=20, hidden_features=256, drop_rate=0.1, loss_type="MAERankLoss",
                optimizer_type="sgd", select_criteria="bykrcc", initial_lr=1e-1, weight_decay=0.005, patience=5, use_swa=True,
                l1_w=0.6, rank_w=1.0, momentum=0.9, seed=0, logistic_fit="scipy",
                beta1=0.9, beta2=0.999, adam_eps=1e-8, lr_step_size=2, lr_gamma=0.95,   # optimizer_type 'adam' only
                batchnorm=True, validation="kfold")   # False / 'holdout': model_regression_simple.py's head and split (SIMPLE_DEFAULTS)
LIVE, SWA, BEST = 0, 1, 2      # parameter sets of the device state
ETA_MIN = 1e-5                 # CosineAnnealingLR(eta_min=1e-5), model_regression.py:383
SWA_ANNEAL_EPOCHS = 10         # SWALR's default anneal_epochs
STATE_KEYS = ("fc1.weight", "fc1.bias", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "fc2.weight", "fc2.bias",
              "fc3.weight", "fc3.bias")
PLAIN_STATE_KEYS = tuple(k for k in STATE_KEYS if not k.startswith("bn1."))   # the plain Mlp of model_regression_simple.py:37-58
# model_regression_simple.py's protocol (its argparse defaults, :735-742, where they differ from model_regression.py's): the plain
# head, one train_test_split(test_size=0.2, random_state=42) for validation instead of the K folds
SIMPLE_DEFAULTS = dict(batchnorm=False, validation="holdout", epochs=120, initial_lr=1e-2, weight_decay=5e-4)


def is_plain_state_dict(state_dict):
    """True when no key of the state dict (a 'module.' prefix aside) belongs to bn1: the plain Mlp's."""
    return not any((k[7:] if k.startswith("module.") else k).startswith("bn1.") for k in state_dict)


# ---- pure host arithmetic ---------------------------------------------------------------------------------------------
def lr_schedule(epochs, initial_lr, swa_start=None, use_swa=True, eta_min=ETA_MIN, anneal_epochs=SWA_ANNEAL_EPOCHS,
                scheduler="cosine", step_size=2, gamma=0.95):
    """The learning rate in force during each epoch (and after the last: epochs + 1 values) when CosineAnnealingLR(T_max=epochs,
    eta_min) - or, with scheduler='step', StepLR(step_size, gamma), the Adam branch's (model_regression.py:385-386) - and, from
    swa_start on, SWALR(swa_lr=initial_lr, anneal_strategy='cos') both step on the same optimizer, as the reference chains
    them (model_regression.py:408-411).  Both schedulers are recursive in the optimizer's current lr, so each sees what the
    other wrote; this is torch's arithmetic, in float64, statement for statement."""
    if scheduler not in ("cosine", "step"):
        raise ValueError(f"head training: scheduler {scheduler!r} (cosine | step)")
    if swa_start is None:
        swa_start = int(epochs * 0.7)
    if not use_swa:
        swa_start = epochs
    lr = float(initial_lr)
    out = [lr]
    swa_steps = 0   # SWALR's _step_count - 1: its construction is step 0 and leaves the lr as it is
    for epoch in range(epochs):
        last = epoch + 1   # the scheduler's last_epoch after this step
        if scheduler == "step":
            if last % step_size == 0:
                lr = lr * gamma
        elif (last - 1 - epochs) % (2 * epochs) == 0:
            lr = lr + (initial_lr - eta_min) * (1 - math.cos(math.pi / epochs)) / 2
        else:
            lr = ((1 + math.cos(math.pi * last / epochs)) / (1 + math.cos(math.pi * (last - 1) / epochs)) * (lr - eta_min) + eta_min)
        if epoch >= swa_start:
            swa_steps += 1
            anneal = lambda t: (1 - math.cos(math.pi * t)) / 2
            prev_alpha = anneal(max(0, min(1, (swa_steps - 1) / max(1, anneal_epochs))))
            prev_lr = initial_lr if prev_alpha == 1 else (lr - prev_alpha * initial_lr) / (1 - prev_alpha)
            alpha = anneal(max(0, min(1, swa_steps / max(1, anneal_epochs))))
            lr = initial_lr * alpha + prev_lr * (1 - alpha)
        out.append(lr)
    return out


def kfold_indices(n, n_splits, random_state=42):
    """[(train_idx, val_idx)] of sklearn's KFold(n_splits, shuffle=True, random_state).split: a RandomState(random_state)
    shuffle of arange(n) cut into folds of n // k (+1 for the first n % k); both index lists ascending, as the boolean
    masks of sklearn give them."""
    idx = np.arange(n)
    np.random.RandomState(random_state).shuffle(idx)
    sizes = np.full(n_splits, n // n_splits, dtype=int)
    sizes[:n % n_splits] += 1
    out, start = [], 0
    for size in sizes:
        mask = np.zeros(n, dtype=bool)
        mask[idx[start:start + size]] = True
        out.append((np.flatnonzero(~mask), np.flatnonzero(mask)))
        start += size
    return out


def kendall_tau_b(x, y):
    """Kendall's tau-b (scipy.stats.kendalltau's statistic, ties included); nan when either input is constant."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    n = x.size
    if n < 2:
        return float("nan")
    iu = np.triu_indices(n, 1)
    sx = np.sign(x[:, None] - x[None, :])[iu]
    sy = np.sign(y[:, None] - y[None, :])[iu]
    n0 = n * (n - 1) // 2
    n1 = int((sx == 0).sum())
    n2 = int((sy == 0).sum())
    den = math.sqrt(float(n0 - n1) * float(n0 - n2))
    return float((sx * sy).sum() / den) if den > 0 else float("nan")


def logistic_rmse(y_true, y_pred):
    """RMSE after the 4-parameter logistic fit (model_regression.py:138-153); needs scipy ('byrmse' only)."""
    from scipy.optimize import curve_fit

    def f(X, b1, b2, b3, b4):
        return b2 + (b1 - b2) / (1 + np.exp(-(X - b3) / np.abs(b4)))
    beta = [np.max(y_true), np.min(y_true), np.mean(y_pred), 0.5]
    popt, _ = curve_fit(f, y_pred, y_true, p0=beta, maxfev=100000000)
    return float(np.sqrt(np.mean((y_true - f(y_pred, *popt)) ** 2)))


def epoch_batches(n, batch_size, rng=None):
    """Row positions of one epoch's batches: a seeded permutation (rng) or in order (None); the last short batch is kept as
    DataLoader keeps it, but a last batch of ONE row is skipped with a warning - train-mode BatchNorm has no variance
    there and torch raises."""
    order = rng.permutation(n) if rng is not None else np.arange(n)
    batches = [order[i:i + batch_size] for i in range(0, n, batch_size)]
    if batches and len(batches[-1]) == 1:
        warnings.warn(f"head training: the last batch of {n} rows at batch_size {batch_size} has one row and is skipped")
        batches.pop()
    return batches


def init_state_dict(input_features, hidden_features=256, seed=0, batchnorm=True):
    """A fresh Mlp's state dict: nn.Linear's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases, BatchNorm
    gamma 1 / beta 0 / mean 0 / var 1 - drawn from numpy's RandomState(seed), not torch's generator.  batchnorm=False: the plain
    Mlp's six tensors, the same draws."""
    rng = np.random.RandomState(seed)
    h1, h2 = hidden_features, hidden_features // 2

    def lin(out_f, in_f):
        k = 1.0 / math.sqrt(in_f)
        return (rng.uniform(-k, k, size=(out_f, in_f)).astype(np.float32), rng.uniform(-k, k, size=(out_f,)).astype(np.float32))
    w1, b1 = lin(h1, input_features)
    w2, b2 = lin(h2, h1)
    w3, b3 = lin(1, h2)
    if not batchnorm:
        return {"fc1.weight": w1, "fc1.bias": b1, "fc2.weight": w2, "fc2.bias": b2, "fc3.weight": w3, "fc3.bias": b3}
    return {"fc1.weight": w1, "fc1.bias": b1, "bn1.weight": np.ones(h1, np.float32), "bn1.bias": np.zeros(h1, np.float32),
            "bn1.running_mean": np.zeros(h1, np.float32), "bn1.running_var": np.ones(h1, np.float32),
            "bn1.num_batches_tracked": np.int64(0), "fc2.weight": w2, "fc2.bias": b2, "fc3.weight": w3, "fc3.bias": b3}


# ---- the device state -------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class HeadTrainer:
    """The training state of one Mlp inside a RelaxEngine (relax_head_train_*).  `xp` is the matrix after
    RelaxEngine.head_train_transform ([n, Fpad] fp32 on the device), `y` its targets (fp32 [n] on the device).
    An engine holds ONE training state: creating another HeadTrainer on it replaces the state, and every method of the
    earlier object raises from then on (its matrices may have another width than the kernels would stride by).
    batchnorm=False: the plain Mlp of model_regression_simple.py (no bn1) - the state holds the six tensors of PLAIN_STATE_KEYS,
    fc1.bias has a real gradient, update_bn does nothing; every method acts on whichever variant the state has."""

    def __init__(self, engine, input_features, hidden_features=256, max_batch=256, batchnorm=True):
        self.eng, self.lib, self.h = engine, engine.lib, engine.h
        self.F, self.H1, self.H2 = int(input_features), int(hidden_features), int(hidden_features) // 2
        self.max_batch = int(max_batch)
        self.Fpad = (self.F + 31) // 32 * 32
        self.batchnorm = bool(batchnorm)
        self.keys = STATE_KEYS if self.batchnorm else PLAIN_STATE_KEYS
        if self.batchnorm:
            engine._check(self.lib.relax_head_train_init(self.h, self.F, self.H1, self.max_batch), "relax_head_train_init")
        else:
            engine._check(self.lib.relax_head_train_init_ex(self.h, self.F, self.H1, self.max_batch, 0), "relax_head_train_init_ex")
        engine._head_train_generation = self.generation = getattr(engine, "_head_train_generation", 0) + 1

    def arch(self):
        """The variant the device state reports (relax_head_train_arch): True with bn1, False for the plain head."""
        self._live()
        out = C.c_int(-1)
        self.eng._check(self.lib.relax_head_train_arch(self.h, C.byref(out)), "relax_head_train_arch")
        return bool(out.value)

    def _live(self, xp=None, y=None):
        if getattr(self.eng, "_head_train_generation", None) != self.generation:
            raise RuntimeError("this HeadTrainer's device state has been replaced by a later HeadTrainer on the same engine")
        if xp is not None and not (xp.is_cuda and xp.dtype == torch.float32 and xp.ndim == 2 and xp.shape[1] == self.Fpad
                                   and xp.is_contiguous()):
            raise ValueError(f"head training: the matrix must be a contiguous fp32 device tensor [n, {self.Fpad}] "
                             f"(RelaxEngine.head_train_transform), got {tuple(xp.shape)} {xp.dtype}")
        if y is not None and not (y.is_cuda and y.dtype == torch.float32 and y.shape == (xp.shape[0],) and y.is_contiguous()):
            raise ValueError(f"head training: targets must be a contiguous fp32 device tensor [{xp.shape[0]}]")

    def _idx(self, index, n):
        """A batch's rows as device int32.  A host list is checked against [0, n); a device int32 tensor is passed as it is -
        the kernels clamp a row outside the matrix instead of reading there, so a wrong entry trains on a wrong row."""
        if isinstance(index, torch.Tensor) and index.dtype == torch.int32 and index.is_cuda:
            return index
        host = np.ascontiguousarray(index.cpu().numpy() if isinstance(index, torch.Tensor) else index, dtype=np.int64).reshape(-1)
        if host.size and (host.min() < 0 or host.max() >= n):
            raise IndexError(f"head training: batch rows outside [0, {n})")
        return torch.as_tensor(host.astype(np.int32)).to(self.eng.device)

    def import_state(self, state_dict, which=LIVE):
        self._live()
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        nbt = int(np.asarray(torch.as_tensor(sd.get("bn1.num_batches_tracked", 0)).cpu()))
        nav = int(np.asarray(torch.as_tensor(sd.get("n_averaged", 0)).cpu()))
        # a plain trainer hands bn1's tensors on as well: relax_head_train_import refuses them by name rather than dropping them
        wanted = STATE_KEYS if self.batchnorm else PLAIN_STATE_KEYS + tuple(k for k in STATE_KEYS if k.startswith("bn1."))
        ptrs, names, numels, n, keep = self.eng._marshal_state_dict({k: v for k, v in sd.items() if k in wanted})
        self.eng._check(self.lib.relax_head_train_import(self.h, which, ptrs, names, numels, n, nbt, nav), "relax_head_train_import")
        del keep

    def _export_flat(self, which, momentum):
        self._live()
        flat = np.empty(self.lib.relax_head_train_export_numel(self.h), dtype=np.float32)
        counters = np.zeros(2, dtype=np.int64)
        self.eng._check(self.lib.relax_head_train_export(self.h, which, int(momentum), C.c_void_p(flat.ctypes.data),
                                                         C.c_void_p(counters.ctypes.data), _stream()), "relax_head_train_export")
        return self._unflatten(flat), counters

    def _unflatten(self, flat):
        shapes = {"fc1.weight": (self.H1, self.F), "fc2.weight": (self.H2, self.H1), "fc2.bias": (self.H2,), "fc3.weight": (1, self.H2),
                  "fc3.bias": (1,)}
        out, o = {}, 0
        for key in self.keys:
            shape = shapes.get(key, (self.H1,))
            size = int(np.prod(shape))
            out[key] = flat[o:o + size].reshape(shape).copy()
            o += size
        return out

    def export_state(self, which=LIVE):
        """The set as host fp32 arrays under the reference's key names and shapes (+ bn1.num_batches_tracked; n_averaged for
        the SWA set; a plain trainer: the six tensors, no bn1 key).  RelaxEngine.load_mlp_head takes it as it is."""
        out, counters = self._export_flat(which, False)
        if self.batchnorm:
            out["bn1.num_batches_tracked"] = np.int64(counters[0])
        if which == SWA:
            out["n_averaged"] = np.int64(counters[1])
        return out

    def export_momentum(self):
        """The SGD momentum buffer of each parameter of the live set (zeros under the two buffer keys)."""
        return self._export_flat(LIVE, True)[0]

    def copy(self, dst, src):
        self._live()
        self.eng._check(self.lib.relax_head_train_copy(self.h, dst, src, _stream()), "relax_head_train_copy")

    def step(self, xp, y, index, lr, momentum=0.9, weight_decay=0.005, l1_w=0.6, rank_w=1.0, drop_rate=0.1, seed=0, step=0,
             want_masks=False):
        """One SGD step on the rows `index`.  Enqueues only; returns (mask1, mask2) uint8 device tensors if want_masks."""
        self._live(xp, y)
        index = self._idx(index, xp.shape[0])
        B = int(index.numel())
        m1 = torch.empty((B, self.H1), dtype=torch.uint8, device=self.eng.device) if want_masks else None
        m2 = torch.empty((B, self.H2), dtype=torch.uint8, device=self.eng.device) if want_masks else None
        rc = self.lib.relax_head_train_step(self.h, _ptr(xp), _ptr(y), xp.shape[0], _ptr(index), B, lr, momentum, weight_decay, l1_w,
                                            rank_w, drop_rate, int(seed), int(step), _ptr(m1), _ptr(m2), _stream())
        self.eng._check(rc, "relax_head_train_step")
        return (m1, m2) if want_masks else None

    def step_adam(self, xp, y, index, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.005, decoupled=False, l1_w=0.6, rank_w=1.0,
                  drop_rate=0.1, seed=0, step=0, want_masks=False):
        """One Adam (decoupled: AdamW) step on the rows `index`, otherwise as step().  One state takes either step() or step_adam()
        between two import_state calls, not both: the first optimizer block is SGD's momentum to the one and exp_avg to the other."""
        self._live(xp, y)
        index = self._idx(index, xp.shape[0])
        B = int(index.numel())
        m1 = torch.empty((B, self.H1), dtype=torch.uint8, device=self.eng.device) if want_masks else None
        m2 = torch.empty((B, self.H2), dtype=torch.uint8, device=self.eng.device) if want_masks else None
        rc = self.lib.relax_head_train_step_adam(self.h, _ptr(xp), _ptr(y), xp.shape[0], _ptr(index), B, lr, beta1, beta2, eps,
                                                 weight_decay, int(bool(decoupled)), l1_w, rank_w, drop_rate, int(seed), int(step),
                                                 _ptr(m1), _ptr(m2), _stream())
        self.eng._check(rc, "relax_head_train_step_adam")
        return (m1, m2) if want_masks else None

    def export_optimizer_state(self):
        """Adam's state as torch's optimizer.state_dict() holds it: {'exp_avg': {key: array}, 'exp_avg_sq': {key: array}, 'step': t},
        host fp32 arrays under the parameters' keys."""
        self._live()
        out = {}
        for which, name in enumerate(("exp_avg", "exp_avg_sq")):
            flat = np.empty(self.lib.relax_head_train_export_numel(self.h), dtype=np.float32)
            t = C.c_int64(0)
            self.eng._check(self.lib.relax_head_train_export_optimizer(self.h, which, C.c_void_p(flat.ctypes.data), C.byref(t), _stream()),
                            "relax_head_train_export_optimizer")
            out[name] = {k: v for k, v in self._unflatten(flat).items() if not k.startswith("bn1.running_")}
            out["step"] = int(t.value)
        return out

    def import_optimizer_state(self, state):
        """What export_optimizer_state returned (or the same from torch), after import_state, which starts a new optimizer."""
        self._live()
        strip = lambda d: {(k[7:] if k.startswith("module.") else k): v for k, v in d.items()}
        avg, sq = strip(state["exp_avg"]), strip(state["exp_avg_sq"])
        keys = [k for k in self.keys if not k.startswith("bn1.running_")]
        if not self.batchnorm:   # bn1's moments, if the caller brings them, go along: the library refuses them by name
            keys += [k for k in ("bn1.weight", "bn1.bias") if k in avg and k in sq]
        ptrs, names, numels, n, keep = self.eng._marshal_state_dict({k: avg[k] for k in keys})
        ptrs_sq, _, numels_sq, _, keep_sq = self.eng._marshal_state_dict({k: sq[k] for k in keys})
        if list(numels) != list(numels_sq):
            raise ValueError("head training: exp_avg and exp_avg_sq differ in their sizes")
        self.eng._check(self.lib.relax_head_train_import_optimizer(self.h, ptrs, ptrs_sq, names, numels, n, int(state["step"])),
                        "relax_head_train_import_optimizer")
        del keep, keep_sq

    def evaluate(self, xp, y, index, which=LIVE, l1_w=0.6, rank_w=1.0):
        """Eval-mode predictions (device fp32 [B]) of one batch; with y its criterion goes into the evaluation accumulator."""
        self._live(xp, y)
        index = self._idx(index, xp.shape[0])
        B = int(index.numel())
        pred = torch.empty((B,), dtype=torch.float32, device=self.eng.device)
        rc = self.lib.relax_head_train_eval(self.h, which, _ptr(xp), _ptr(y), xp.shape[0], _ptr(index), B, l1_w, rank_w, _ptr(pred),
                                            _stream())
        self.eng._check(rc, "relax_head_train_eval")
        return pred

    def predict(self, xp, rows=None, which=LIVE):
        """Eval-mode predictions of any number of rows (batches of max_batch)."""
        rows = np.arange(xp.shape[0]) if rows is None else np.asarray(rows)
        return torch.cat([self.evaluate(xp, None, rows[i:i + self.max_batch], which) for i in range(0, len(rows), self.max_batch)])

    def bn_pass(self, xp, index, which, reset=False):
        self._live(xp)
        index = self._idx(index, xp.shape[0]) if index is not None else None
        B = int(index.numel()) if index is not None else 0
        rc = self.lib.relax_head_train_bn_pass(self.h, which, int(reset), _ptr(xp), xp.shape[0] if xp is not None else 0, _ptr(index), B,
                                               _stream())
        self.eng._check(rc, "relax_head_train_bn_pass")

    def update_bn(self, xp, batches, which):
        """torch.optim.swa_utils.update_bn over `batches` (lists of rows); nothing on a plain trainer, as update_bn returns at once
        for a model without BatchNorm."""
        if not self.batchnorm:
            self._live()
            return
        self.bn_pass(None, None, which, reset=True)
        for b in batches:
            self.bn_pass(xp, b, which)

    def swa_update(self):
        self._live()
        self.eng._check(self.lib.relax_head_train_swa_update(self.h, _stream()), "relax_head_train_swa_update")

    def read_loss(self, which=0, reset=True):
        """(sum of batch losses, sum of batch loss x rows, batches) since the last reset: the one host read of an epoch."""
        self._live()
        out = (C.c_double * 3)()
        self.eng._check(self.lib.relax_head_train_loss_read(self.h, which, int(reset), out, _stream()), "relax_head_train_loss_read")
        return float(out[0]), float(out[1]), int(out[2])

    def pad_abs_sum(self):
        """(sum |fc1.weight[:, F:Fpad]|, sum |its momentum[:, F:Fpad]|) of the live set: the K padding, exactly 0 at all times."""
        self._live()
        out = (C.c_double * 2)()
        self.eng._check(self.lib.relax_head_train_pad_abs_sum(self.h, out, _stream()), "relax_head_train_pad_abs_sum")
        return float(out[0]), float(out[1])

    def pad_abs_sum_adam(self):
        """pad_abs_sum with Adam's second moment as a third sum: (fc1.weight, exp_avg, exp_avg_sq)[:, F:Fpad], exactly 0 at all times."""
        self._live()
        out = (C.c_double * 3)()
        self.eng._check(self.lib.relax_head_train_pad_abs_sum_adam(self.h, out, _stream()), "relax_head_train_pad_abs_sum_adam")
        return float(out[0]), float(out[1]), float(out[2])

    def dw1_adam_only(self, fused, B, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.005, decoupled=False):
        """dw1_only under Adam / AdamW."""
        self._live()
        self.eng._check(self.lib.relax_head_train_dw1_adam(self.h, int(bool(fused)), int(B), lr, beta1, beta2, eps, weight_decay,
                                                           int(bool(decoupled)), _stream()), "relax_head_train_dw1_adam")

    def dw1_only(self, fused, B, lr=0.01, momentum=0.9, weight_decay=0.005):
        """The dW1 stage of a step alone, on what the last step left (tools/head_train_bench.py): fused, or GEMM + separate update."""
        self._live()
        self.eng._check(self.lib.relax_head_train_dw1(self.h, int(bool(fused)), int(B), lr, momentum, weight_decay, _stream()),
                        "relax_head_train_dw1")

    def criterion(self, pred, target, l1_w=0.6, rank_w=1.0):
        """MAEAndRankLoss of device fp32 [B] vectors -> (loss [1], gradient [B]) on the device."""
        self._live()
        pred = pred.to(self.eng.device, torch.float32).contiguous()
        target = target.to(self.eng.device, torch.float32).contiguous()
        loss = torch.empty((1,), dtype=torch.float32, device=self.eng.device)
        grad = torch.empty_like(pred)
        rc = self.lib.relax_head_criterion(self.h, _ptr(pred), _ptr(target), int(pred.numel()), l1_w, rank_w, _ptr(loss), _ptr(grad),
                                           _stream())
        self.eng._check(rc, "relax_head_criterion")
        return loss, grad


# ---- the loops --------------------------------------------------------------------------------------------------------
def _config(config):
    cfg = dict(DEFAULTS)
    cfg.update(config or {})
    if cfg["optimizer_type"] not in ("sgd", "adam"):
        raise ValueError(f"head training: optimizer_type {cfg['optimizer_type']!r} (sgd | adam)")
    if cfg["loss_type"] != "MAERankLoss":
        raise ValueError("head training: only loss_type='MAERankLoss' is implemented (the reference's MSELoss branch is dead code)")
    if cfg["select_criteria"] not in ("bykrcc", "byrmse", "val_loss"):
        raise ValueError(f"head training: select_criteria {cfg['select_criteria']!r}")
    if cfg["logistic_fit"] not in ("scipy", "device"):
        raise ValueError(f"head training: logistic_fit {cfg['logistic_fit']!r} (scipy | device)")
    if not isinstance(cfg["batchnorm"], (bool, np.bool_)):
        raise ValueError(f"head training: batchnorm {cfg['batchnorm']!r} (True | False)")
    if cfg["validation"] not in ("kfold", "holdout"):
        raise ValueError(f"head training: validation {cfg['validation']!r} (kfold | holdout)")
    if cfg["select_criteria"] == "byrmse" and cfg["logistic_fit"] == "scipy" and not _have_scipy():
        cfg["logistic_fit"] = "device"   # no curve_fit here: the device fit (csrc/metrics.hip) takes its place
    return cfg


def _have_scipy():
    try:
        import scipy.optimize  # noqa: F401
    except ImportError:
        return False
    return True


def _schedule(cfg, swa_start, use_swa):
    """The reference pairs SGD with CosineAnnealingLR and Adam / AdamW with StepLR (model_regression.py:381-386, fine_tune.py:151-158)."""
    if cfg["optimizer_type"] == "adam":
        return lr_schedule(cfg["epochs"], cfg["initial_lr"], swa_start, use_swa, scheduler="step", step_size=cfg["lr_step_size"],
                           gamma=cfg["lr_gamma"])
    return lr_schedule(cfg["epochs"], cfg["initial_lr"], swa_start, use_swa)


def _step(tr, cfg, xp, y, rows, lr, step, decoupled):
    """One step of the configured optimizer; `decoupled`: 'adam' means AdamW (fine_tune.py:155), not Adam (model_regression.py:385)."""
    if cfg["optimizer_type"] == "adam":
        tr.step_adam(xp, y, rows, lr, cfg["beta1"], cfg["beta2"], cfg["adam_eps"], cfg["weight_decay"], decoupled, cfg["l1_w"],
                     cfg["rank_w"], cfg["drop_rate"], cfg["seed"], step)
    else:
        tr.step(xp, y, rows, lr, cfg["momentum"], cfg["weight_decay"], cfg["l1_w"], cfg["rank_w"], cfg["drop_rate"], cfg["seed"], step)


def _device_krcc(engine, y_true, y_pred):
    """kendall_tau_b on the device (the pair pass of csrc/metrics.hip): the same expression from the same integer counts, so
    the two agree bit for bit and no selection changes; nan below two rows, as kendall_tau_b gives it."""
    return _metrics.kendall(engine, y_true, y_pred)["krcc"] if len(y_true) >= 2 else float("nan")


def _prepare(engine, features, mos):
    features = torch.as_tensor(features).to(engine.device, torch.float32).contiguous()
    y = torch.as_tensor(np.asarray(mos.detach().cpu() if isinstance(mos, torch.Tensor) else mos, dtype=np.float32)).to(engine.device)
    if features.ndim != 2 or y.shape != (features.shape[0],):
        raise ValueError(f"head training: features {tuple(features.shape)} / mos {tuple(y.shape)}")
    scaler = engine.fit_scaler(features)
    xp = engine.head_train_transform(features, scaler["scale"], scaler["min"])
    return xp, y, scaler


def _evaluate_set(tr, xp, y, rows, which, cfg):
    preds = [tr.evaluate(xp, y, rows[i:i + cfg["batch_size"]], which, cfg["l1_w"], cfg["rank_w"])
             for i in range(0, len(rows), cfg["batch_size"])]
    _, weighted, _ = tr.read_loss(1)
    return weighted / len(rows), torch.cat(preds).cpu().numpy().astype(np.float64)


def fit_head(engine, features, mos, config=None):
    """train_and_evaluate (model_regression.py:335-471) on the device.  features [n, F] (device tensor, as the dataset pass
    leaves it, or anything torch.as_tensor takes), mos [n].  Returns (state_dict, scaler, history): the kept model under the
    reference's key names, {'imputer_statistics', 'scale', 'min'} float64 [F], and per-fold 'train_loss' / 'val_loss' /
    'metric' / 'lr' lists plus 'best' = (fold, epoch, metric) and 'predictions', the kept model's eval-mode scores of every row
    as the training path computes them (host arrays only: nothing of the device state outlives the call).
    config['batchnorm'] = False trains the plain Mlp of model_regression_simple.py (six tensors, no bn1 key); config['validation']
    = 'holdout' runs the body once on that script's single 80/20 split (:357) instead of the K folds - the LR chain, the SWA start,
    the selection, the early stopping and the snapshot on improvement are one fold's, and history['folds'] holds that one split.
    (The script's loss-list padding, which slipped into its epoch loop when the fold loop went, is not reproduced: one list per epoch.)"""
    cfg = _config(config)   # optimizer_type 'adam': optim.Adam (weight decay as an L2 term) under StepLR, model_regression.py:385-386
    xp, y, scaler = _prepare(engine, features, mos)
    y_host = y.cpu().numpy().astype(np.float64)
    n, F = xp.shape[0], int(features.shape[1])
    epochs, bs = cfg["epochs"], cfg["batch_size"]
    batchnorm = bool(cfg["batchnorm"])
    tr = HeadTrainer(engine, F, cfg["hidden_features"], max_batch=max(2, min(bs, 1024)), batchnorm=batchnorm)
    use_swa = bool(cfg["use_swa"])
    swa_start = int(epochs * 0.7) if use_swa else epochs
    lrs = _schedule(cfg, swa_start, use_swa)
    lower_is_better = cfg["select_criteria"] in ("byrmse", "val_loss")
    best_metric = float("inf") if lower_is_better else float("-inf")
    history = {"train_loss": [], "val_loss": [], "metric": [], "lr": lrs, "best": None, "folds": []}
    have_best = False
    step = 0
    if cfg["validation"] == "holdout":   # model_regression_simple.py:357: one train_test_split(test_size=0.2, random_state=42), no KFold
        splits = [_metrics.holdout_split(n, 0.2, 42)]
    else:
        splits = kfold_indices(n, cfg["n_splits"])
    for fold, (train_idx, val_idx) in enumerate(splits):
        tr.import_state(init_state_dict(F, cfg["hidden_features"], seed=cfg["seed"] + fold, batchnorm=batchnorm), LIVE)
        if use_swa:
            tr.copy(SWA, LIVE)   # AveragedModel(model): a deep copy, n_averaged 0
        rng = np.random.RandomState(cfg["seed"] * 1000003 + fold)
        train_losses, val_losses, metrics = [], [], []
        best_val_loss, no_improve = float("inf"), 0
        for epoch in range(epochs):
            rows_seen = 0
            for b in epoch_batches(len(train_idx), bs, rng):
                _step(tr, cfg, xp, y, train_idx[b], lrs[epoch], step, decoupled=False)
                step += 1
                rows_seen += len(b)
            _, weighted, _ = tr.read_loss(0)
            train_losses.append(weighted / max(rows_seen, 1))
            swa_on = use_swa and epoch >= swa_start
            if swa_on:
                tr.swa_update()
            current = SWA if swa_on else LIVE
            val_loss, val_pred = _evaluate_set(tr, xp, y, val_idx, current, cfg)
            val_losses.append(val_loss)
            if cfg["select_criteria"] == "bykrcc":
                metric = _device_krcc(engine, y_host[val_idx], val_pred)
            elif cfg["select_criteria"] == "byrmse":
                metric = (_metrics.device_logistic_rmse(engine, y_host[val_idx], val_pred) if cfg["logistic_fit"] == "device"
                          else logistic_rmse(y_host[val_idx], val_pred))
            else:
                metric = val_loss
            metrics.append(metric)
            if (metric < best_metric) if lower_is_better else (metric > best_metric):
                best_metric = metric
                tr.copy(BEST, current)
                have_best = True
                history["best"] = (fold, epoch, metric)
            if swa_on:   # early stopping is active from swa_start; an improvement keeps the LIVE model, as the reference does (:445)
                if val_loss < best_val_loss:
                    best_val_loss, no_improve = val_loss, 0
                    tr.copy(BEST, LIVE)
                    have_best = True
                else:
                    no_improve += 1
                    if no_improve >= cfg["patience"]:
                        break
        if not have_best:   # every metric was nan (a constant validation fold): keep the last model rather than nothing
            tr.copy(BEST, LIVE)
            have_best = True
        if use_swa:
            tr.update_bn(xp, [train_idx[b] for b in epoch_batches(len(train_idx), bs, rng)], BEST)
        history["train_loss"].append(train_losses)
        history["val_loss"].append(val_losses)
        history["metric"].append(metrics)
        history["folds"].append((train_idx, val_idx))
    # the kept model's eval-mode predictions on every row, as the training path computes them (host float32 [n])
    history["predictions"] = tr.predict(xp, None, BEST).cpu().numpy()
    return tr.export_state(BEST), scaler, history


def fit_head_simple(engine, features, mos, config=None):
    """train_and_evaluate of model_regression_simple.py (:335-467), the protocol behind the reference's KoNViD-1k / YouTube-UGC /
    LIVE-VQC / CVD2014 numbers: fit_head under SIMPLE_DEFAULTS (the plain head, one 80/20 validation split, 120 epochs, lr 1e-2,
    weight decay 5e-4); `config` overrides them."""
    return fit_head(engine, features, mos, dict(SIMPLE_DEFAULTS, **(config or {})))


def fine_tune_head(engine, state_dict, features, mos, config=None):
    """fine_tune_model (fine_tune.py:130-190): start from state_dict, one split, batches in order, SWA from int(0.75 epochs);
    the result is the SWA average after update_bn (or the live model without SWA).  optimizer_type 'adam' is AdamW here
    (fine_tune.py:155).  Returns (state_dict, scaler, history); under 'adam' history['optimizer_state'] holds the live model's
    moments and step count.
    The scaler is fitted on `features`, as the reference's fine-tuning script preprocesses its own data."""
    cfg = _config(config)
    xp, y, scaler = _prepare(engine, features, mos)
    n, F = xp.shape[0], int(features.shape[1])
    epochs, bs = cfg["epochs"], cfg["batch_size"]
    hidden = int(np.asarray(state_dict["fc1.bias" if "fc1.bias" in state_dict else "module.fc1.bias"]).shape[0])
    # a state dict without bn1 keys fine-tunes the plain head (beyond the reference, whose fine_tune.py builds the BatchNorm Mlp)
    tr = HeadTrainer(engine, F, hidden, max_batch=max(2, min(bs, 1024)), batchnorm=not is_plain_state_dict(state_dict))
    tr.import_state(state_dict, LIVE)
    use_swa = bool(cfg["use_swa"])
    swa_start = int(epochs * 0.75) if use_swa else epochs
    lrs = _schedule(cfg, swa_start, use_swa)
    if use_swa:
        tr.copy(SWA, LIVE)
    losses, step = [], 0
    rows = np.arange(n)
    for epoch in range(epochs):
        rows_seen = 0
        for b in epoch_batches(n, bs, None):
            _step(tr, cfg, xp, y, rows[b], lrs[epoch], step, decoupled=True)
            step += 1
            rows_seen += len(b)
        _, weighted, _ = tr.read_loss(0)
        losses.append(weighted / max(rows_seen, 1))
        if use_swa and epoch >= swa_start:
            tr.swa_update()
    result = LIVE
    if use_swa and epochs - 1 >= swa_start:
        tr.update_bn(xp, [rows[b] for b in epoch_batches(n, bs, np.random.RandomState(cfg["seed"]))], SWA)
        result = SWA
    history = {"train_loss": losses, "lr": lrs, "predictions": tr.predict(xp, None, result).cpu().numpy()}
    if cfg["optimizer_type"] == "adam":
        history["optimizer_state"] = tr.export_optimizer_state()   # of the live model: what HeadTrainer.import_optimizer_state resumes from
    return tr.export_state(result), scaler, history
