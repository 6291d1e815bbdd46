"""Restatement (TEST INFRASTRUCTURE, not product) of what the head's training path computes, in torch on the CPU, in fp32 or
fp64: the reference's Mlp in train mode, its MAE + rank criterion, optim.SGD, the scaler fit.  This project's own text, in the
manner of oracle/mlp_ref.py; pinned to the reference's own classes by tests/golden/head_train.npz
(tools/make_head_train_golden.py), replayed in tests/test_head_train_cpu.py.

Follows src/model_regression.py: Mlp :37-58, MAEAndRankLoss.forward :69-89 (use_margin off), preprocess_data :122-135,
optim.SGD(momentum=0.9) :382.  Dropout takes GIVEN masks (the GPU step's own, written out by it): no generator is restated.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

BN_EPS = 1e-5
PARAM_KEYS = ("fc1.weight", "fc1.bias", "bn1.weight", "bn1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
BUFFER_KEYS = ("bn1.running_mean", "bn1.running_var")


class Mlp(nn.Module):
    def __init__(self, input_features, hidden_features=256, drop_rate=0.0):
        super().__init__()
        self.fc1 = nn.Linear(input_features, hidden_features)
        self.bn1 = nn.BatchNorm1d(hidden_features, eps=BN_EPS, momentum=0.1)
        self.fc2 = nn.Linear(hidden_features, hidden_features // 2)
        self.fc3 = nn.Linear(hidden_features // 2, 1)
        self.drop_rate = drop_rate
        self.masks = None          # (mask1 [B,H1], mask2 [B,H2]) of the next train-mode forward

    def _drop(self, h, layer):
        if not self.training or self.drop_rate == 0:
            return h
        if self.masks is None:
            raise RuntimeError("train-mode forward with dropout needs the masks of the step it replays")
        return h * torch.as_tensor(self.masks[layer]).to(h.dtype) / (1.0 - self.drop_rate)

    def forward(self, x):
        h = self._drop(F.gelu(self.bn1(self.fc1(x))), 0)
        h = self._drop(F.gelu(self.fc2(h)), 1)
        return self.fc3(h)


def make_model(state_dict, drop_rate=0.0, dtype=torch.float32):
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items() if k != "n_averaged"}
    hidden, feats = sd["fc1.weight"].shape
    m = Mlp(feats, hidden, drop_rate)
    sd.setdefault("bn1.num_batches_tracked", torch.tensor(0))
    sd["fc3.weight"] = sd["fc3.weight"].reshape(1, -1)
    m.load_state_dict(sd)
    return m.to(dtype)


def state_of(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def mae_rank_loss(pred, target, l1_w=0.6, rank_w=1.0):
    """pred, target [B] (any float dtype) -> scalar."""
    pred, target = pred.reshape(-1), target.reshape(-1)
    n = pred.shape[0]
    l_mae = (pred - target).abs().mean() * l1_w
    pd = pred[:, None] - pred[None, :]
    td = target[:, None] - target[None, :]
    l_rank = F.relu(td - torch.sign(td) * pd).sum() / (n * (n - 1))
    return l_mae + l_rank * rank_w


def make_sgd(model, lr, momentum=0.9, weight_decay=0.005):
    return torch.optim.SGD(model.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)


def train_step(model, opt, x, y, l1_w=0.6, rank_w=1.0, masks=None, lr=None):
    """One iteration of the reference's train_one_epoch.  Returns (loss, predictions, gradients by key) as numpy."""
    model.train()
    model.masks = masks
    if lr is not None:
        for g in opt.param_groups:
            g["lr"] = lr
    dtype = next(model.parameters()).dtype
    x = torch.as_tensor(x).to(dtype)
    y = torch.as_tensor(y).to(dtype)
    opt.zero_grad()
    pred = model(x).reshape(-1)
    loss = mae_rank_loss(pred, y, l1_w, rank_w)
    loss.backward()
    grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    opt.step()
    model.masks = None
    return float(loss.detach()), pred.detach().numpy().copy(), grads


def momentum_of(model, opt):
    return {k: opt.state[p]["momentum_buffer"].detach().numpy().copy() for k, p in model.named_parameters()}


@torch.no_grad()
def eval_forward(model, x):
    model.eval()
    dtype = next(model.parameters()).dtype
    return model(torch.as_tensor(x).to(dtype)).reshape(-1).numpy().copy()


def fit_scaler(x):
    """preprocess_data's fit in numpy float64: NaN / inf -> 0, column mean, MinMaxScaler's scale_ / min_."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[~np.isfinite(x)] = 0.0
    dmin, dmax = x.min(axis=0), x.max(axis=0)
    rng = dmax - dmin
    scale = np.where(rng < 10 * np.finfo(np.float64).eps, 1.0, 1.0 / np.where(rng == 0, 1.0, rng))
    return {"imputer_statistics": x.mean(axis=0), "scale": scale, "min": 0.0 - dmin * scale, "data_min": dmin, "data_max": dmax}


def train_transform(x, scale, min_):
    x = np.asarray(x, dtype=np.float64).copy()
    x[~np.isfinite(x)] = 0.0
    return (x * scale + min_).astype(np.float32)


def kink_margins(pred, target):
    """Distances of a batch from the criterion's kinks: min |p - y| and min |td - sign(td) pd| over pairs with td != 0."""
    p = np.asarray(pred, dtype=np.float64).ravel()
    y = np.asarray(target, dtype=np.float64).ravel()
    td = y[:, None] - y[None, :]
    v = np.abs(td - np.sign(td) * (p[:, None] - p[None, :]))
    return float(np.abs(p - y).min()), float(v[td != 0].min())
