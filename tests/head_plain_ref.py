"""Restatement (TEST INFRASTRUCTURE, not product) of the plain head's training step - the Mlp of the reference's
src/model_regression_simple.py:37-58, whose bn1 is commented out - in torch on the CPU, in fp32 or fp64, under SGD, Adam and AdamW.
This project's own text; pinned to the reference's own classes by tests/golden/head_plain.npz (tools/make_head_plain_golden.py),
replayed in tests/test_head_plain_cpu.py.  The criterion, the step, the optimizer helpers and the kink margins are those of
tests/head_train_ref.py, which this module reuses; only the model differs.

  fc1 -> GELU -> dropout -> fc2 -> GELU -> dropout -> fc3          (dropout takes GIVEN masks, as in head_train_ref)
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import head_train_ref as R

PARAM_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
B1, B2, EPS = 0.9, 0.999, 1e-8          # torch's Adam defaults, the reference's (model_regression_simple.py:381)

mae_rank_loss, make_sgd, train_step, momentum_of, state_of, eval_forward, kink_margins = (
    R.mae_rank_loss, R.make_sgd, R.train_step, R.momentum_of, R.state_of, R.eval_forward, R.kink_margins)


class PlainMlp(nn.Module):
    def __init__(self, input_features, hidden_features=256, drop_rate=0.0):
        super().__init__()
        self.fc1 = nn.Linear(input_features, hidden_features)
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
        h = self._drop(F.gelu(self.fc1(x)), 0)
        h = self._drop(F.gelu(self.fc2(h)), 1)
        return self.fc3(h)


def make_model(state_dict, drop_rate=0.0, dtype=torch.float32):
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items() if k in PARAM_KEYS}
    hidden, feats = sd["fc1.weight"].shape
    m = PlainMlp(feats, hidden, drop_rate)
    sd["fc3.weight"] = sd["fc3.weight"].reshape(1, -1)
    m.load_state_dict(sd)
    return m.to(dtype)


def make_adam(model, decoupled, lr, wd):
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return cls(model.parameters(), lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)


def make_optimizer(model, kind, lr, wd, momentum=0.9):
    """kind: 'sgd' | 'adam' | 'adamw'."""
    return make_sgd(model, lr, momentum, wd) if kind == "sgd" else make_adam(model, kind == "adamw", lr, wd)


def moments_of(model, opt):
    """({key: exp_avg}, {key: exp_avg_sq}, step) of an Adam / AdamW that has stepped."""
    named = list(model.named_parameters())
    steps = {int(opt.state[p]["step"]) for _, p in named}
    assert len(steps) == 1
    return ({k: opt.state[p]["exp_avg"].detach().numpy().copy() for k, p in named},
            {k: opt.state[p]["exp_avg_sq"].detach().numpy().copy() for k, p in named}, steps.pop())


def load_moments(model, opt, state):
    for k, p in model.named_parameters():
        opt.state[p] = {"step": torch.tensor(float(state["step"])),
                        "exp_avg": torch.as_tensor(np.asarray(state["exp_avg"][k])).to(p.dtype).reshape(p.shape).clone(),
                        "exp_avg_sq": torch.as_tensor(np.asarray(state["exp_avg_sq"][k])).to(p.dtype).reshape(p.shape).clone()}


def restated_step(state, x, y, kind, lr, wd, l1_w=0.6, rank_w=1.0, drop_rate=0.0, masks=None, momentum=0.9, opt_state=None):
    """One step from `state` in fp32 and in fp64: {'32' | '64': {'state', 'loss', 'pred', 'grads', and 'mom' (SGD) or 'exp_avg',
    'exp_avg_sq', 'step' (Adam / AdamW)}}."""
    out = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        m = make_model(state, drop_rate, dt)
        opt = make_optimizer(m, kind, lr, wd, momentum)
        if opt_state is not None and opt_state["step"] > 0:
            load_moments(m, opt, opt_state)
        loss, pred, grads = train_step(m, opt, x, y, l1_w, rank_w, masks)
        r = dict(state=state_of(m), loss=loss, pred=pred, grads=grads)
        if kind == "sgd":
            r["mom"] = momentum_of(m, opt)
        else:
            r["exp_avg"], r["exp_avg_sq"], r["step"] = moments_of(m, opt)
        out[name] = r
    return out


def conditioned(sq64, mask_rel=1e-4):
    """The well-conditioned elements of a tensor under Adam, from the fp64 run's exp_avg_sq after the step (the mask of
    tests/test_gpu_head_train_adam.py): sqrt(exp_avg_sq) >= mask_rel x the tensor's largest."""
    r = np.sqrt(np.asarray(sq64, np.float64))
    return r >= mask_rel * r.max()


# ---- the cases the GPU tests step on (tests/test_gpu_head_plain.py); tests/test_head_plain_cpu.py holds their inputs to the
# ---- Adam gate's condition without a GPU -----------------------------------------------------------------------------------
ADAM_CFG = dict(lr=1e-2, wd=5e-4, l1_w=0.6, rank_w=1.0)      # model_regression_simple.py's initial_lr and weight_decay
SGD_CFG = dict(lr=0.1, mu=0.9, wd=0.005, l1_w=0.6, rank_w=1.0)   # the golden run's
SMALL_BATCHES = (2, 37, 64)                                   # the minimum batch, an odd one, max_batch: F = 200, hidden 128


def plain_of(state_dict):
    """The six tensors of a state dict that may carry bn1 keys as well."""
    return {k: np.asarray(v) for k, v in state_dict.items() if k in PARAM_KEYS}


def small_case(B):
    """(init, x [B + 5, 200], y, rows [B]) of the one-step case at batch B."""
    from relax_vqa_amd import head_train
    rng = np.random.RandomState(100 + B)
    x = rng.uniform(0, 1, size=(B + 5, 200)).astype(np.float32)
    y = (1 + 4 * rng.uniform(size=B + 5)).astype(np.float32)
    return head_train.init_state_dict(200, 128, seed=B, batchnorm=False), x, y, rng.permutation(B + 5)[:B]


def full_width_case():
    """(init, x [264, 35203], y, rows [256]): the full-width step on the rows of tests/test_gpu_head_train.py's, from a fresh
    nn.Linear-style initial state.  (synth.mlp_head_state_dict's weights are drawn for a BatchNorm behind fc1: without it three of
    the 256 hidden units sit in GELU's flat tail with a gradient of zero, 1.17 % of fc1.bias - past the Adam gate's cap on
    ill-conditioned elements, which is a condition on the inputs.)"""
    from relax_vqa_amd import head_train
    F_, B = 35203, 256
    rng = np.random.RandomState(11)
    x = rng.uniform(0, 1, size=(B + 8, F_)).astype(np.float32)
    y = (1 + 4 * rng.uniform(size=B + 8)).astype(np.float32)
    return head_train.init_state_dict(F_, 256, seed=11, batchnorm=False), x, y, rng.permutation(B + 8)[:B]
