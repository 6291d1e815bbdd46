"""Inputs and references of the streaming-attention checks (csrc/attention_stream.hip), shared by tests/test_gpu_vit_patch8.py and
tools/vit_patch8_bench.py: the operator-level cases, their fp64 reference on the CPU, torch's own fp32 result on the CPU (the yardstick
of the 785-token parity gate), and the gate itself, read from profiles/vit_patch8_parity.json."""
import functools
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "vit_patch8_parity.json")
PARITY_CAP = 8.0      # the cap the head-training parity uses

# (ntok, images, heads): what each exercises
CASES = [
    (33, 2, 3),       # the second key tile holds one real key
    (64, 1, 3),       # no padding at all
    (197, 3, 12),     # comparison with the single-tile kernels
    (785, 2, 3),      # the real geometry
    (785, 6, 12),     # more work items (504) than CUs
]
SCALES = [1.0, 4.0]   # N(0,1) operands; x 4: logits of +-60, near one-hot rows
KEY_ORDERS = ["ascending", "descending"]


def random_qkv(ntok, n_img, heads, scale):
    g = np.random.default_rng(1000 * ntok + 10 * n_img + heads)
    return torch.from_numpy(g.standard_normal((n_img * ntok, 3 * heads * 64), dtype=np.float32) * np.float32(scale))


def ordered_qkv(order, ntok=785, n_img=1, heads=3):
    """k_j proportional to j u for a fixed unit vector u, every q a positive multiple of u: logits a_i j / ntok with a_i in [10, 60].
    ascending: the row maximum sits in the LAST key tile and every tile raises it (a rescale at every tile); descending: it sits in the
    first tile.  V is N(0,1)."""
    g = np.random.default_rng(7)
    u = g.standard_normal(64)
    u = (u / np.linalg.norm(u)).astype(np.float32)
    j = np.arange(ntok, dtype=np.float32)
    ramp = (j if order == "ascending" else (ntok - 1 - j)) / np.float32(ntok)
    qkv = np.empty((n_img, ntok, 3, heads, 64), dtype=np.float32)
    a = g.uniform(10.0, 60.0, (n_img, ntok, heads)).astype(np.float32)
    qkv[:, :, 0] = a[..., None] * u
    qkv[:, :, 1] = (8.0 * ramp)[None, :, None, None] * u
    qkv[:, :, 2] = g.standard_normal((n_img, ntok, heads, 64), dtype=np.float32)
    return torch.from_numpy(qkv.reshape(n_img * ntok, 3 * heads * 64))


def attention_cpu(qkv, n_img, ntok, heads, dtype):
    t = qkv.to(dtype).reshape(n_img, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4)
    attn = ((t[0] @ t[1].transpose(-2, -1)) * 64 ** -0.5).softmax(dim=-1)
    return (attn @ t[2]).transpose(1, 2).reshape(n_img * ntok, heads * 64)


@functools.lru_cache(maxsize=None)
def case(ntok, n_img, heads, scale):
    """-> (qkv fp32, fp64 reference, torch-CPU fp32 result), computed once per case"""
    qkv = random_qkv(ntok, n_img, heads, scale)
    return qkv, attention_cpu(qkv, n_img, ntok, heads, torch.float64), attention_cpu(qkv, n_img, ntok, heads, torch.float32)


@functools.lru_cache(maxsize=None)
def order_case(order):
    qkv = ordered_qkv(order)
    return qkv, attention_cpu(qkv, 1, 785, 3, torch.float64)


def parity_ratio(got, ref64, cpu32):
    """How far the kernel's result is from fp64, in units of torch-CPU fp32's own distance: the larger of the mean and the max ratio."""
    e = (got.cpu().double() - ref64).abs()
    c = (cpu32.double() - ref64).abs()
    return max(e.mean().item() / c.mean().item(), e.max().item() / c.max().item())


def parity_gate():
    """The gate of the 785-token fp32 parity check: the next power of two above the measured ratio recorded in
    profiles/vit_patch8_parity.json, capped at PARITY_CAP (a ratio above the cap is a bug, not a gate)."""
    with open(PARITY_JSON) as f:
        ratio = float(json.load(f)["fp32_stream_vs_torch_cpu_fp32"]["worst_ratio"])
    gate = 1.0
    while gate <= ratio:
        gate *= 2.0
    return min(gate, PARITY_CAP)
