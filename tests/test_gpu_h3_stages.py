"""gemm_h3's operand rings (csrc/gemm_h2.hip: three LDS stages for one operand, two for the other, counted waits with DMAs in flight
across the barriers) at the smallest shapes where such a ring can go wrong.  Everything goes through op_gemm and checks with the
profile counters that the plain f16x2 GEMM (read kind 9) ran.

  1. Zero-padded K gives the same bits.  Appending whole all-zero 32-k steps to A and W leaves every row scale and every earlier
     instruction as it was and adds exact zeros to the fp32 accumulators: the outputs must be EQUAL.  K = 256 + 32 j covers every
     residue of the six-region period and both tail branches of the three-product form (8 .. 14 steps), K = 32 .. 224 the
     four-product form with fewer steps than stages (1 .. 7).  M = 300: two row tiles, the second ragged (rows past M are out-of-range
     DMA lanes).  A stage read before its DMA has landed, or a wrong wait count, shows as garbage or as a difference between two runs.
  2. The fp32-grade gate of tests/fp32_grade.py with the tail split on: every tile of a 300 x 256 problem is in the tail, so each runs
     as K slices that start at kt_begin != 0.
  3. The same gate on fc2's shape (23040 x 768 x 3072: 270 tiles, more than CUs, and a real tail).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fp32_grade
from tests.gpu_common import engine, exact_fp32_gemm, launches

pytestmark = pytest.mark.gpu

M_RAGGED = 300


def _operands(seed, M, N, K):
    g = np.random.default_rng(seed)
    A = torch.from_numpy(g.standard_normal((M, K)).astype(np.float32)).cuda()
    W = torch.from_numpy((g.standard_normal((N, K)) * K ** -0.5).astype(np.float32)).cuda()
    b = torch.from_numpy(g.standard_normal(N).astype(np.float32)).cuda()
    r = torch.from_numpy(g.standard_normal((M, N)).astype(np.float32)).cuda()
    return A, W, b, r


def _run_h3(eng, A, W, b=None, r=None, act=0, in_place=False):
    """op_gemm, asserting that the plain f16x2 GEMM ran and nothing else."""
    def run():
        if in_place:
            rr = r.clone()
            eng.op_gemm(A, W, b, rr, act=act, out=rr)
            return rr
        return eng.op_gemm(A, W, b, r, act=act)

    got, n_launch = launches(eng, run)
    assert n_launch[9] >= 1 and n_launch[3] == 0 and n_launch[0] == 0, f"not the f16x2 GEMM: {n_launch}"
    return got


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bias_inplace_residual_gelu"])
@pytest.mark.parametrize("k0,pads", [(256, (32, 64, 96, 128, 160, 192)), (32, (32, 64, 96, 128, 160, 192))],
                         ids=["three_products_nk8to14", "four_products_nk1to7"])
def test_zero_padded_k_gives_the_same_bits(k0, pads, fused):
    eng = engine()
    assert eng.precision() == "f16x2"
    A, W, b, r = _operands(11 + k0, M_RAGGED, 512, k0)
    kw = dict(b=b, r=r, act=2, in_place=True) if fused else {}
    eng.set_option("gemm_split_k", 0)       # no slice boundary moves with K
    try:
        base = _run_h3(eng, A, W, **kw)
        assert torch.isfinite(base).all()
        assert torch.equal(base, _run_h3(eng, A, W, **kw)), f"K = {k0}: two runs differ"
        for pad in pads:
            Ap, Wp = F.pad(A, (0, pad)).contiguous(), F.pad(W, (0, pad)).contiguous()
            got = _run_h3(eng, Ap, Wp, **kw)
            again = _run_h3(eng, Ap, Wp, **kw)
            assert torch.equal(got, again), f"K = {k0} + {pad} zeros: two runs differ"
            bad = (got != base).nonzero()
            assert bad.numel() == 0, (f"K = {k0} + {pad} zero columns ({(k0 + pad) // 32} steps) differs from K = {k0} at {bad.shape[0]} "
                                      f"outputs, first {bad[0].tolist()}: {got[tuple(bad[0])].item()} vs {base[tuple(bad[0])].item()}")
    finally:
        eng.set_option("gemm_split_k", 1)


def _gate(eng, M, N, K, seed):
    A, W, _, _ = _operands(seed, M, N, K)
    ref = (A.double() @ W.double().T).cpu().numpy()
    mag = (A.double().abs() @ W.double().abs().T).cpu().numpy()
    mag += fp32_grade.h2_floor(A.abs().amax(dim=1).cpu().numpy(), W.abs().amax(dim=1).cpu().numpy())
    got32 = exact_fp32_gemm(eng, A, W).cpu().numpy()
    assert eng.get_option("gemm_split_k") == 1
    got = _run_h3(eng, A, W)
    assert torch.equal(got, _run_h3(eng, A, W)), f"{M}x{N}x{K}: two runs differ"
    what = f"f16x2 gemm {M}x{N}x{K}, tail split on"
    ratios = fp32_grade.check(got.cpu().numpy(), got32, ref, mag, what, slack=fp32_grade.SLACK + fp32_grade.h2_slack(K))
    print(f"\nGATE {what}: mean e / mean e32 {ratios[0]:.3f}, max e / max e32 {ratios[1]:.3f}, max e {ratios[2]:.3e}")


@pytest.mark.parametrize("K", [256, 288, 320, 352, 384, 416, 768, 3072])
def test_gate_with_every_tile_in_the_tail(K):
    eng = engine()
    assert eng.precision() == "f16x2"
    _gate(eng, M_RAGGED, 256, K, 100 + K)


def test_gate_on_fc2_shape_more_tiles_than_cus():
    eng = engine()
    assert eng.precision() == "f16x2"
    _gate(eng, 23040, 768, 3072, 7)
