"""The contractions and the backbones past 2^31- and 2^32-byte tensors: the sizes between 512 and 2048 fragments at which the headline
benchmark runs and no other test does (tests/large_batch_cases.py states which tensor each case pushes past which threshold, at the
smallest count that crosses, and tests/test_large_batch_cases_cpu.py checks that table without a GPU).

Every big input is gathered on the device from a small device-resident block by the index map i -> i % period, so nothing larger than the
block exists on the host, and with the tail split off every row of the big result has to be, bit for bit, the row of the block's result
it is a copy of (a): no row depends on its batch.  The block's own result goes against an fp64 CPU reference (b).  The periods are primes
(997 rows, 61 and 7 images): they divide no tile size, so tiles straddle period boundaries, and 2^31 / row_bytes or 2^32 / row_bytes is
never a multiple of the period, so an address that wraps by 2^31 or 2^32 bytes cannot land on a row of equal content (asserted per case
in tests/test_large_batch_cases_cpu.py::test_a_wrap_never_lands_on_equal_content).

The cases run on a private engine whose arenas (tens of GB at these counts) are released when the module ends; the operator cases come
first, the models after.  RELAX_LARGE_BATCH_OUT=path writes each test's wall time and the engine's peak workspace as JSON
(profiles/large_batch_parity.json)."""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet50_ref, vit_ref
from relax_vqa_amd.engine import LAYER_STACK_DIM, RN50_POOL_DIM, RelaxEngine, pack_conv_weight
from tests import large_batch_cases as lb, vit_canvas_ref, vit_layers_ref, vit_patch8_cases
from tests.gpu_common import assert_close, launches, synth

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x6", "f16x2"]
NEEDED_FREE_GIB = 80
SEEN = {"seconds": {}, "peak_workspace_mib": 0}
# gpu_common.launches: {read kind: launches}; 0 the exact-fp32 kernel, 3 bf16x6, 7 every f16x2 launch, 9 the plain f16x2 GEMMs
ROUTE_FP32, ROUTE_X6, ROUTE_H2_GEMM, ROUTE_H2_CONV = {0: 1, 3: 0, 7: 0, 9: 0}, {0: 0, 3: 1, 7: 0, 9: 0}, {0: 0, 3: 0, 7: 1, 9: 1}, {0: 0, 3: 0, 7: 1, 9: 0}


@functools.lru_cache(maxsize=None)
def _rn_weights():
    return synth.resnet50_state_dict()


@functools.lru_cache(maxsize=None)
def _vit_weights():
    return synth.vit_state_dict("vit_base")


@pytest.fixture(scope="module")
def eng():
    free = torch.cuda.mem_get_info()[0]
    if free < NEEDED_FREE_GIB << 30:
        pytest.skip(f"the large-batch cases need {NEEDED_FREE_GIB} GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    e = RelaxEngine(0)
    e.load_resnet50(_rn_weights())
    e.load_vit(_vit_weights(), "vit_base")
    yield e
    e.close()
    torch.cuda.empty_cache()
    out = os.environ.get("RELAX_LARGE_BATCH_OUT")
    if out and SEEN["seconds"]:
        with open(out, "w") as f:
            json.dump({"what": "tests/test_gpu_large_batch.py: wall seconds per test (inputs gathered on the device, the launches, the slice-wise "
                               "comparison, the block's CPU reference where it is computed first) and the peak \"workspace_mib\" of the private engine",
                       **SEEN}, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _each_test(eng, request):
    """Every test starts from the defaults, gives its device memory back, and a device fault ends the session: nothing more is started on
    a card that has faulted."""
    eng.set_precision("f16x2")
    eng.set_option("gemm_split_k", 1)
    eng.set_option("att_h2_stream", 1)
    t0 = time.perf_counter()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault during {request.node.name}: {e}", returncode=3)
    SEEN["seconds"][request.node.name] = round(time.perf_counter() - t0, 2)
    SEEN["peak_workspace_mib"] = max(SEEN["peak_workspace_mib"], eng.get_option("workspace_mib"))
    torch.cuda.empty_cache()


def _periodic(block, n, period, first=0):
    """block[idx(first + i)] for i < n, gathered on the block's device"""
    return block[lb.idx(torch.arange(first, first + n, device=block.device), period)]


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _assert_rows(big, small, period, what, first=0):
    diff = lb.rows_equal_periodic(big, small, period, first=first)
    assert diff is None, (f"{what}: row {diff[0]} of {big.shape[0]} (a copy of block row {lb.idx(first + diff[0], period)}), column {diff[1]}: "
                          f"got {diff[2]!r}, the block alone gives {diff[3]!r}")


def _assert_rows_close(big, small, period, what):
    worst, row, col = lb.rows_close_periodic(big, small, period, rtol=1e-5, atol_frac=1e-5)
    print(f"\n{what}: worst err / bound {worst:.3g} at row {row}, column {col}")
    assert worst <= 1.0, f"{what}: err / bound {worst:.3g} at row {row}, column {col} (rtol 1e-5, floor 1e-5 x mean)"


def _split_off(eng):
    eng.set_option("gemm_split_k", 0)


# ---- the instrument at the real size ----------------------------------------------------------------------------------------------------
def test_the_comparison_reports_one_flipped_element_past_4g():
    """the construction and the slice-wise comparison on a tensor of more than 2^32 bytes on the device: untouched it passes, one element
    flipped in the last row (byte offset past 2^32), then one in a middle slice, is reported exactly (the small sizes:
    tests/test_large_batch_cases_cpu.py)"""
    M, P, N = lb.GEMM_ROWS, lb.PERIOD_ROWS, lb.GEMM_WIDE
    small = _rand(P, N, seed=1).cuda()
    big = _periodic(small, M, P)
    assert big.numel() * 4 >= 2 ** 32 and lb.rows_equal_periodic(big, small, P) is None
    for row, col in ((M - 1, N - 1), (M // 2 + 3, 5)):
        keep = big[row, col].item()
        big[row, col] = keep + 1.0
        assert lb.rows_equal_periodic(big, small, P) == (row, col, big[row, col].item(), small[lb.idx(row, P), col].item())
        worst, r, c = lb.rows_close_periodic(big, small, P, rtol=1e-5, atol_frac=1e-5)
        assert worst > 1.0 and (r, c) == (row, col)
        big[row, col] = keep
    assert lb.rows_close_periodic(big, small, P, rtol=1e-5, atol_frac=1e-5)[0] == 0.0


# ---- op_gemm --------------------------------------------------------------------------------------------------------------------------
# A past 2^32: [M, 3072] x [256, 3072]^T, plain, and bias + residual + GELU with out aliasing residual (fc2's form)
# out past 2^32: [M, 256] x [3072, 256]^T, bias + GELU (fc1's form), and the same with the residual in place
GEMM_SHAPES = {"a_past_4g": (lb.GEMM_WIDE, lb.GEMM_NARROW, ("plain", "bias_res_gelu")),
               "out_past_4g": (lb.GEMM_NARROW, lb.GEMM_WIDE, ("bias_gelu", "bias_res_gelu"))}
GEMM_CASES = [(s, f) for s, (_, _, forms) in GEMM_SHAPES.items() for f in forms]


@functools.lru_cache(maxsize=None)
def _gemm_block(shape):
    """-> the block's operands (host) and the fp64 reference of each form"""
    K, N, _ = GEMM_SHAPES[shape]
    P = lb.PERIOD_ROWS
    A, W, b, r = _rand(P, K, seed=K + 1), _rand(N, K, seed=K + 2, scale=K ** -0.5), _rand(N, seed=K + 3), _rand(P, N, seed=K + 4)
    y = A.double() @ W.double().T
    want = {"plain": y, "bias_gelu": F.gelu(y + b.double()), "bias_res_gelu": F.gelu(y + b.double() + r.double())}
    return A, W, b, r, {k: v.float().numpy() for k, v in want.items()}


def _gemm(eng, A, W, b, r, form):
    """r: a tensor of this call's own (the in-place form overwrites it)"""
    if form == "plain":
        return eng.op_gemm(A, W)
    if form == "bias_gelu":
        return eng.op_gemm(A, W, b, act=2)
    return eng.op_gemm(A, W, b, r, act=2, out=r)


def _gemm_pair(eng, shape, form):
    """-> (out_big, out_small, launches of the big call)"""
    A, W, b, r, _ = _gemm_block(shape)
    A, W, b, r = A.cuda(), W.cuda(), b.cuda(), r.cuda()
    M, P = lb.GEMM_ROWS, lb.PERIOD_ROWS
    small = _gemm(eng, A, W, b, r.clone(), form)
    big_r = _periodic(r, M, P) if form == "bias_res_gelu" else None
    big_A = _periodic(A, M, P)
    big, counts = launches(eng, lambda: _gemm(eng, big_A, W, b, big_r, form))
    return big, small, counts


@pytest.mark.parametrize("shape,form", GEMM_CASES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_op_gemm_rows_past_4g_are_the_blocks_bits(eng, precision, shape, form):
    eng.set_precision(precision)
    _split_off(eng)
    big, small, counts = _gemm_pair(eng, shape, form)
    assert counts == {"fp32": ROUTE_FP32, "bf16x6": ROUTE_X6, "f16x2": ROUTE_H2_GEMM}[precision], f"another kernel family ran: {counts}"
    assert tuple(big.shape) == (lb.GEMM_ROWS, GEMM_SHAPES[shape][1])
    _assert_rows(big, small, lb.PERIOD_ROWS, f"op_gemm {shape} {form} {precision}")
    assert_close(small, _gemm_block(shape)[4][form], f"op_gemm {shape} {form} {precision}: the block against fp64")


@pytest.mark.parametrize("shape,form", GEMM_CASES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_op_gemm_past_4g_with_the_tail_split_on(eng, precision, shape, form):
    """the default finishing path: equal to fp32 rounding, the bound the headline test uses for split on against split off"""
    eng.set_precision(precision)
    big, small, _ = _gemm_pair(eng, shape, form)
    _assert_rows_close(big, small, lb.PERIOD_ROWS, f"op_gemm {shape} {form} {precision}, tail split on")
    assert_close(small, _gemm_block(shape)[4][form], f"op_gemm {shape} {form} {precision}, tail split on: the block against fp64")


# ---- op_conv2d_nhwc -------------------------------------------------------------------------------------------------------------------
# name -> H, Cin, Cout, k, pad; the input is addressed by pixel and lies past 2^32 bytes from image 1338 on
CONVS = {"conv1x1": (56, 256, 64, 1, 0), "conv3x3": (112, 64, 64, 3, 1)}
# under f16x2 the 3x3 is the narrow gemm_x6<H2> form; the 1x1 onto 64 columns has no f16x2 kernel and runs bf16x6 on the fp32 pixels
CONV_ROUTES = {("conv1x1", "f16x2"): ROUTE_X6, ("conv3x3", "f16x2"): ROUTE_H2_CONV}


@functools.lru_cache(maxsize=None)
def _conv_block(name):
    H, Cin, Cout, k, pad = CONVS[name]
    P = lb.PERIOD_OP_IMAGES
    x, w = _rand(P, Cin, H, H, seed=H + 1), _rand(Cout, Cin, k, k, seed=H + 2, scale=(Cin * k * k) ** -0.5)
    b, r = _rand(Cout, seed=H + 3), _rand(P, Cout, H, H, seed=H + 4)
    y = F.conv2d(x.double(), w.double(), b.double(), padding=pad)
    want = {False: F.relu(y).float().numpy(), True: F.relu(y + r.double()).float().numpy()}
    return (x.permute(0, 2, 3, 1).contiguous(), torch.from_numpy(pack_conv_weight(w.numpy())), b, r.permute(0, 2, 3, 1).contiguous(), want)


@pytest.mark.parametrize("residual", [False, True], ids=["relu", "residual_relu"])
@pytest.mark.parametrize("name", list(CONVS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_op_conv2d_pixels_past_4g_are_the_blocks_bits(eng, precision, name, residual):
    H, Cin, Cout, k, pad = CONVS[name]
    x, wp, b, r, want = _conv_block(name)
    x, wp, b, r = x.cuda(), wp.cuda(), b.cuda(), r.cuda()
    n, P = lb.CONV_IMAGES, lb.PERIOD_OP_IMAGES
    eng.set_precision(precision)
    _split_off(eng)
    small = eng.op_conv2d_nhwc(x, wp, b, r if residual else None, Cout, k, k, 1, pad, act=1)
    big_x, big_r = _periodic(x, n, P), _periodic(r, n, P) if residual else None
    big, counts = launches(eng, lambda: eng.op_conv2d_nhwc(big_x, wp, b, big_r, Cout, k, k, 1, pad, act=1))
    route = CONV_ROUTES.get((name, precision), {"fp32": ROUTE_FP32, "bf16x6": ROUTE_X6}.get(precision))
    assert counts == route, f"another kernel family ran: {counts}"
    what = f"op_conv2d_nhwc {name} {'residual ' if residual else ''}{precision}"
    assert tuple(big.shape) == (n, H, H, Cout)
    _assert_rows(big, small, P, what)
    assert_close(small.permute(0, 3, 1, 2), want[residual], f"{what}: the block against fp64")


# ---- attention ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attention_block(ntok, heads):
    P = lb.PERIOD_OP_IMAGES
    qkv = vit_patch8_cases.random_qkv(ntok, P, heads, 1.0)
    return qkv, vit_patch8_cases.attention_cpu(qkv, P, ntok, heads, torch.float64).float().numpy()


def _attention_case(eng, fn, n, ntok, heads, what):
    qkv, want = _attention_block(ntok, heads)
    P = lb.PERIOD_OP_IMAGES
    qkv = qkv.cuda()
    small = fn(qkv, P)
    big_qkv = _periodic(qkv.view(P, ntok, -1), n, P).view(n * ntok, -1)
    assert big_qkv.numel() * 4 >= 2 ** 31
    big = fn(big_qkv, n)
    _assert_rows(big.view(n, -1), small.view(P, -1), P, what)
    assert_close(small, want, f"{what}: the block against fp64")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_op_attention_qkv_past_2g(eng, precision):
    """1201 images x 12 heads = 14 412 items: every persistent workgroup walks about 56 of them with the next item's prefetch; under
    f16x2 the one scale comes from the whole tensor's maximum, which the periodic tensor shares with its block"""
    eng.set_precision(precision)
    _attention_case(eng, lambda q, n: eng.op_attention(q, n, lb.ATT_HEADS), lb.ATT_IMAGES, 197, lb.ATT_HEADS, f"op_attention {precision}")


@pytest.mark.parametrize("precision,stream", [("fp32", 1), ("bf16x6", 1), ("f16x2", 1), ("f16x2", 0)],
                         ids=["fp32", "bf16x6", "f16x2-att_h2_stream", "f16x2-bf16x6_route"])
def test_op_attention_ex_785_tokens_qkv_past_2g(eng, precision, stream):
    eng.set_precision(precision)
    eng.set_option("att_h2_stream", stream)
    ntok, heads = lb.ATT_EX_TOKENS, lb.ATT_EX_HEADS
    _attention_case(eng, lambda q, n: eng.op_attention_ex(q, n, ntok, heads), lb.ATT_EX_IMAGES, ntok, heads,
                    f"op_attention_ex {precision} att_h2_stream={stream}")


# ---- pooling (no contraction in them: fp32 only) ----------------------------------------------------------------------------------------
def test_op_bn_relu_maxpool_past_4g(eng):
    eng.set_precision("fp32")
    P, n = lb.PERIOD_OP_IMAGES, lb.CONV_IMAGES
    x, sc, sh = _rand(P, 64, 112, 112, seed=31), _rand(64, seed=32), _rand(64, seed=33)
    want = F.max_pool2d(F.relu(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)), 3, 2, 1).float().numpy()
    x, sc, sh = x.permute(0, 2, 3, 1).contiguous().cuda(), sc.cuda(), sh.cuda()
    small = eng.op_bn_relu_maxpool(x, sc, sh)
    big = eng.op_bn_relu_maxpool(_periodic(x, n, P), sc, sh)
    _assert_rows(big, small, P, "op_bn_relu_maxpool")
    assert_close(small.permute(0, 3, 1, 2), want, "op_bn_relu_maxpool: the block against fp64")


def test_op_gap_past_4g(eng):
    eng.set_precision("fp32")
    P, n = lb.PERIOD_OP_IMAGES, lb.CONV_IMAGES
    x = _rand(P, 112 * 112, 64, seed=34) + 0.3
    want = x.double().mean(dim=1).float().numpy()
    x = x.cuda()
    small = eng.op_gap(x)
    big = eng.op_gap(_periodic(x, n, P))
    _assert_rows(big, small, P, "op_gap")
    assert_close(small, want, "op_gap: the block against fp64")


# ---- the models -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _image_block():
    return np.random.default_rng(61).integers(0, 256, (lb.PERIOD_IMAGES, 224, 224, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _vit_oracle():
    tsd = vit_ref.to_torch_state_dict(_vit_weights())
    return vit_ref.tokens(tsd, _image_block()[:3], 12), vit_ref.pool_features(tsd, _image_block()[:3], 12)


@functools.lru_cache(maxsize=None)
def _rn_oracle():
    tsd = resnet50_ref.to_torch_state_dict(_rn_weights())
    return resnet50_ref.layer_stack_features(tsd, _image_block()[:3]), resnet50_ref.pool_features(tsd, _image_block()[:3])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_vit_features_1777_images(eng, precision):
    """f16x2: the fc1 planes past 2^32 and the qkv planes past 2^31; bf16x6: both past 2^32; fp32: the fc1 output"""
    want_tokens, want_pooled = _vit_oracle()
    eng.set_precision(precision)
    _split_off(eng)
    block = torch.from_numpy(_image_block()).cuda()
    n, P = lb.VIT_IMAGES, lb.PERIOD_IMAGES
    tok_s, pool_s = eng.vit_features(block, tokens=True, pooled=True)
    tok, pool = eng.vit_features(_periodic(block, n, P), tokens=True, pooled=True)
    assert tuple(tok.shape) == (n, 196, 768) and tuple(pool.shape) == (n, 2304)
    _assert_rows(tok, tok_s, P, f"vit_features tokens {precision}")
    _assert_rows(pool, pool_s, P, f"vit_features pooled {precision}")
    assert_close(tok_s[:3], want_tokens, f"vit_features tokens {precision}: the block against the oracle")
    assert_close(pool_s[:3], want_pooled, f"vit_features pooled {precision}: the block against the oracle")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_resnet50_clip_features_1342_images(eng, precision):
    """conv1's raw output and the layer1 block outputs past 2^32 (their bf16x6 planes from image 892 on); the pool rows start at image
    671 = 11 x 61, a whole number of periods"""
    want_ls, want_pool = _rn_oracle()
    eng.set_precision(precision)
    _split_off(eng)
    block = torch.from_numpy(_image_block()).cuda()
    n, P = lb.RN_IMAGES // 2, lb.PERIOD_IMAGES
    ls_s, _ = eng.resnet50_clip_features(block, P)
    _, pool_s = eng.resnet50_clip_features(block, 0)
    ls, pool = eng.resnet50_clip_features(_periodic(block, 2 * n, P), n)
    assert tuple(ls.shape) == (n, LAYER_STACK_DIM) and tuple(pool.shape) == (n, RN50_POOL_DIM)
    _assert_rows(ls, ls_s, P, f"resnet50_clip_features layer stack {precision}")
    _assert_rows(pool, pool_s, P, f"resnet50_clip_features pool {precision}", first=n)
    assert_close(ls_s[:3], want_ls, f"resnet50_clip_features layer stack {precision}: the block against the oracle")
    assert_close(pool_s[:3], want_pool, f"resnet50_clip_features pool {precision}: the block against the oracle")


def test_vit_intermediate_layers_1777_images(eng):
    """f16x2: the fused tap kernel reads the residual stream deep in the arena, behind fc1 planes of more than 2^32 bytes"""
    _split_off(eng)
    block = torch.from_numpy(_image_block()).cuda()
    n, P = lb.VIT_IMAGES, lb.PERIOD_IMAGES
    small = eng.vit_intermediate_layers(block, n=2, cls=True, pooled=True)
    big = eng.vit_intermediate_layers(_periodic(block, n, P), n=2, cls=True, pooled=True)
    taps = vit_layers_ref.intermediate_layers(vit_ref.to_torch_state_dict(_vit_weights()), vit_canvas_ref.preprocess_bgr_u8(_image_block()[:3]),
                                              12, 16, n=2, dtype=torch.float64)
    for k in range(2):
        for key in ("cls", "pooled"):
            _assert_rows(big[key][k], small[key][k], P, f"vit_intermediate_layers tap {k} {key}")
        assert_close(small["cls"][k][:3], taps[k][:, 0].float().numpy(), f"vit_intermediate_layers tap {k} cls: the block against fp64")
        assert_close(small["pooled"][k][:3], vit_layers_ref.pooled(taps[k]).astype(np.float32), f"vit_intermediate_layers tap {k} pooled: the block against fp64")


@pytest.mark.parametrize("split", [0, 1], ids=["tail_split_off", "tail_split_on"])
def test_clip_vectors_28_clips_of_32_pairs(eng, split):
    """One clip_vectors call at the benchmark's clip shape and the smallest clip count that crosses (1792 fragments per backbone), the clips
    drawn with repetition from three: every row is the row its clip gets alone - bit for bit with the tail split off, to fp32 rounding
    with it on.  (Against the oracle this path stands in tests/test_gpu_bench_path.py.)"""
    eng.set_option("gemm_split_k", split)
    distinct = [torch.from_numpy(synth.synthetic_clip(lb.CLIP_PAIRS, lb.CLIP_H, lb.CLIP_W, clip_id=700 + j, distinct=4)).cuda()
                for j in range(lb.CLIP_DISTINCT)]
    alone = torch.cat([eng.clip_vectors([c]) for c in distinct])
    both = eng.clip_vectors([distinct[lb.idx(i, lb.CLIP_DISTINCT)] for i in range(lb.CLIPS)])
    assert tuple(both.shape) == (lb.CLIPS, LAYER_STACK_DIM + RN50_POOL_DIM + 6 * 768) and bool(torch.isfinite(both).all())
    assert not torch.equal(alone[0], alone[1]) and not torch.equal(alone[1], alone[2])
    if split == 0:
        _assert_rows(both, alone, lb.CLIP_DISTINCT, "clip_vectors, 28 clips, tail split off")
    else:
        _assert_rows_close(both, alone, lb.CLIP_DISTINCT, "clip_vectors, 28 clips, tail split on")
