"""bf16x6 (csrc/gemm_x6.hip): fp32 operands as three bf16 planes, six partial products on the bf16 MFMA, fp32 accumulate.
The claim under test is fp32-GRADE accuracy: against an fp64 reference its error is no larger than the exact-fp32 path's
(v_mfma_f32_32x32x2_f32, an fp32 FMA chain), not merely "within the 1e-3 bar"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_common import assert_close, engine, launches

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


@pytest.fixture()
def x6():
    eng = engine()
    prev = eng.precision()
    eng.set_precision("bf16x6")
    assert eng.precision() == "bf16x6"
    yield eng
    eng.set_precision(prev)


def test_f16x2_is_the_default_arithmetic():
    """(f16x2 = two fp16 planes for the plain GEMMs with N % 256 == 0 - the ViT -, bf16x6 for everything else: tests/test_gpu_h2.py)"""
    from relax_vqa_amd.engine import RelaxEngine
    eng = RelaxEngine(0)
    assert eng.precision() == "f16x2"
    eng.close()


def test_permutation_matrix_copies_values_bit_for_bit(x6):
    """W = a permutation matrix: out[m, n] = A[m, perm[n]] EXACTLY (x = hi + mid + lo is an exact split, every other
    product is 0): checks the sp3 layout, the swizzled LDS image, the DMA piece map and the C write in one go; the
    asymmetric permutation catches any transpose, M = 300 the zero-page rows past M."""
    M, K = 300, 256
    A = _rand(M, K, seed=1) * torch.logspace(-6, 6, K)[None, :]
    for N in (256, 128, 64):
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(N))[:N]
        W = torch.zeros(N, K)
        W[torch.arange(N), perm] = 1.0
        got = x6.op_gemm(A.cuda(), W.cuda()).cpu()
        assert torch.equal(got, A[:, perm]), f"N={N}"


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (1000, 256, 512), (197 * 3, 2304, 768), (50, 64, 64), (4096, 64, 576),
                                   (777, 3072, 768), (12608, 768, 3072), (2049, 384, 4608)])
def test_error_is_no_larger_than_the_fp32_paths(M, N, K):
    eng = engine()
    A, W = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5)
    ref = A.double() @ W.double().T
    eng.set_precision("fp32")
    e32 = (eng.op_gemm(A.cuda(), W.cuda()).cpu().double() - ref).abs()
    eng.set_precision("bf16x6")
    try:
        got = eng.op_gemm(A.cuda(), W.cuda())
    finally:
        pass   # the autouse fixture restores the engine's precision
    e6 = (got.cpu().double() - ref).abs()
    scale = ref.abs().mean().item()
    print(f"\\n{M}x{N}x{K}: mean |err| / mean |ref|: fp32 {e32.mean().item() / scale:.3e}  bf16x6 {e6.mean().item() / scale:.3e};"
          f"  max: fp32 {e32.max().item() / scale:.3e}  bf16x6 {e6.max().item() / scale:.3e}")
    assert_close(got, ref.float().numpy(), f"x6 gemm {M}x{N}x{K}")
    assert e6.mean().item() <= 1.05 * e32.mean().item() + 1e-12, "bf16x6 mean error exceeds the fp32 FMA chain's"
    assert e6.max().item() <= 1.5 * e32.max().item() + 1e-12, "bf16x6 worst error exceeds the fp32 FMA chain's"


def test_wide_dynamic_range_operands():
    """Values spanning 2^-40 .. 2^40 inside one row: every plane keeps fp32's exponent range (bf16 has fp32's exponent), so
    nothing over- or underflows; what is left is how the matrix core aligns 16 products of very different size before its
    single rounding.  Measured against the sum of magnitudes and beside the fp32 FMA chain on the same data."""
    eng = engine()
    M, N, K = 257, 128, 512
    g = torch.Generator().manual_seed(5)
    A = _rand(M, K, seed=3) * torch.exp2(torch.randint(-40, 41, (M, K), generator=g).float())
    W = _rand(N, K, seed=4) * torch.exp2(torch.randint(-20, 21, (N, K), generator=g).float())
    ref = A.double() @ W.double().T
    mag = (A.double().abs() @ W.double().abs().T)
    eng.set_precision("fp32")
    e32 = ((eng.op_gemm(A.cuda(), W.cuda()).cpu().double() - ref).abs() / mag)
    eng.set_precision("bf16x6")
    try:
        e6 = ((eng.op_gemm(A.cuda(), W.cuda()).cpu().double() - ref).abs() / mag)
    finally:
        pass   # the autouse fixture restores the engine's precision
    print(f"\nerr / sum|a||w|: fp32 mean {e32.mean().item():.3e} max {e32.max().item():.3e}; bf16x6 mean {e6.mean().item():.3e} max {e6.max().item():.3e}")
    assert e6.max().item() < 1e-6 and e6.mean().item() < 1.5e-7


@pytest.mark.parametrize("act", [0, 1, 2])
def test_epilogue(x6, act):
    M, N, K = 333, 192, 96
    A, W, b, r = _rand(M, K, seed=3), _rand(N, K, seed=4, scale=0.1), _rand(N, seed=5), _rand(M, N, seed=6)
    y = A.double() @ W.double().T + b.double() + r.double()
    want = [y, F.relu(y), F.gelu(y)][act].float().numpy()
    assert_close(x6.op_gemm(A.cuda(), W.cuda(), b.cuda(), r.cuda(), act=act), want, f"x6 epilogue act={act}")
    rr = r.cuda().clone()
    x6.op_gemm(A.cuda(), W.cuda(), b.cuda(), rr, act=act, out=rr)
    assert_close(rr, want, f"x6 in-place residual act={act}")


def test_gelu_is_the_erf_gelu_to_fp32_rounding(each_precision):
    """csrc/gelu.h (branch-free erfc form, tools/gelu_fit.py) against the fp64 function: identity weights make the contraction exact,
    so the output IS gelu(x).  Largest error one rounding of the result; closer to the fp64 function than torch's own fp32 GELU
    (which evaluates 1 + erf(x / sqrt 2) with its cancellation for x < 0).  Large tile (M >= 256) and small-tile / split finish paths."""
    eng = engine()
    rng = np.random.default_rng(5)
    x = np.concatenate([np.linspace(-9, 9, 64 * 700), rng.standard_normal(64 * 300) * 2, [-0.0, 0.0, 1e-30, -1e-30, 30.0, -30.0] * 32])
    x = torch.from_numpy(x[: (x.size // 64) * 64].astype(np.float32).reshape(-1, 64))
    eye = torch.eye(64)
    true = (0.5 * x.double() * torch.special.erfc(-x.double() / np.sqrt(2.0))).numpy()
    for rows in (x, x[:100]):
        got = eng.op_gemm(rows.cuda(), eye.cuda(), act=2).cpu().double().numpy()
        err = np.abs(got - true[: rows.shape[0]])
        ref_err = np.abs(F.gelu(rows).double().numpy() - true[: rows.shape[0]])
        print(f"\n{each_precision} rows {rows.shape[0]}: gelu max abs err {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e}; torch fp32: {ref_err.max():.3e} / {np.sqrt((ref_err ** 2).mean()):.3e}")
        assert err.max() < 5e-7 and np.sqrt((err ** 2).mean()) < 1e-7
        assert np.sqrt((err ** 2).mean()) <= np.sqrt((ref_err ** 2).mean())
    z = eng.op_gemm(torch.tensor([[-0.0] * 64] * 16).cuda(), eye.cuda(), act=2).cpu()
    assert torch.all(z == 0)


@pytest.mark.parametrize("M,N,K", [(300, 64, 16), (1000, 128, 256), (5000, 192, 1024), (777, 320, 4608), (256 * 9 + 5, 64, 576),
                                   (70000, 128, 512)])
def test_fp32_activation_rows_give_the_bits_of_split_planes(x6, M, N, K):
    """Contractions onto 64 / 128-column tiles (N % 256 != 0) read the fp32 rows of A and split them inside the K loop
    ("x6_fp32_rows", default on); with the option off A is converted to split planes first.  Same values, same products, same
    order: the outputs are equal bit for bit, with bias + residual + GELU and with the tail split on and off (70000 rows: more than
    one round of tiles, so whole-K tiles and K slices both occur; K = 16: a single step; 4608: the longest K of the models)."""
    A, W = _rand(M, K, seed=21).cuda(), _rand(N, K, seed=22, scale=K ** -0.5).cuda()
    b, r = _rand(N, seed=23).cuda(), _rand(M, N, seed=24).cuda()
    assert x6.get_option("x6_fp32_rows") == 1
    for split in (1, 0):
        x6.set_option("gemm_split_k", split)
        try:
            got = x6.op_gemm(A, W, bias=b, residual=r, act=2)
            x6.set_option("x6_fp32_rows", 0)
            want = x6.op_gemm(A, W, bias=b, residual=r, act=2)
        finally:
            x6.set_option("x6_fp32_rows", 1)
            x6.set_option("gemm_split_k", 1)
        assert torch.equal(got, want), f"split_k={split}"
    ref = torch.nn.functional.gelu(A.double() @ W.double().T + b.double() + r.double()).float().cpu().numpy()
    assert_close(got, ref, "fp32-row contraction")


def test_resnet50_fp32_block_outputs_give_the_bits_of_split_planes(x6):
    """ResNet-50 with the layer1 / layer2 block outputs as fp32 rows (default) against split planes everywhere: layer stack, pool
    vector, the clip path and every exported tap are equal bit for bit, with the tail split on and off."""
    rn50_weights()
    f = torch.from_numpy(_fragments(6)).cuda()
    res = {}
    for rows in (1, 0):
        x6.set_option("x6_fp32_rows", rows)
        try:
            for split in (1, 0):
                x6.set_option("gemm_split_k", split)
                ls, pool, taps = x6.resnet50_features(f, taps=range(15))
                cls, cpool = x6.resnet50_clip_features(f, 3)
                res[rows, split] = [ls, pool, cls, cpool] + [taps[i] for i in range(15)]
        finally:
            x6.set_option("x6_fp32_rows", 1)
            x6.set_option("gemm_split_k", 1)
    for split in (1, 0):
        for i, (a, b) in enumerate(zip(res[1, split], res[0, split])):
            assert torch.equal(a, b), f"output {i}, split_k={split}"


def test_split_k_is_deterministic_and_optional(x6):
    """300 tiles of 256x256: 44 tail tiles are cut along K.  Same bits run to run; with gemm_split_k = 0 the bits do not
    depend on how many rows travel together."""
    M, N, K = 256 * 100, 768, 768
    A, W = _rand(M, K, seed=8).cuda(), _rand(N, K, seed=9, scale=K ** -0.5).cuda()
    a = x6.op_gemm(A, W)
    b = x6.op_gemm(A, W)
    assert torch.equal(a, b)
    x6.set_option("gemm_split_k", 0)
    try:
        whole = x6.op_gemm(A, W)
        part = x6.op_gemm(A[: 256 * 7], W)
    finally:
        x6.set_option("gemm_split_k", 1)
    assert torch.equal(whole[: 256 * 7], part)
    assert_close(a, whole.cpu().numpy(), "split-K vs whole-K", rtol=1e-4, atol_frac=1e-5)


# ---- the ViT under bf16x6 -----------------------------------------------------------------------------------------------
import os  # noqa: E402

from oracle import fragment_ref, pooling_ref, vit_ref  # noqa: E402
from tests.gpu_common import synth, vit_weights  # noqa: E402


def _fragments(n, seed=0):
    frs = []
    for i in range(n):
        o, nx = synth.synthetic_pair(240, 320, 500 + seed * 64 + i)
        f = fragment_ref.fragment_pair(o, nx)
        frs.append(f["ori_frag"] if i % 2 == 0 else f["diff_frag"])
    return np.stack(frs)


@pytest.mark.parametrize("name,heads", [("vit_tiny", 3), ("vit_base", 12)])
def test_vit_matches_reference_golden_tokens_under_x6(golden_dir, x6, name, heads):
    vit_weights(name)
    z = np.load(os.path.join(golden_dir, f"{name}_tokens.npz"))
    tokens, pooled = x6.vit_features(torch.from_numpy(z["frags"]).cuda(), tokens=True, pooled=True)
    assert_close(tokens, z["tokens"], f"{name} tokens (bf16x6) vs reference VisionTransformer")
    want = np.stack([pooling_ref.vit_pool_vector(t) for t in z["tokens"]])
    assert_close(pooled, want, f"{name} pooled (bf16x6) vs reference process_video_feature")


def test_vit_base_error_against_fp64_is_no_larger_than_the_fp32_paths():
    """12 blocks deep: tokens of the fp32 path and of the bf16x6 path against an fp64 run of the oracle (same fp32
    weights and inputs, all arithmetic in double)."""
    sd = vit_weights("vit_base")
    eng = engine()
    frags = _fragments(3, seed=2)
    sd64 = {k: v.double() for k, v in vit_ref.to_torch_state_dict(sd).items()}
    ref = vit_ref.forward_tokens(sd64, vit_ref.preprocess_bgr_u8(frags).double(), 12).numpy()
    f = torch.from_numpy(frags).cuda()
    eng.set_precision("fp32")
    t32, _ = eng.vit_features(f, tokens=True, pooled=False)
    eng.set_precision("bf16x6")
    try:
        t6, _ = eng.vit_features(f, tokens=True, pooled=False)
        t6b, _ = eng.vit_features(f, tokens=True, pooled=False)
    finally:
        pass   # the autouse fixture restores the engine's precision
    assert torch.equal(t6, t6b), "bf16x6 is not deterministic"
    e32 = np.abs(t32.cpu().numpy().astype(np.float64) - ref)
    e6 = np.abs(t6.cpu().numpy().astype(np.float64) - ref)
    n32 = np.linalg.norm(e32) / np.linalg.norm(ref)
    n6 = np.linalg.norm(e6) / np.linalg.norm(ref)
    print(f"\nvit_base tokens vs fp64: norm-rel fp32 {n32:.3e} bf16x6 {n6:.3e}; max abs fp32 {e32.max():.3e} bf16x6 {e6.max():.3e}")
    assert n6 <= 1.1 * n32 and e6.max() <= 1.5 * e32.max()


# ---- convolutions and ResNet-50 under bf16x6 ------------------------------------------------------------------------------
from oracle import resnet50_ref  # noqa: E402
from relax_vqa_amd.engine import pack_conv_weight  # noqa: E402
from tests.gpu_common import rn50_weights  # noqa: E402

CONVS = [  # Nimg, H, Cin, Cout, k, stride, pad  (implicit GEMM: padding taps are zero-filled by the DMA's range check)
    (2, 56, 64, 64, 1, 1, 0), (2, 56, 64, 64, 3, 1, 1), (2, 56, 128, 128, 3, 2, 1), (3, 28, 256, 512, 1, 2, 0),
    (2, 14, 256, 256, 3, 1, 1), (5, 7, 512, 512, 3, 1, 1), (2, 7, 2048, 512, 1, 1, 0), (3, 30, 32, 64, 3, 2, 1),
    (7, 7, 512, 2048, 1, 1, 0),
]


@pytest.mark.parametrize("Nimg,H,Cin,Cout,k,stride,pad", CONVS)
def test_conv2d_nhwc_under_x6(Nimg, H, Cin, Cout, k, stride, pad):
    eng = engine()
    x = _rand(Nimg, Cin, H, H, seed=7)
    w = _rand(Cout, Cin, k, k, seed=8, scale=(Cin * k * k) ** -0.5)
    b = _rand(Cout, seed=9)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()
    wp = torch.from_numpy(pack_conv_weight(w.numpy())).cuda()
    eng.set_precision("fp32")
    e32 = (eng.op_conv2d_nhwc(x_nhwc, wp, b.cuda(), None, Cout, k, k, stride, pad, act=1).permute(0, 3, 1, 2).cpu().double() - ref).abs()
    eng.set_precision("bf16x6")
    try:
        got = eng.op_conv2d_nhwc(x_nhwc, wp, b.cuda(), None, Cout, k, k, stride, pad, act=1).permute(0, 3, 1, 2)
    finally:
        pass   # the autouse fixture restores the engine's precision
    assert_close(got, ref.float().numpy(), f"x6 conv {Nimg}x{H}x{Cin}->{Cout} k{k}s{stride}")
    e6 = (got.cpu().double() - ref).abs()
    assert e6.mean().item() <= 1.05 * e32.mean().item() + 1e-12 and e6.max().item() <= 1.5 * e32.max().item() + 1e-12


@pytest.mark.parametrize("Nimg,H,Cin,Cout,k,stride,pad", [(2, 28, 32, 64, 7, 2, 3),      # 49 taps: beyond the kernel's 32-tap mask
                                                          (2, 20, 8, 64, 3, 1, 1),       # Cin = 8: no 16-channel chunk
                                                          (2, 12, 16, 64, 5, 2, 2),      # K = 400, packed to 416: neither split form
                                                          (2, 14, 64, 64, 1, 1, 0)])     # (control: this one IS a bf16x6 shape)
def test_conv_geometries_outside_the_x6_kernel_fall_back_to_the_fp32_kernel(Nimg, H, Cin, Cout, k, stride, pad):
    """Round-2 advice: under the default arithmetic relax_op_conv2d_nhwc must keep accepting what the fp32 kernel accepted
    (e.g. a 7x7 filter with Cin % 32 == 0) instead of failing with 'more than 32 taps'."""
    eng = engine()
    assert eng.precision() == "f16x2"      # (the default; convolutions run bf16x6 under it)
    x = _rand(Nimg, Cin, H, H, seed=17)
    w = _rand(Cout, Cin, k, k, seed=18, scale=(Cin * k * k) ** -0.5)
    ref = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad).float().numpy()
    got, n_launch = launches(eng, lambda: eng.op_conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().cuda(), torch.from_numpy(pack_conv_weight(w.numpy())).cuda(),
                                                             None, None, Cout, k, k, stride, pad, act=0).permute(0, 3, 1, 2))
    assert_close(got, ref, f"conv {Cin}->{Cout} k{k} under the default precision")
    want = {0: 0, 3: 1, 7: 0} if k == 1 else {0: 1, 3: 0, 7: 0}     # the control runs bf16x6, the others the exact-fp32 kernel
    assert {kind: n_launch[kind] for kind in want} == want, n_launch


def test_misaligned_operands_are_refused_not_faulted():
    """Round-2 advice: the bf16x6 launcher reads and writes 16-byte units; a view that starts 4 bytes into a buffer must come back
    as RELAX_ERR_INVALID, not as a GPU fault."""
    eng = engine()
    A, W = _rand(64, 64, seed=1).cuda(), _rand(64, 64, seed=2).cuda()
    flat = torch.zeros(64 * 64 + 4, device="cuda")
    skew = flat[1:1 + 64 * 64].view(64, 64)                       # 4-byte offset
    assert skew.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        eng.op_gemm(A, W, out=skew)
    bias = torch.zeros(65, device="cuda")[1:]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        eng.op_gemm(A, W, bias=bias)
    torch.cuda.synchronize()
    assert_close(eng.op_gemm(A, W), (A.double() @ W.double().T).float().cpu().numpy(), "the handle still works")


def test_resnet50_every_tap_under_x6_and_error_against_fp64():
    """All 15 hooked activations + the 13120 / 2051 features on the bf16x6 path: inside the 1e-3 bar against the fp32 oracle;
    and against an fp64 run of the oracle, beside the two fp32 implementations at hand: this library's exact-fp32 MFMA path (an
    fp32 FMA chain, round-to-nearest at every step) and torch's CPU fp32 convolutions (what the reference itself computes
    with).  Measured (norm-relative, per tap, shallow -> deep): FMA chain 1.4e-7 .. 6.8e-7, bf16x6 1.4e-7 .. 9.2e-7, torch CPU
    fp32 2.2e-7 .. 1.3e-6: on every tap bf16x6 is closer to the exact result than the reference's own arithmetic, and within
    1.6x of the FMA chain (the bf16 matrix core aligns the 16 products of an instruction before one rounding, which is not
    unbiased for post-ReLU data: the spatial means keep 5e-7 where the other two keep 2e-7; the largest ratio, 1.56 at
    layer3[0], is an unsplit sum over K = 768 - every tapped launch runs unsplit since its spatial mean is formed in the
    epilogue - where the same tap summed in three K slices measured 1.4).  Bar: 1e-3."""
    sd = rn50_weights()
    eng = engine()
    frags = _fragments(3)
    f = torch.from_numpy(frags).cuda()
    eng.set_precision("fp32")
    ls32, pool32, taps32 = eng.resnet50_features(f, taps=range(15))
    eng.set_precision("bf16x6")
    ls6, pool6, taps6 = eng.resnet50_features(f, taps=range(15))
    ls6b, _ = eng.resnet50_features(f)
    assert torch.equal(ls6, ls6b), "bf16x6 ResNet-50 is not deterministic"
    tsd = resnet50_ref.to_torch_state_dict(sd)
    ref_taps, _ = resnet50_ref.forward_taps(tsd, resnet50_ref.preprocess_bgr_u8(frags))
    sd64 = {k: v.double() for k, v in tsd.items()}
    ref64, avg64 = resnet50_ref.forward_taps(sd64, resnet50_ref.preprocess_bgr_u8(frags).double())

    def rel(a, r):
        return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - r) / np.linalg.norm(r))

    for i, name in enumerate(pooling_ref.RESNET50_TAPS):
        assert_close(taps6[i], ref_taps[name].numpy(), f"x6 {name}")
        r = ref64[name].numpy()
        n32, n6, ncpu = rel(taps32[i].cpu().numpy(), r), rel(taps6[i].cpu().numpy(), r), rel(ref_taps[name].numpy(), r)
        print(f"{name:22s} vs fp64: fp32 MFMA path {n32:.3e}  bf16x6 {n6:.3e}  torch CPU fp32 {ncpu:.3e}")
        assert n6 <= ncpu and n6 <= 1.6 * n32, name    # closer to exact than the reference's own fp32 arithmetic, on every tap
    want_ls = resnet50_ref.layer_stack_features(tsd, frags)
    want_pool = resnet50_ref.pool_features(tsd, frags)
    assert_close(ls6, want_ls, "x6 layer-stack")
    assert_close(pool6, want_pool, "x6 pool")
    ls64 = torch.cat([t.mean(dim=(2, 3)) for t in ref64.values()], dim=1).numpy()
    n32, n6, ncpu = rel(ls32.cpu().numpy(), ls64), rel(ls6.cpu().numpy(), ls64), rel(want_ls, ls64)
    print(f"layer-stack 13120 vs fp64: fp32 MFMA path {n32:.3e}  bf16x6 {n6:.3e}  torch CPU fp32 {ncpu:.3e}")
    assert n6 < 1e-6      # the spatial means keep the (small) bias of the matrix core's product alignment: measured 5e-7


@pytest.mark.parametrize("n_img,heads,scale", [(1, 3, 1.0), (3, 12, 1.0), (2, 6, 4.0), (40, 12, 2.0)])
def test_attention_under_x6(n_img, heads, scale):
    """softmax(q k^T / 8) v with both contractions on split planes (csrc/attention_x6.hip) against fp64, beside the fp32-MFMA
    attention kernel; scale 4 makes logits of +-60 (near one-hot rows); 40 images x 12 heads = 480 items > 256 workgroups
    exercises the persistent loop (K of the next item prefetched under the output phase)."""
    eng = engine()
    dim = heads * 64
    qkv = _rand(n_img * 197, 3 * dim, seed=17, scale=scale)
    t = qkv.double().reshape(n_img, 197, 3, heads, 64).permute(2, 0, 3, 1, 4)
    attn = ((t[0] @ t[1].transpose(-2, -1)) * 64 ** -0.5).softmax(dim=-1)
    ref = (attn @ t[2]).transpose(1, 2).reshape(n_img * 197, dim)
    eng.set_precision("fp32")
    e32 = (eng.op_attention(qkv.cuda(), n_img, heads).cpu().double() - ref).abs()
    eng.set_precision("bf16x6")
    got = eng.op_attention(qkv.cuda(), n_img, heads)
    again = eng.op_attention(qkv.cuda(), n_img, heads)
    assert torch.equal(got, again)
    assert_close(got, ref.float().numpy(), f"x6 attention n={n_img} heads={heads}")
    e6 = (got.cpu().double() - ref).abs()
    print(f"\nattention {n_img}x{heads} scale {scale}: mean err fp32 {e32.mean().item():.3e} x6 {e6.mean().item():.3e}; max fp32 {e32.max().item():.3e} x6 {e6.max().item():.3e}")
    assert e6.mean().item() <= 1.25 * e32.mean().item() + 1e-12 and e6.max().item() <= 2.0 * e32.max().item() + 1e-12
