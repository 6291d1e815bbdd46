"""f16x2 - the default arithmetic - on random shapes and contents (hypothesis, derandomized), under the fp32-grade gate of
tests/fp32_grade.py: error against fp64, measured against the sum of magnitudes, no larger than the exact-fp32 path's on the same
inputs.  Every test checks through the profile counters that the kernel it means to test ran:

  * op_gemm: gemm_h3 / gemm_h2 (read kind 9), every h2_form, the 16-k form that K % 32 == 16 takes on its own, the four-product form
    below K = 256, the tail split-K (splitk_finish_h2); per-row scales on rows 2^-30 .. 2^30 apart, values 2^-12 .. 2^0 apart inside
    a row, all-zero and single-nonzero rows;
  * op_conv2d_nhwc: the wide gemm_h3 form (Cout % 256 == 0) and the narrow gemm_x6<H2> form (64 / 128 / 192 columns) with one scale
    per IMAGE (kind 7 minus kind 9); non-square maps, images on both sides of the 256-row tile (one image per tile: one scale; the
    `two_sc` path of gemm_x6.hip), batch invariance; rn_h2_early = 0 sends the narrow form to bf16x6 (kind 3);
  * op_attention: attention_h2 (att_h2 = 1) and attention_x6 under f16x2 (att_h2 = 0).

The fp64 references run on the device (torch's fp64 matmul, not the project's kernels).  Each example prints its gate ratios
(`GATE <what> mean e / mean e32, max e / max e32`)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from relax_vqa_amd.engine import pack_conv_weight
from tests import fp32_grade
from tests.gpu_common import engine, exact_fp32_gemm, launches

pytestmark = pytest.mark.gpu
COMMON = dict(deadline=None, derandomize=True, database=None, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])

FAMILIES = ["normal", "rows_2^-30..2^30", "in_row_2^-12..2^0", "zero_rows", "single_nonzero_rows"]


def _record(what, ratios):
    print(f"\nGATE {what}: mean e / mean e32 {ratios[0]:.3f}, max e / max e32 {ratios[1]:.3f}, max e {ratios[2]:.3e}")


def _act64(y, act):
    return [y, F.relu(y), F.gelu(y)][act]


def _gemm_operands(g, family, M, N, K):
    """A [M, K] of the family, W [N, K], and each row's size (residuals follow it, so that they do not hide the product)."""
    A = g.standard_normal((M, K))
    row = np.ones(M)
    if family == "rows_2^-30..2^30":
        row = np.exp2(g.integers(-30, 31, M).astype(np.float64))
        A *= row[:, None]
    elif family == "in_row_2^-12..2^0":
        A *= np.exp2(g.integers(-12, 1, (M, K)).astype(np.float64))
    elif family in ("zero_rows", "single_nonzero_rows"):
        rows = np.flatnonzero(g.random(M) < 0.3)
        A[rows] = 0
        if family == "single_nonzero_rows":
            A[rows, g.integers(0, K, rows.size)] = g.standard_normal(rows.size) * np.exp2(g.integers(-20, 21, rows.size).astype(np.float64))
    W = g.standard_normal((N, K)) * K ** -0.5
    if family == "in_row_2^-12..2^0":
        W *= np.exp2(g.integers(-8, 1, (N, K)).astype(np.float64))
    return torch.from_numpy(A.astype(np.float32)), torch.from_numpy(W.astype(np.float32)), row


K_WEIGHTED = st.one_of(st.sampled_from([16, 48, 240, 256, 272, 752, 768, 784]), st.integers(1, 288).map(lambda j: 16 * j))


@settings(max_examples=70, **COMMON)
@given(m=st.integers(1, 1500), big=st.integers(0, 11), n=st.sampled_from([256, 512, 768, 1024, 2304, 3072]), k=K_WEIGHTED,
       act=st.sampled_from([0, 1, 2]), with_bias=st.booleans(), res=st.sampled_from(["none", "residual", "in_place"]),
       form=st.sampled_from([1, 1, 0, 2]), family=st.sampled_from(FAMILIES), seed=st.integers(0, 2 ** 31 - 1))
def test_f16x2_gemm_on_random_shapes(m, big, n, k, act, with_bias, res, form, family, seed):
    """out = act(A W^T + bias + residual) under f16x2 against fp64: the gate; the same bits run to run; with the tail split off, a
    random window of rows has the same bits alone; the 3- and 4-stage forms of the 16-k loop give the same bits."""
    if big == 0:        # one draw in twelve: more than 256 tiles of 256 x 256 (more tiles than CUs, and a real tail)
        n = max(n, 2304)
        m = (256 * 256 // (n // 256) // 256 + 1) * 256 + m % 256
        k = min(k, 1024)
    g = np.random.default_rng(seed)
    A, W, row = _gemm_operands(g, family, m, n, k)
    b = torch.from_numpy(g.standard_normal(n).astype(np.float32)) if with_bias else None
    r = torch.from_numpy((g.standard_normal((m, n)) * row[:, None]).astype(np.float32)) if res != "none" else None
    Ad, Wd = A.cuda(), W.cuda()
    bd = b.cuda() if with_bias else None
    rd = r.cuda() if r is not None else None
    y = Ad.double() @ Wd.double().T
    mag = Ad.double().abs() @ Wd.double().abs().T
    if with_bias:
        y, mag = y + bd.double(), mag + bd.double().abs()
    if r is not None:
        y, mag = y + rd.double(), mag + rd.double().abs()
    ref = _act64(y, act).cpu().numpy()
    mag = mag.cpu().numpy() + fp32_grade.h2_floor(A.abs().amax(dim=1).numpy(), W.abs().amax(dim=1).numpy())
    del y

    eng = engine()
    assert eng.precision() == "f16x2"
    got32 = exact_fp32_gemm(eng, Ad, Wd, bd, rd, act).cpu().numpy()

    def run():
        if res == "in_place":
            rr = rd.clone()
            eng.op_gemm(Ad, Wd, bd, rr, act=act, out=rr)
            return rr
        return eng.op_gemm(Ad, Wd, bd, rd, act=act)

    eng.set_option("h2_form", form)
    try:
        got, n_launch = launches(eng, run)
        assert n_launch[9] >= 1 and n_launch[3] == 0 and n_launch[0] == 0, f"not the f16x2 GEMM: {n_launch}"
        assert torch.equal(got, run()), "f16x2 GEMM is not deterministic"
        what = f"f16x2 gemm {m}x{n}x{k} form{form} act{act} bias{with_bias} {res} {family}"
        _record(what, fp32_grade.check(got.cpu().numpy(), got32, ref, mag, what, slack=fp32_grade.SLACK + fp32_grade.h2_slack(1 if family == "single_nonzero_rows" else k)))
        if form == 0 or k % 32:         # the 16-k form: 3 (default) or 4 LDS stages, the same products in the same order
            eng.set_option("h2_stages", 4)
            try:
                assert torch.equal(got, run()), "h2_stages 3 and 4 differ"
            finally:
                eng.set_option("h2_stages", 3)
        eng.set_option("gemm_split_k", 0)
        try:
            whole = eng.op_gemm(Ad, Wd, bd, rd, act=act)
            r0 = int(g.integers(0, m))
            r1 = int(g.integers(r0 + 1, m + 1))
            part = eng.op_gemm(Ad[r0:r1].contiguous(), Wd, bd, rd[r0:r1].contiguous() if rd is not None else None, act=act)
        finally:
            eng.set_option("gemm_split_k", 1)
        assert torch.equal(whole[r0:r1], part), f"rows {r0}:{r1} of {m} depend on the batch"
    finally:
        eng.set_option("h2_form", 1)


# ---- convolutions ---------------------------------------------------------------------------------------------------------
WIDE_GEOMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)]                # (k, stride, pad) of the gemm_h3 form
NARROW_FILTERS = [(3, 32), (3, 64), (3, 128), (4, 16), (4, 32), (2, 64)]   # (k, Cin): k k Cin % 32 == 0 and >= 256


def _conv64(x, w, stride, pad):
    """fp64 convolution on the device as im2col + matmul: x [N, C, H, W], w [Cout, C, k, k] -> [N, Cout, L]."""
    cols = F.unfold(x, w.shape[2], padding=pad, stride=stride)
    return w.reshape(w.shape[0], -1) @ cols


@settings(max_examples=60, **COMMON)
@given(data=st.data(), form=st.sampled_from(["wide", "narrow"]), nimg=st.integers(1, 40), act=st.sampled_from([0, 1, 2]),
       with_res=st.booleans(), with_bias=st.booleans(), zero_img=st.booleans(), early=st.sampled_from([1, 1, 1, 0]),
       seed=st.integers(0, 2 ** 31 - 1))
def test_f16x2_conv_on_random_geometries(data, form, nimg, act, with_res, with_bias, zero_img, early, seed):
    """op_conv2d_nhwc under f16x2, both forms, one scale per image (each image x 2^-12 .. 2^12, possibly one all-zero image): the gate
    PER IMAGE (that image's own sum of magnitudes); with the tail split off every image's bits are the same alone and in the reversed
    batch - the check on the row -> image lookups (img_of_row, two_sc)."""
    if form == "wide":
        cin = data.draw(st.sampled_from([32, 64, 128, 256]), "cin")
        cout = data.draw(st.sampled_from([256, 512]), "cout")
        k, stride, pad = data.draw(st.sampled_from(WIDE_GEOMS), "geom")
    else:
        cout = data.draw(st.sampled_from([64, 128, 192]), "cout")
        k, cin = data.draw(st.sampled_from(NARROW_FILTERS), "filter")
        stride = data.draw(st.sampled_from([1, 2]), "stride")
        pad = data.draw(st.sampled_from([0, k // 2]), "pad")
    lo = max(3, k - 2 * pad)
    h = data.draw(st.integers(lo, 40), "h")
    w = data.draw(st.integers(lo, 40), "w")
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    nimg = max(1, min(nimg, 3_000_000 // (ho * wo * cout)))      # (the gate runs on the host: at most ~3M outputs per example)
    g = np.random.default_rng(seed)
    sc = np.exp2(g.integers(-12, 13, nimg).astype(np.float64))
    if zero_img and nimg > 1:
        sc[g.integers(0, nimg)] = 0.0
    x = torch.from_numpy((g.standard_normal((nimg, cin, h, w)) * sc[:, None, None, None]).astype(np.float32)).cuda()
    wt = torch.from_numpy((g.standard_normal((cout, cin, k, k)) * (cin * k * k) ** -0.5).astype(np.float32)).cuda()
    b = torch.from_numpy((g.standard_normal(cout) * 2.0 ** -6).astype(np.float32)).cuda() if with_bias else None
    res = torch.from_numpy((g.standard_normal((nimg, cout, ho, wo)) * sc[:, None, None, None]).astype(np.float32)).cuda() if with_res else None
    y = _conv64(x.double(), wt.double(), stride, pad)
    mag = _conv64(x.double().abs(), wt.double().abs(), stride, pad)
    if with_bias:
        y, mag = y + b.double()[None, :, None], mag + b.double().abs()[None, :, None]
    if with_res:
        y, mag = y + res.double().reshape(nimg, cout, -1), mag + res.double().abs().reshape(nimg, cout, -1)
    ref = _act64(y, act).cpu().numpy()
    mag = mag.cpu().numpy()
    del y

    eng = engine()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous()
    r_nhwc = res.permute(0, 2, 3, 1).contiguous() if with_res else None
    wp = torch.from_numpy(pack_conv_weight(wt.cpu().numpy())).cuda()
    assert wp.shape[1] == k * k * cin, "the geometry must not need K padding (the f16x2 forms refuse it)"

    def conv(xx, rr):
        return eng.op_conv2d_nhwc(xx, wp, b, rr, cout, k, k, stride, pad, act=act)

    def flat(o):        # NHWC -> [N, Cout, L], the layout of the reference
        return o.permute(0, 3, 1, 2).reshape(o.shape[0], cout, -1).cpu().numpy()

    eng.set_precision("fp32")
    got32 = flat(conv(x_nhwc, r_nhwc))
    eng.set_precision("f16x2")
    eng.set_option("rn_h2_early", early)
    try:
        got, n_launch = launches(eng, lambda: conv(x_nhwc, r_nhwc))
        if form == "narrow" and not early:
            assert n_launch[3] >= 1 and n_launch[7] == 0, f"rn_h2_early = 0: the narrow form must run bf16x6: {n_launch}"
        else:
            assert n_launch[7] - n_launch[9] >= 1 and n_launch[9] == 0 and n_launch[3] == 0 and n_launch[0] == 0, \
                f"not the f16x2 convolution: {n_launch}"
        assert torch.equal(got, conv(x_nhwc, r_nhwc)), "not deterministic"
        gf = flat(got)
        worst = (0.0, 0.0, 0.0)
        for i in range(nimg):
            what = (f"{'bf16x6' if form == 'narrow' and not early else 'f16x2'} conv {form} image {i} (x {sc[i]:g}) of {nimg}x{h}x{w}x{cin}"
                    f"->{cout} k{k}s{stride}p{pad} act{act} res{with_res} bias{with_bias}")
            ratios = fp32_grade.check(gf[i], got32[i], ref[i], mag[i], what, slack=fp32_grade.SLACK + fp32_grade.h2_slack(k * k * cin))
            worst = tuple(max(a, c) for a, c in zip(worst, ratios))
        _record(f"conv {form} early{early} {nimg}x{h}x{w}x{cin}->{cout} k{k}s{stride} rows/img {ho * wo} (worst image)", worst)
        eng.set_option("gemm_split_k", 0)
        try:
            whole = conv(x_nhwc, r_nhwc)
            i = int(g.integers(0, nimg))
            alone = conv(x_nhwc[i:i + 1].contiguous(), r_nhwc[i:i + 1].contiguous() if with_res else None)
            rev = conv(x_nhwc.flip(0).contiguous(), r_nhwc.flip(0).contiguous() if with_res else None)
        finally:
            eng.set_option("gemm_split_k", 1)
        assert torch.equal(whole[i], alone[0]), f"image {i} of {nimg} differs when it runs alone"
        for j in range(nimg):
            assert torch.equal(whole[j], rev[nimg - 1 - j]), f"image {j} of {nimg} differs in the reversed batch"
    finally:
        eng.set_option("rn_h2_early", 1)


# ---- attention ------------------------------------------------------------------------------------------------------------
@settings(max_examples=30, **COMMON)
@given(n_img=st.integers(1, 45), heads=st.sampled_from([1, 3, 6, 12]), scale=st.floats(0.02, 5.0), outlier=st.booleans(),
       att_h2=st.sampled_from([1, 1, 0]), seed=st.integers(0, 2 ** 31 - 1))
def test_f16x2_attention_on_random_inputs(n_img, heads, scale, outlier, att_h2, seed):
    """softmax(q k^T / 8) v under f16x2 against fp64 and beside the exact-fp32 path, error normalised by the max |v| of each (image,
    head).  The operator entry takes ONE scale from the whole qkv tensor (csrc/h2.h): the magnitudes of a call stay comparable - the
    outlier rows are the 6x of tests/test_gpu_random_cases.py.  n_img = 45 with 12 heads passes the persistent loop's 256 workgroups."""
    g = np.random.default_rng(seed)
    dim = heads * 64
    qkv = torch.from_numpy((g.standard_normal((n_img * 197, 3 * dim)) * scale).astype(np.float32))
    if outlier:
        qkv[int(g.integers(0, n_img * 197)), :dim] *= 6.0
        qkv[int(g.integers(0, n_img * 197)), dim:2 * dim] *= 6.0
    qkv = qkv.cuda()
    t = qkv.double().reshape(n_img, 197, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref = (((t[0] @ t[1].transpose(-2, -1)) * 64 ** -0.5).softmax(dim=-1) @ t[2]).transpose(1, 2).reshape(n_img * 197, dim).cpu().numpy()
    mag = fp32_grade.attention_mag(t[2].abs().amax(dim=(2, 3)).cpu().numpy(), 197)
    eng = engine()
    eng.set_precision("fp32")
    got32 = eng.op_attention(qkv, n_img, heads).cpu().numpy()
    eng.set_precision("f16x2")
    eng.set_option("att_h2", att_h2)
    try:
        assert eng.precision() == "f16x2" and eng.get_option("att_h2") == att_h2     # (attention has no profile counter)
        got = eng.op_attention(qkv, n_img, heads)
        assert torch.equal(got, eng.op_attention(qkv, n_img, heads)), "not deterministic"
    finally:
        eng.set_option("att_h2", 1)
    what = f"attention {'attention_h2' if att_h2 else 'attention_x6'} n={n_img} heads={heads} scale={scale:.3f} outlier={outlier}"
    _record(what, fp32_grade.check(got.cpu().numpy(), got32, ref, mag, what, slack=fp32_grade.SLACK + fp32_grade.h2_slack(64), max_abs=None))
