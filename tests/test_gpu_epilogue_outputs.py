"""The outputs of the convolution epilogues that only the model drivers use, at operator level (RelaxEngine.op_conv2d_nhwc_ex,
op_bn_relu_maxpool with amax_out): the per-image maxima (amax_out) the f16x2 scales are derived from, the outputs as fp16 planes, the
residual read as planes, the first stage of the fused spatial mean, the back-to-back conv2 -> conv3 launch.

Every check relates two outputs of the SAME launch, two launches that must give the same bits, or a launch to the numpy restatement
of a documented rounding rule (tests/h2_restated.py, anchored by tests/test_h2_restated_cpu.py): exact, or under a derived bound.  The
fp32 `out` itself is gated against fp64 by tests/test_gpu_h2_random.py and tests/test_gpu_h2.py.

  (a) planted maxima: amax_out[i] == bits of out[i].max() of the same launch, with the maximum of one image planted at the first /
      last row of the image, on either side of a row-tile boundary inside it, at the last row of M, at the first / last column and on
      either side of a column-tile boundary - by one large fp32 residual entry, and (1x1) by an input pixel scaled by 64; the other
      images' maxima keep their bits; in the reversed batch every maximum follows its image
  (b) zeros of either sign: an image whose pre-activations are all negative, an all-zero image (+0.0 and -0.0) with zero bias (+0.0
      and -0.0): amax_out == 0x00000000 - a single -0.0 output (bits 0x80000000) would win every integer maximum
  (c) the plane output == split2 of the launch's own fp32 out, as uint16, with a caller-made power-of-two scale per image
  (d) a residual given as planes == the same launch given the fp32 residual (hi + lo) * inv, bit for bit
  (e) group sums against the fp64 sums of the launch's own out: |error| <= g 2^-24 sum |x| (g fp32 additions in any order, first
      order); with out_rows / gap_rows below M the rest keeps a sentinel and the part below the limits has the bits of the unrestricted launch
  (f) the stem (bn_relu_maxpool): bits of y.max() per image, planted at the four corners and in the last channel, an all-zero image

Which kernel ran: every f16x2 convolution launch - gemm_h3's convolution form, gemm_x6<H2>, the back-to-back form - is one span of
read kind 7 that is not of kind 9 (kind 9 counts the plain GEMMs alone, csrc/api.hip), so each test asserts exactly its number of
launches there and none on any other contraction kernel; WHICH of the forms it is follows from the dispatch rule the entry shares
with relax_op_conv2d_nhwc (Cout % 256 == 0: gemm_h3).  The split-K finish has no counter: the cases meant to reach it assert that the
launch's fp32 bits differ from the unsplit launch's (the K sums were cut), after which its maxima are checked like any other.

The maxima-posting sites and the fixed cases that reach them (rows per image r, rows M):
  gemm_h3 epilogue, global atomics (r < 18)        wide r = 1, 4, 9, 16 with gemm_split_k 0 (and with 1 where K < 256)
  gemm_h3 epilogue, LDS table `simg`               wide r = 49, 196, 784 with gemm_split_k 0
  splitk_finish_h2, `s_mx`                         wide with gemm_split_k 1 and K >= 256 (every tile of these small problems is tail)
  gemm_x6<H2> per-tile LDS path / global atomics   narrow r = 49, 196 / r = 1 .. 16
  gemm_x6<H2> `two_img`                            narrow r = 784
  back-to-back form, two slots per tile            b2b cases (r = 784), b2b_rows 256 and 128
  bn_relu_maxpool block maxima                     test_stem_maxima

Refused combinations (asserted in test_refusals; none is a ResNet-50 / VGG-16 layer geometry): amax_out with act != 1; a narrow-form
plane output with act != 1; the fused mean with Ho*Wo % 4 != 0; a plane residual on the narrow form, or together with an fp32
residual; the back-to-back form with Ho*Wo < 256, with Ho*Wo % 16 != 0, without a residual, or onto Cout other than 64 / 128; a
geometry with no f16x2 form; a stem map without whole blocks per image."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from hypothesis import given, settings
from hypothesis import strategies as st

from relax_vqa_amd.engine import pack_conv_weight
from tests import h2_restated
from tests.gpu_common import engine, launches
from tests.test_gpu_h2_random import COMMON, NARROW_FILTERS, WIDE_GEOMS, _conv64

pytestmark = pytest.mark.gpu

HOWO = {1: (1, 1), 4: (2, 2), 9: (3, 3), 16: (4, 4), 49: (7, 7), 196: (14, 14), 784: (28, 28)}
NIMG = [1, 2, 7, 23, 37]
SENTINEL = 0x7FC0DEAD          # a NaN pattern no kernel produces
PLANT = 5000.0                 # far above every output of these inputs (|out| < 2^4 x a few sigma)
MAX_OUTPUTS = 5_000_000

# form: wide (gemm_h3) | narrow (gemm_x6<H2>) | b2b (3x3 + 1x1 back to back); r = Ho*Wo; cout3 / b2b_rows: b2b only
Case = namedtuple("Case", "form r nimg cin cout k stride pad cout3 b2b_rows")


def _wide(r, nimg, cin, cout, geom):
    return Case("wide", r, nimg, cin, cout, *WIDE_GEOMS[geom], 0, 256)


def _narrow(r, nimg, cout, filt, stride, padded):
    k, cin = NARROW_FILTERS[filt]
    return Case("narrow", r, nimg, cin, cout, k, stride, k // 2 if padded else 0, 0, 256)


# Every value of the lists at least once, every r on both forms, the small maps with more than 16 images (r < 18 cannot use the 16-slot LDS
# table), r = 49 with 5 - 6 images per tile, r = 196 straddling, r = 784 several tiles per image; M ragged against 256 and 128
WIDE_CASES = [
    _wide(1, 37, 256, 256, 0), _wide(1, 1, 32, 256, 0), _wide(4, 23, 64, 512, 2), _wide(9, 37, 32, 256, 3), _wide(16, 23, 256, 512, 1),
    _wide(49, 7, 64, 256, 2), _wide(49, 23, 32, 512, 0), _wide(196, 2, 256, 256, 0), _wide(196, 7, 64, 512, 3), _wide(784, 1, 32, 256, 0),
    _wide(784, 2, 256, 512, 2), _wide(196, 37, 64, 256, 1),
]
NARROW_CASES = [
    _narrow(1, 37, 64, 0, 1, True), _narrow(4, 23, 128, 1, 2, True), _narrow(9, 7, 192, 2, 1, True), _narrow(16, 37, 64, 3, 1, True),
    _narrow(49, 23, 128, 4, 1, False), _narrow(196, 2, 192, 5, 1, False), _narrow(196, 7, 64, 1, 2, True), _narrow(784, 2, 128, 0, 1, True),
    _narrow(784, 7, 64, 3, 2, True), _narrow(784, 1, 192, 1, 1, True),
]
B2B_CASES = [Case("b2b", 784, n, c, c, 3, 1, 1, c3, rows) for (c, c3) in ((64, 256), (128, 512)) for rows in (256, 128)
             for n in ((1, 7) if c == 64 else (2,))]
CASES = WIDE_CASES + NARROW_CASES + B2B_CASES


def _id(c):
    return f"{c.form}-r{c.r}-n{c.nimg}-{c.cin}to{c.cout}{'to%d' % c.cout3 if c.cout3 else ''}-k{c.k}s{c.stride}p{c.pad}" + \
        (f"-rows{c.b2b_rows}" if c.form == "b2b" else "")


def _in_size(o, k, stride, pad):
    for h in range(1, 80):
        if h + 2 * pad >= k and (h + 2 * pad - k) // stride + 1 == o:
            return h
    raise AssertionError("no input size for this output size")


def _has_in_size(o, k, stride, pad):
    return any(h + 2 * pad >= k and (h + 2 * pad - k) // stride + 1 == o for h in range(1, 80))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _img_max_bits(out, nimg):
    return _bits(out.reshape(nimg, -1).amax(dim=1))


@functools.lru_cache(maxsize=None)
def _inputs(case, seed=0):
    """The operands of a case (made once, shared by its tests, never modified) and the per-image maxima of its fp64 reference."""
    c = case
    g = np.random.default_rng([seed, c.r, c.nimg, c.cin, c.cout, c.k, c.stride, c.pad, c.cout3])
    ho, wo = HOWO[c.r]
    h, w = _in_size(ho, c.k, c.stride, c.pad), _in_size(wo, c.k, c.stride, c.pad)
    cn = c.cout3 or c.cout
    assert c.nimg * c.r * cn <= MAX_OUTPUTS
    sc = np.exp2(g.integers(-4, 5, c.nimg).astype(np.float64))[:, None, None, None]
    x = torch.from_numpy((g.standard_normal((c.nimg, c.cin, h, w)) * sc).astype(np.float32)).cuda()
    wt = torch.from_numpy((g.standard_normal((c.cout, c.cin, c.k, c.k)) * (c.cin * c.k * c.k) ** -0.5).astype(np.float32)).cuda()
    d = dict(case=c, ho=ho, wo=wo, h=h, w=w, cn=cn, M=c.nimg * c.r, g=g,
             x=x.permute(0, 2, 3, 1).contiguous(), wp=torch.from_numpy(pack_conv_weight(wt.cpu().numpy())).cuda(),
             bias=torch.from_numpy((g.standard_normal(c.cout) * 0.25).astype(np.float32)).cuda(),
             res=torch.from_numpy((g.standard_normal((c.nimg, ho, wo, cn)) * sc.reshape(-1, 1, 1, 1)).astype(np.float32)).cuda(), w3=None, bias3=None)
    y = _conv64(x.double(), wt.double(), c.stride, c.pad) + d["bias"].double()[None, :, None]          # [N, Cout, L]
    if c.form == "b2b":
        d["w3"] = torch.from_numpy((g.standard_normal((cn, c.cout)) * c.cout ** -0.5).astype(np.float32)).cuda()
        d["bias3"] = torch.from_numpy((g.standard_normal(cn) * 0.25).astype(np.float32)).cuda()
        y = d["w3"].double() @ F.relu(y) + d["bias3"].double()[None, :, None]
    d["y64"] = y.permute(0, 2, 1).contiguous()                                                       # [N, L, Cn], before residual / ReLU
    return d


def _tile(c):
    """(rows, columns) of an output tile: where the row -> image lookups and the per-tile reductions have their seams."""
    if c.form == "wide":
        return 256, 256
    if c.form == "b2b":
        return (c.b2b_rows if c.cout == 64 else 256), 64
    return 256, (128 if c.cout % 128 == 0 else 64)


class _Runner:
    """Launches of one case, each checked through the profile counters: one f16x2 convolution span per launch, nothing else."""

    def __init__(self, inp, split):
        self.inp, self.eng, self.split = inp, engine(), split

    def __enter__(self):
        assert self.eng.precision() == "f16x2"
        self.eng.set_option("gemm_split_k", self.split)
        self.eng.set_option("b2b_rows", self.inp["case"].b2b_rows)
        return self

    def __exit__(self, *exc):
        self.eng.set_option("gemm_split_k", 1)
        self.eng.set_option("b2b_rows", 256)

    def __call__(self, x=None, bias="case", residual="case", act=1, **kw):
        i, c = self.inp, self.inp["case"]
        bias = i["bias"] if isinstance(bias, str) else bias
        residual = i["res"] if isinstance(residual, str) else residual
        got, n = launches(self.eng, lambda: self.eng.op_conv2d_nhwc_ex(
            i["x"] if x is None else x, i["wp"], bias, c.cout, c.k, c.k, c.stride, c.pad, act=act, residual=residual, w3=i["w3"], bias3=i["bias3"], **kw))
        assert n[7] - n[9] == 1 and n[9] == 0 and n[3] == 0 and n[0] == 0, f"not exactly one f16x2 convolution launch: {n}"
        return got


def _plant_positions(c, M):
    """(image, row inside the image, column) of each position class, rows and columns paired round robin."""
    bm, bn = _tile(c)
    cn = c.cout3 or c.cout
    t = c.nimg // 2                                   # the chosen image
    rows = [(t, 0), (t, c.r - 1), (c.nimg - 1, c.r - 1)]            # first / last row of the image, last row of M
    for b in range(bm, M, bm):                        # the rows on either side of the first and last tile boundaries strictly inside an image
        if b % c.r:
            rows += [((b - 1) // c.r, (b - 1) % c.r), (b // c.r, b % c.r)]
            break
    for b in range(((M - 1) // bm) * bm, 0, -bm):
        if b % c.r:
            rows += [((b - 1) // c.r, (b - 1) % c.r), (b // c.r, b % c.r)]
            break
    cols = [0, cn - 1] + ([bn - 1, bn] if cn > bn else []) + ([cn - bn - 1, cn - bn] if cn > 2 * bn else [])
    n = max(len(rows), len(cols))
    return [(*rows[j % len(rows)], cols[j % len(cols)]) for j in range(n)]


def _check_maxima(got, nimg, what):
    want = _img_max_bits(got["out"], nimg)
    assert torch.equal(got["amax"], want), (f"{what}: amax_out differs from the bits of out.max() at images "
                                            f"{torch.nonzero(got['amax'] != want).flatten().tolist()[:8]}: "
                                            f"{[hex(v & 0xFFFFFFFF) for v in got['amax'][got['amax'] != want].tolist()[:8]]}")
    return want


def _planted_maxima(inp, split, positions, input_plant=True):
    c, M = inp["case"], inp["M"]
    with _Runner(inp, split) as run:
        base = run(amax=True)
        base_max = _check_maxima(base, c.nimg, "no plant")
        assert float(base["out"].max()) < PLANT / 8
        for (img, row, col) in positions:
            res = inp["res"].clone()
            res.view(c.nimg, c.r, -1)[img, row, col] = PLANT
            got = run(residual=res, amax=True)
            mx = _check_maxima(got, c.nimg, f"plant at image {img} row {row} column {col}")
            flat = got["out"].view(c.nimg, c.r, -1)[img]
            assert int(flat.argmax()) == row * flat.shape[1] + col and float(flat.max()) > PLANT / 2, "the plant is not the image's maximum"
            others = torch.arange(c.nimg, device=mx.device) != img
            assert torch.equal(mx[others], base_max[others]), f"plant in image {img}: another image's maximum moved"
        if input_plant and c.form == "wide" and c.k == 1:          # no residual: one input pixel x 64 (the output row of a 1x1 follows it)
            plain = _check_maxima(run(residual=None, amax=True), c.nimg, "no residual")
            for (img, row, _) in positions[:3]:
                x = inp["x"].clone()
                oy, ox = divmod(row, inp["wo"])
                x[img, oy * c.stride, ox * c.stride] *= 64.0
                got = run(x=x, residual=None, amax=True)
                mx = _check_maxima(got, c.nimg, f"input pixel of image {img} row {row} x 64")
                assert int(got["out"].view(c.nimg, c.r, -1)[img].amax(dim=1).argmax()) == row, "the scaled pixel's row does not hold the maximum"
                others = torch.arange(c.nimg, device=mx.device) != img
                assert torch.equal(mx[others], plain[others]), "another image's maximum moved"
        # the reversed batch: every maximum is that of its own launch, and - the K sums not depending on the position: tail split off -
        # follows its image bit for bit
        rev = run(x=inp["x"].flip(0).contiguous(), residual=inp["res"].flip(0).contiguous(), amax=True)
        mx = _check_maxima(rev, c.nimg, "reversed batch")
        if not split:
            assert torch.equal(mx.flip(0), base_max), "a maximum does not follow its image into the reversed batch"
    return base


def _zero_maxima(inp, split):
    c = inp["case"]
    if c.nimg < 2:
        return
    a, z = c.nimg // 2, (c.nimg // 2 + 1) % c.nimg
    wp = inp["wp"].abs()
    with _Runner(dict(inp, wp=wp, w3=inp["w3"].abs() if c.form == "b2b" else None), split) as run:
        # b2b: relu(conv2) >= 0 times w3 >= 0 is >= 0 whatever the input, so the negative image comes from conv3's bias and residual
        for sign in (1.0, -1.0):
            run.inp["wp"] = wp * sign
            x = inp["x"].clone()
            x[a] = -sign * x[a].abs()
            x[z] = 0.0
            x[z].view(-1)[1::2] = -0.0
            assert bool((_bits(x[z]) < 0).any()), "-0.0 inputs are meant"
            bias = torch.full_like(inp["bias"], -1.0)
            if c.form == "b2b":
                res = torch.zeros_like(inp["res"])
                res[a] = -1e6
                run.inp["bias3"] = torch.zeros_like(inp["bias3"])
                got = run(x=x, bias=bias, residual=res, amax=True)
            else:
                got = run(x=x, bias=bias, residual=None, amax=True)
            mx = _check_maxima(got, c.nimg, f"negative image, weights x {sign:+.0f}")
            assert int(mx[a]) == 0 and int(mx[z]) == 0, f"all-negative pre-activations: maxima {hex(int(mx[a]) & 0xFFFFFFFF)}, {hex(int(mx[z]) & 0xFFFFFFFF)}"
            assert not bool(_bits(got["out"][a]).any()) and not bool(_bits(got["out"][z]).any()), "an output of a negative image is not +0.0"
            # zero bias of either sign: the all-zero image's outputs are +0.0 and its maximum 0x00000000
            zb = torch.zeros_like(inp["bias"])
            zb[1::2] = -0.0
            if c.form == "b2b":
                zb3 = torch.zeros_like(inp["bias3"])
                zb3[1::2] = -0.0
                run.inp["bias3"] = zb3
                res = torch.zeros_like(inp["res"])
                res[z].view(-1)[::3] = -0.0
                got = run(x=x, bias=zb, residual=res, amax=True)
            else:
                got = run(x=x, bias=zb, residual=None, amax=True)
            mx = _check_maxima(got, c.nimg, f"zero image, weights x {sign:+.0f}")
            assert int(mx[z]) == 0, f"all-zero image: maximum {hex(int(mx[z]) & 0xFFFFFFFF)}"
            assert not bool(_bits(got["out"][z]).any()), "an output of the all-zero image is not +0.0"
            assert bool((mx[torch.arange(c.nimg, device=mx.device) != z] >= 0).all())


def _out_scales(inp):
    """Per image the power of two that puts TWICE the maximum of the fp64 reference (residual added, ReLU) into [2^14, 2^15)."""
    ref = F.relu(inp["y64"] + inp["res"].double().reshape(inp["y64"].shape))
    return h2_restated.pow2_scale(2.0 * ref.reshape(ref.shape[0], -1).amax(dim=1).cpu().numpy(), 15)


def _plane_output(inp, split):
    c = inp["case"]
    s = _out_scales(inp)
    with _Runner(inp, split) as run:
        got = run(out_h2=True, img_out_scale=torch.from_numpy(s).cuda(), amax=True)
    _check_maxima(got, c.nimg, "with the plane output")
    out = got["out"].reshape(inp["M"], -1).cpu().numpy()
    hi, lo = h2_restated.from_rows(got["out_h2"].cpu().numpy().view(np.uint16))
    want_hi, want_lo = h2_restated.split2(out, np.repeat(s, c.r)[:, None])
    assert np.isfinite(hi.view(np.float16)).all(), "a non-finite hi: the scale from twice the fp64 maximum did not hold"
    for name, g_, w_ in (("hi", hi, want_hi), ("lo", lo, want_lo)):
        bad = np.argwhere(g_ != w_)
        assert bad.size == 0, (f"{name} plane differs from split2(out * scale) at {len(bad)} places, first (row, column) {bad[0].tolist()}: "
                               f"{hex(g_[tuple(bad[0])])} != {hex(w_[tuple(bad[0])])}, out {out[tuple(bad[0])]!r}")


def _plane_residual(inp):
    c = inp["case"]
    assert c.form == "wide"
    r = inp["res"].reshape(inp["M"], -1).cpu().numpy()
    s = h2_restated.pow2_scale(np.abs(r).reshape(c.nimg, -1).max(axis=1), 14)
    inv = (1.0 / s).astype(np.float32)
    hi, lo = h2_restated.split2(r, np.repeat(s, c.r)[:, None])
    exact = torch.from_numpy(h2_restated.join2(hi, lo, np.repeat(inv, c.r)[:, None])).cuda().reshape(inp["res"].shape)
    planes = torch.from_numpy(h2_restated.to_rows(hi, lo).view(np.int16)).cuda()
    with _Runner(inp, 1) as run:                       # (a plane residual runs unsplit: the fp32 twin is told to)
        a = run(residual=None, residual_h2=planes, img_res_inv=torch.from_numpy(inv).cuda(), amax=True)
        b = run(residual=exact, no_split=True, amax=True)
    _check_maxima(a, c.nimg, "plane residual")
    assert torch.equal(_bits(a["out"]), _bits(b["out"])), "the residual as planes and as the fp32 values (hi + lo) * inv give different bits"
    assert torch.equal(a["amax"], b["amax"])


def _group_sums(inp, split):
    c, M, cn = inp["case"], inp["M"], inp["cn"]
    if c.r % 4:
        return
    with _Runner(inp, split) as run:
        full = run(gap=True, no_split=True, amax=True)
        g = full["gap_group"]
        assert g == (4 if c.form == "wide" or c.r % 16 else 16)
        _check_maxima(full, c.nimg, "with the group sums")
        x = full["out"].reshape(M // g, g, cn).double()
        err = (full["gap"].double() - x.sum(dim=1)).abs()
        bound = g * 2.0 ** -24 * x.abs().sum(dim=1)
        assert bool((err <= bound).all()), f"group sums: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
        if M // g < 2:
            return
        gap_rows, out_rows = g * ((M // g + 1) // 2), M // 2 + 1
        out = torch.full((c.nimg, inp["ho"], inp["wo"], cn), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        gap = torch.full((M // g, cn), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        run(out=out, gap=gap, gap_rows=gap_rows, out_rows=out_rows)
        ob, gb = _bits(out).reshape(M, cn), _bits(gap)
        assert bool((ob[out_rows:] == SENTINEL).all()), "a row at or past out_rows was written"
        assert bool((gb[gap_rows // g:] == SENTINEL).all()), "a group at or past gap_rows was written"
        assert torch.equal(ob[:out_rows], _bits(full["out"]).reshape(M, cn)[:out_rows]), "rows below out_rows differ from the unrestricted launch"
        assert torch.equal(gb[:gap_rows // g], _bits(full["gap"])[:gap_rows // g]), "groups below gap_rows differ from the unrestricted launch"


def _reaches_split_finish(inp):
    """The tail split cuts K (every tile of these problems is a tail tile; it needs K / 32 >= 8 steps: host_logic.cpp)."""
    c = inp["case"]
    return c.form == "wide" and c.k * c.k * c.cin >= 256


def _with_split(cases):
    """gemm_h3 under gemm_split_k 1 and 0; gemm_x6<H2> and the back-to-back form never split (launch_x6_variant): 0 alone."""
    return [pytest.param(c, s, id=f"{_id(c)}-split{s}") for c in cases for s in ((1, 0) if c.form == "wide" else (0,))]


@pytest.mark.parametrize("case, split", _with_split(CASES))
def test_planted_maxima(case, split):
    inp = _inputs(case)
    base = _planted_maxima(inp, split, _plant_positions(case, inp["M"]))
    if split and _reaches_split_finish(inp):
        with _Runner(inp, 0) as run:
            unsplit = run(amax=True)
        assert not torch.equal(base["out"], unsplit["out"]), "gemm_split_k 1 gave the unsplit bits: the split-K finish did not run"


@pytest.mark.parametrize("case, split", _with_split([c for c in CASES if c.nimg > 1]))
def test_zero_maxima(case, split):
    _zero_maxima(_inputs(case), split)


@pytest.mark.parametrize("case, split", _with_split(CASES))
def test_plane_output(case, split):
    _plane_output(_inputs(case), split)


@pytest.mark.parametrize("case", WIDE_CASES, ids=_id)
def test_plane_residual(case):
    _plane_residual(_inputs(case))


@pytest.mark.parametrize("case", [c for c in CASES if c.r % 4 == 0], ids=_id)
def test_group_sums(case):
    _group_sums(_inputs(case), 1)


# ---- the same on drawn cases ---------------------------------------------------------------------------------------------------
@st.composite
def _cases(draw):
    form = draw(st.sampled_from(["wide", "wide", "narrow", "narrow", "b2b"]))
    if form == "b2b":
        cout, cout3 = draw(st.sampled_from([(64, 256), (128, 512)]))
        nimg = draw(st.sampled_from([n for n in NIMG if n * 784 * cout3 <= MAX_OUTPUTS]))
        return Case("b2b", 784, nimg, cout, cout, 3, 1, 1, cout3, draw(st.sampled_from([256, 128])))
    r = draw(st.sampled_from(sorted(HOWO)))
    if form == "wide":
        cin, cout = draw(st.sampled_from([32, 64, 256])), draw(st.sampled_from([256, 512]))
        k, stride, pad = draw(st.sampled_from(WIDE_GEOMS))
    else:
        cout = draw(st.sampled_from([64, 128, 192]))
        k, cin = draw(st.sampled_from(NARROW_FILTERS))
        stride = draw(st.sampled_from([1, 2]))
        pad = draw(st.sampled_from([p for p in (0, k // 2) if _has_in_size(HOWO[r][0], k, stride, p)]))      # (only maps that some input size gives)
    nimg = draw(st.sampled_from([n for n in NIMG if n * r * cout <= MAX_OUTPUTS]))
    return Case(form, r, nimg, cin, cout, k, stride, pad, 0, 256)


@settings(max_examples=40, **COMMON)
@given(case=_cases(), split=st.sampled_from([1, 0]), seed=st.integers(1, 2 ** 20), pick=st.integers(0, 2 ** 20))
def test_epilogue_outputs_on_drawn_cases(case, split, seed, pick):
    """(a) - (e) on drawn accepted geometries and contents: one planted position per example, drawn among the classes."""
    inp = _inputs.__wrapped__(case, seed)
    positions = _plant_positions(case, inp["M"])
    split = split if case.form == "wide" else 0
    _planted_maxima(inp, split, [positions[pick % len(positions)]], input_plant=pick % 3 == 0)
    _zero_maxima(inp, split)
    _plane_output(inp, split)
    if case.form == "wide":
        _plane_residual(inp)
    _group_sums(inp, split)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """What the launchers document as refused comes back as an error and writes nothing."""
    eng = engine()

    def refused(case, match, **kw):
        inp = _inputs(case)
        out = torch.full((case.nimg, inp["ho"], inp["wo"], inp["cn"]), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        args = dict(residual=inp["res"], w3=inp["w3"], bias3=inp["bias3"], out=out)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            eng.op_conv2d_nhwc_ex(inp["x"], inp["wp"], inp["bias"], case.cout, case.k, case.k, case.stride, case.pad, **args)
        torch.cuda.synchronize()
        assert bool((_bits(args["out"]) == SENTINEL).all()), "a refused launch wrote its output"

    wide9, wide49, narrow9 = WIDE_CASES[3], WIDE_CASES[5], NARROW_CASES[2]
    refused(wide49, "amax_out needs act == 1", amax=True, act=0)
    refused(narrow9, "go with a ReLU", amax=True, act=2)
    refused(narrow9, "go with a ReLU", out_h2=True, img_out_scale=torch.ones(narrow9.nimg, device="cuda"), act=0)
    refused(wide9, "Ho\\*Wo % 4 == 0", gap=True)
    refused(wide49, "Ho\\*Wo % 4 == 0", gap=True)
    refused(narrow9, "Ho\\*Wo % 4 == 0", gap=True)
    inp = _inputs(wide49)
    planes = torch.zeros((inp["M"], 2 * inp["cn"]), dtype=torch.int16, device="cuda")
    refused(wide49, "bad residual", residual_h2=planes, img_res_inv=torch.ones(wide49.nimg, device="cuda"))
    refused(wide49, "bad residual", residual=None, residual_h2=planes)
    inp = _inputs(narrow9)
    planes = torch.zeros((inp["M"], 2 * inp["cn"]), dtype=torch.int16, device="cuda")
    refused(narrow9, "goes with the wide form", residual=None, residual_h2=planes, img_res_inv=torch.ones(narrow9.nimg, device="cuda"))
    # the back-to-back form: images of at least 256 pixels and a multiple of 16, an fp32 residual, 64 or 128 columns in the middle
    for c in (NARROW_CASES[6], NARROW_CASES[3]):           # r = 196 (< 256, not a multiple of 16), r = 16
        g = np.random.default_rng(1)
        w3 = torch.from_numpy(g.standard_normal((256, c.cout)).astype(np.float32)).cuda()
        i = _inputs(c)
        refused(c, "back-to-back form needs", w3=w3, bias3=torch.zeros(256, device="cuda"),
                residual=torch.zeros((c.nimg, i["ho"], i["wo"], 256), device="cuda"),
                out=torch.full((c.nimg, i["ho"], i["wo"], 256), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32))
    refused(B2B_CASES[0], "back-to-back form needs", residual=None)
    c = NARROW_CASES[9]                                     # 192 columns in the middle
    i = _inputs(c)
    refused(c, "back-to-back form needs", w3=torch.zeros((256, 192), device="cuda"), bias3=torch.zeros(256, device="cuda"),
            residual=torch.zeros((c.nimg, i["ho"], i["wo"], 256), device="cuda"),
            out=torch.full((c.nimg, i["ho"], i["wo"], 256), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32))
    # no f16x2 form: a 1x1 onto 64 columns
    x = torch.zeros((1, 4, 4, 64), device="cuda")
    with pytest.raises(RuntimeError, match="has no f16x2 form"):
        eng.op_conv2d_nhwc_ex(x, torch.zeros((64, 64), device="cuda"), None, 64, 1, 1, 1, 0)
    eng.set_precision("bf16x6")
    try:
        with pytest.raises(RuntimeError, match="gemm_precision"):
            i = _inputs(wide49)
            eng.op_conv2d_nhwc_ex(i["x"], i["wp"], i["bias"], wide49.cout, wide49.k, wide49.k, wide49.stride, wide49.pad)
    finally:
        eng.set_precision("f16x2")


# ---- the stem ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw, nimg", [(112, 3), (8, 37)], ids=["112x112x64", "8x8x64"])
def test_stem_maxima(hw, nimg):
    """bn_relu_maxpool's per-image maxima (block maxima, then image_max_of_blocks) == bits of y.max(); 8x8x64 is the smallest 64-channel
    map with whole 256-thread blocks per image (4 x 4 x 16 threads: one block per image)."""
    eng = engine()
    g = np.random.default_rng(hw)
    C = 64
    x = torch.from_numpy(g.standard_normal((nimg, hw, hw, C)).astype(np.float32)).cuda()
    scale = torch.from_numpy(g.uniform(0.5, 2.0, C).astype(np.float32)).cuda()
    shift = torch.from_numpy((g.standard_normal(C) * 0.5).astype(np.float32)).cuda()
    z = nimg // 2
    x[z] = -x[z].abs()                              # all outputs of image z are zero: relu(negative * scale + shift), shift <= 0 there
    shift_z = -shift.abs()

    def run(xx, sh):
        amax = torch.full((nimg,), -1, dtype=torch.int32, device="cuda")
        y = eng.op_bn_relu_maxpool(xx, scale, sh, amax_out=amax)
        assert torch.equal(y, eng.op_bn_relu_maxpool(xx, scale, sh)), "the output depends on amax_out"
        want = _img_max_bits(y, nimg)
        assert torch.equal(amax, want), f"stem maxima {amax.tolist()} != bits of y.max() {want.tolist()}"
        return y, amax

    y, base = run(x, shift_z)
    assert int(base[z]) == 0 and not bool(_bits(y[z]).any()), "the all-zero image"
    t = 0 if z else nimg - 1
    o = hw // 2
    for (oy, ox, ch) in ((0, 0, 0), (0, o - 1, 1), (o - 1, 0, C - 2), (o - 1, o - 1, C - 1), (o // 2, o // 2, C - 1)):
        xp = x.clone()
        xp[t, min(2 * oy, hw - 1), min(2 * ox, hw - 1), ch] = PLANT
        y, amax = run(xp, shift_z)
        flat = y[t].reshape(-1)
        assert float(flat.max()) > PLANT / 4 and bool(y[t, oy, ox, ch] == flat.max()), "the plant is not the image's maximum"
        others = torch.arange(nimg, device="cuda") != t
        assert torch.equal(amax[others], base[others])
    with pytest.raises(RuntimeError, match="whole blocks per image"):
        eng.op_bn_relu_maxpool(torch.zeros((2, 6, 6, C), device="cuda"), scale, shift, amax_out=torch.zeros(2, dtype=torch.int32, device="cuda"))
