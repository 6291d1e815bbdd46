"""The f16x2 streaming attention (csrc/attention_stream_h2.hip) on the GPU: the operator (op_attention_ex under f16x2 with "att_h2_stream")
against fp64 and against torch-CPU fp32's own distance from fp64, and ViT-B forwards at token counts other than 197 against the CPU
restatement and against the bf16x6 streaming route they replace.  The measured ratios live in profiles/attention_stream_h2_parity.json
(written by tools/attention_stream_h2_parity.py from the functions below); the gates are the next power of two above them, capped."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import vit_ref
from tests import gpu_common, vit_canvas_ref, vit_patch8_cases as cases
from tests.gpu_common import assert_close, engine, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "attention_stream_h2_parity.json")
MODEL_CAP = 4.0
TILE, QBLOCK = 64, 128          # host::kAttStreamH2KeyTile / kAttStreamH2QBlock (tests/test_attention_stream_h2_cpu.py reads them from the plan)

# (ntok, images, heads)
OP_CASES = [
    (1, 2, 3),
    (TILE, 1, 3),
    (TILE + 1, 2, 3),       # the second tile holds one real key
    (QBLOCK + 1, 1, 3),     # the second query block holds one query
    (197, 3, 12),
    (785, 2, 3),
    (785, 6, 12),           # more items than CUs
    (4097, 1, 2),
]


@pytest.fixture(autouse=True)
def _options_are_restored():
    eng = engine()
    before = eng.get_option("att_h2_stream"), eng.get_option("att_h2")
    yield
    eng.set_option("att_h2_stream", before[0])
    eng.set_option("att_h2", before[1])
    eng.set_precision("f16x2")


def _route(stream, att_h2=1):
    eng = engine()
    eng.set_precision("f16x2")
    eng.set_option("att_h2", att_h2)
    eng.set_option("att_h2_stream", stream)
    return eng


def _gate(ratio, cap):
    gate = 1.0
    while gate <= ratio:
        gate *= 2.0
    return min(gate, cap)


def _recorded(section):
    with open(PARITY_JSON) as f:
        return float(json.load(f)[section]["worst_ratio"])


def _norm_rel(got, ref64):
    got = got.cpu().double() if isinstance(got, torch.Tensor) else torch.from_numpy(np.asarray(got)).double()
    ref64 = ref64.double() if isinstance(ref64, torch.Tensor) else torch.from_numpy(np.asarray(ref64)).double()
    return float(torch.linalg.norm(got - ref64) / torch.linalg.norm(ref64))


# ---- operator level --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op_case(ntok, n_img, heads, scale):
    if (ntok, n_img, heads) in cases.CASES:
        return cases.case(ntok, n_img, heads, scale)
    qkv = cases.random_qkv(ntok, n_img, heads, scale)
    return qkv, cases.attention_cpu(qkv, n_img, ntok, heads, torch.float64), cases.attention_cpu(qkv, n_img, ntok, heads, torch.float32)


def _op_run(qkv, n_img, ntok, heads, ref64, what):
    """-> the new route's result, checked: 1e-3 of fp64, the same bits on a second call, other bits than the bf16x6 route's"""
    x = qkv.cuda()
    eng = _route(1)
    got = eng.op_attention_ex(x, n_img, ntok, heads)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    rel = _norm_rel(got, ref64)
    print(f"\n{what}: norm-rel error against fp64 {rel:.3e}")
    assert rel < 1e-3, f"{what}: {rel:.3e} from fp64"
    assert torch.equal(got, eng.op_attention_ex(x, n_img, ntok, heads)), f"{what}: a second call gives other bits"
    old = _route(0).op_attention_ex(x, n_img, ntok, heads)
    assert _norm_rel(old, ref64) < 1e-3
    assert not torch.equal(got, old), f"{what}: bit-equal to the bf16x6 streaming route - the f16x2 kernel did not run"
    return got


def _parity(got, ref64, cpu32, what):
    """vit_patch8_cases.parity_ratio, or None where torch-CPU fp32 has NO distance from fp64 to measure in: one key, softmax = 1, the output is V
    itself.  The kernel is then held to what two fp16 planes at one scale for the tensor keep of a value: 2^-22 of it (hi and lo round to 11
    bits each), plus half an fp16 subnormal step (2^-25) over the scale, which puts the tensor's maximum at or above 2^14: 2^-39 of it.
    Everything behind the split is exact there: e = 1, planes of 2^14, 1 / l = 1, and a 22-bit value splits again without loss."""
    if float((cpu32.double() - ref64).abs().max()) > 0.0:
        return cases.parity_ratio(got, ref64, cpu32)
    err = (got.cpu().double() - ref64).abs()
    bound = ref64.abs() * 2.0 ** -22 + float(ref64.abs().max()) * 2.0 ** -38
    assert bool((err <= bound).all()), f"{what}: {float((err - bound).max()):.3e} above the bound of the plane format"
    return None


def measure_operator():
    """-> {case: parity ratio}: the kernel's distance from fp64 in units of torch-CPU fp32's own (vit_patch8_cases.parity_ratio)"""
    out = {}
    for ntok, n_img, heads in OP_CASES:
        for scale in cases.SCALES:
            qkv, ref64, cpu32 = _op_case(ntok, n_img, heads, scale)
            got = _route(1).op_attention_ex(qkv.cuda(), n_img, ntok, heads)
            r = _parity(got, ref64, cpu32, f"ntok={ntok} scale {scale}")
            if r is not None:
                out[f"{ntok}x{n_img}x{heads}@{scale}"] = r
    for order in cases.KEY_ORDERS:
        qkv, ref64 = cases.order_case(order)
        got = _route(1).op_attention_ex(qkv.cuda(), 1, 785, 3)
        out[order] = cases.parity_ratio(got, ref64, cases.attention_cpu(qkv, 1, 785, 3, torch.float32))
    return out


@pytest.mark.parametrize("scale", cases.SCALES)
@pytest.mark.parametrize("ntok,n_img,heads", OP_CASES)
def test_operator_against_fp64(ntok, n_img, heads, scale):
    qkv, ref64, cpu32 = _op_case(ntok, n_img, heads, scale)
    what = f"f16x2 streaming attention ntok={ntok} {n_img}x{heads} scale {scale}"
    got = _op_run(qkv, n_img, ntok, heads, ref64, what)
    ratio, gate = _parity(got, ref64, cpu32, what), _gate(_recorded("operator_vs_torch_cpu_fp32"), cases.PARITY_CAP)
    if ratio is None:
        return      # (one key: held to the plane format's bound instead, see _parity)
    print(f"{what}: {ratio:.3f} x torch-CPU fp32's distance from fp64 (gate {gate})")
    assert ratio <= gate, f"{what}: {ratio:.3f} x torch-CPU fp32's distance from fp64, gate {gate}"


@pytest.mark.parametrize("order", cases.KEY_ORDERS)
def test_operator_constructed_key_orders(order):
    """ascending logits: the row maximum sits in the last key tile and moves at every tile; descending: it sits in the first."""
    qkv, ref64 = cases.order_case(order)
    what = f"f16x2 streaming attention 785 keys {order}"
    got = _op_run(qkv, 1, 785, 3, ref64, what)
    ratio = cases.parity_ratio(got, ref64, cases.attention_cpu(qkv, 1, 785, 3, torch.float32))
    gate = _gate(_recorded("operator_vs_torch_cpu_fp32"), cases.PARITY_CAP)
    print(f"{what}: ratio {ratio:.3f} (gate {gate})")
    assert ratio <= gate, f"{what}: {ratio:.3f}, gate {gate}"


def test_the_recorded_operator_ratio_is_below_the_cap():
    assert _recorded("operator_vs_torch_cpu_fp32") <= cases.PARITY_CAP      # a ratio above the cap is a bug, not a gate
    assert _recorded("model_vs_bf16x6_route") <= MODEL_CAP


def test_operator_refuses_bad_arguments():
    eng = _route(1)
    x = torch.zeros((64, 192), device="cuda")
    with pytest.raises(RuntimeError, match="ntok=0"):
        eng._check(eng.lib.relax_op_attention_ex(eng.h, x.data_ptr(), x.data_ptr(), 1, 0, 1, None), "relax_op_attention_ex")
    with pytest.raises(RuntimeError, match="heads=0"):
        eng._check(eng.lib.relax_op_attention_ex(eng.h, x.data_ptr(), x.data_ptr(), 1, 64, 0, None), "relax_op_attention_ex")
    for a, b in ((None, x.data_ptr()), (x.data_ptr(), None)):
        with pytest.raises(RuntimeError, match="NULL"):
            eng._check(eng.lib.relax_op_attention_ex(eng.h, a, b, 1, 64, 1, None), "relax_op_attention_ex")


def test_the_option_reads_back():
    eng = engine()
    for v in (0, 1):
        eng.set_option("att_h2_stream", v)
        assert eng.get_option("att_h2_stream") == v


# ---- model level -----------------------------------------------------------------------------------------------------------------------
# (patch, Hc, Wc, images): 16 tokens; 136 tokens = two query blocks; 1057 tokens = the wide CLS-attention instantiation; ViT-B/8's 785
MODEL_CASES = [(16, 48, 80, 3), (16, 144, 240, 2), (16, 528, 512, 1), (8, 224, 224, 1)]
MODEL_IDS = ["p16-48x80", "p16-144x240", "p16-528x512", "p8-224x224"]


@functools.lru_cache(maxsize=None)
def _weights(patch, adversarial):
    return synth.vit_state_dict("vit_base", patch=patch, adversarial=adversarial)


def _load(patch, adversarial):
    if patch == 16:
        return gpu_common.vit_weights("vit_base", adversarial)
    key = f"vit{patch}:vit_base:{adversarial}"
    if gpu_common._weights.get("vit_loaded") != key:
        engine().load_vit(_weights(patch, adversarial), "vit_base")
        gpu_common._weights["vit_loaded"] = key
    return _weights(patch, adversarial)


def _images(n, Hc, Wc):
    return np.random.default_rng(Hc * 1000 + Wc).integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _model_reference(patch, adversarial, n, Hc, Wc):
    """-> (images, tokens, pooled, the last block's CLS attention row [n, heads, ntok]) of the CPU restatement, once per case"""
    imgs = _images(n, Hc, Wc)
    tsd = vit_ref.to_torch_state_dict(_weights(patch, adversarial))
    _, tok, att = vit_canvas_ref.forward_canvas(tsd, vit_canvas_ref.preprocess_bgr_u8(imgs), 12, patch)
    tok = tok.numpy()
    return imgs, tok, vit_canvas_ref.pooled(tok), att[:, :, 0, :].numpy()


@functools.lru_cache(maxsize=None)
def _model_run(patch, adversarial, n, Hc, Wc, stream, att_h2=1):
    _load(patch, adversarial)
    eng = _route(stream, att_h2)
    imgs = _model_reference(patch, adversarial, n, Hc, Wc)[0]
    tok, pool, _ = eng.vit_features(imgs, tokens=True, pooled=True, attention=True)
    return tok, pool, eng.vit_attention(imgs, with_cls=True)


def _model_ratios(patch, adversarial, n, Hc, Wc):
    """-> {output: distance of the new route from the restatement / the bf16x6 route's distance}"""
    _, tok, pooled, att = _model_reference(patch, adversarial, n, Hc, Wc)
    new, old = _model_run(patch, adversarial, n, Hc, Wc, 1), _model_run(patch, adversarial, n, Hc, Wc, 0)
    return {name: _norm_rel(g, w) / _norm_rel(o, w) for name, g, o, w in zip(("tokens", "pooled", "attention"), new, old, (tok, pooled, att))}


def measure_model():
    out = {}
    for (patch, Hc, Wc, n), cid in zip(MODEL_CASES, MODEL_IDS):
        for adversarial in (False, True):
            for k, v in _model_ratios(patch, adversarial, n, Hc, Wc).items():
                out[f"{cid}{'-adversarial' if adversarial else ''}:{k}"] = v
    return out


@pytest.mark.parametrize("adversarial", [False, True], ids=["regular", "adversarial"])
@pytest.mark.parametrize("patch,Hc,Wc,n", MODEL_CASES, ids=MODEL_IDS)
def test_vit_base_on_the_f16x2_streaming_route(patch, Hc, Wc, n, adversarial):
    imgs, tok, pooled, att = _model_reference(patch, adversarial, n, Hc, Wc)
    g_tok, g_pool, g_row = _model_run(patch, adversarial, n, Hc, Wc, 1)
    what = f"vit_base/{patch} {Hc}x{Wc} f16x2 att_h2_stream{' adversarial' if adversarial else ''}"
    ntok = (Hc // patch) * (Wc // patch) + 1
    assert tuple(g_tok.shape) == (n, ntok - 1, 768) and tuple(g_row.shape) == (n, 12, ntok)
    assert_close(g_tok, tok, f"{what} tokens")
    assert_close(g_pool, pooled, f"{what} pooled")
    assert_close(g_row, att, f"{what} CLS attention row")
    assert float((g_row.sum(dim=2) - 1).abs().max()) <= 1e-5, f"{what}: attention rows do not sum to 1"
    # the new route ran: other bits than the bf16x6 streaming route's
    o_tok = _model_run(patch, adversarial, n, Hc, Wc, 0)[0]
    assert not torch.equal(g_tok, o_tok), f"{what}: bit-equal to the att_h2_stream = 0 route"
    gate = _gate(_recorded("model_vs_bf16x6_route"), MODEL_CAP)
    for name, r in _model_ratios(patch, adversarial, n, Hc, Wc).items():
        print(f"\n{what} {name}: {r:.3f} x the bf16x6 route's distance from the restatement (gate {gate})")
        assert r <= gate, f"{what} {name}: {r:.3f} x the bf16x6 route's distance from the restatement, gate {gate}"


def test_an_image_does_not_depend_on_its_batch():
    _load(16, False)
    eng = _route(1)
    imgs = _images(3, 144, 240)
    tok, pool, att = eng.vit_features(imgs, tokens=True, pooled=True, attention=True)
    for i in range(3):
        t1, p1, a1 = eng.vit_features(imgs[i:i + 1], tokens=True, pooled=True, attention=True)
        assert torch.equal(t1[0], tok[i]) and torch.equal(p1[0], pool[i]) and torch.equal(a1[0], att[i]), f"image {i} alone differs from the batch"


def test_the_last_tap_of_the_layer_stack_is_vit_features():
    _load(16, False)
    eng = _route(1)
    imgs = _images(2, 144, 240)
    tok, pool = eng.vit_features(imgs, tokens=True, pooled=True)
    taps = eng.vit_intermediate_layers(imgs, n=1, tokens=True, cls=True, pooled=True)
    assert torch.equal(taps["tokens"][-1][:, 1:], tok) and torch.equal(taps["pooled"][-1], pool)
    old = _route(0).vit_features(imgs, tokens=True, pooled=False)[0]
    assert not torch.equal(old, tok)


def test_197_tokens_are_untouched_by_the_option():
    _load(16, False)
    imgs = _images(2, 224, 224)
    a = _route(1).vit_features(imgs, tokens=True, pooled=True, attention=True)
    b = _route(0).vit_features(imgs, tokens=True, pooled=True, attention=True)
    for x, y, what in zip(a, b, ("tokens", "pooled", "attention")):
        assert torch.equal(x, y), f"224 x 224: {what} differs between att_h2_stream 1 and 0"
    qkv = cases.case(197, 3, 12, 1.0)[0].cuda()
    assert torch.equal(_route(1).op_attention(qkv, 3, 12), _route(0).op_attention(qkv, 3, 12))


def test_option_0_is_the_bf16x6_streaming_route():
    """att_h2 = 0 takes the bf16x6 branch whatever att_h2_stream says: att_h2_stream = 0 (under att_h2 = 1) must give its bits"""
    patch, Hc, Wc, n = MODEL_CASES[1]
    want = _model_run(patch, False, n, Hc, Wc, 1, 0)
    got = _model_run(patch, False, n, Hc, Wc, 0, 1)
    for x, y, what in zip(got, want, ("tokens", "pooled", "attention")):
        assert torch.equal(x, y), f"{what}: att_h2_stream = 0 differs from the att_h2 = 0 route"
    qkv = cases.case(785, 2, 3, 1.0)[0].cuda()
    assert torch.equal(_route(0, 1).op_attention_ex(qkv, 2, 785, 3), _route(1, 0).op_attention_ex(qkv, 2, 785, 3))
