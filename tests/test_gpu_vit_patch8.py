"""DINO ViTs at patch size 8 (785 tokens) on the GPU: the streaming attention kernels (csrc/attention_stream.hip) at operator level
against fp64, the patch-8 forwards against oracle.vit_ref.forward_tokens(patch=8), and the Python surface around them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit_ref
from tests import gpu_common, vit_patch8_cases as cases
from tests.gpu_common import assert_close, engine, synth

pytestmark = pytest.mark.gpu

HEADS = {"vit_tiny": 3, "vit_small": 6, "vit_base": 12}


# ---- operator level -----------------------------------------------------------------------------------------------------------------
def _stream_both(qkv, n_img, ntok, heads):
    """-> (fp32 streaming result, bf16x6 streaming result); each is checked to be bit-equal on a second call"""
    eng = engine()
    out = {}
    x = qkv.cuda()
    for mode in ("fp32", "bf16x6"):
        eng.set_precision(mode)
        out[mode] = eng.op_attention_ex(x, n_img, ntok, heads)
        assert torch.equal(out[mode], eng.op_attention_ex(x, n_img, ntok, heads)), f"{mode}: a second call gives other bits"
    return out["fp32"], out["bf16x6"]


def _errs(got, ref64):
    e = (got.cpu().double() - ref64).abs()
    return e.mean().item(), e.max().item()


def _check_pair(what, g32, g6, ref64):
    ref = ref64.float().numpy()
    assert_close(g32, ref, f"{what} fp32 streaming")
    assert_close(g6, ref, f"{what} bf16x6 streaming")
    (m32, x32), (m6, x6) = _errs(g32, ref64), _errs(g6, ref64)
    print(f"\n{what}: mean err fp32 {m32:.3e} x6 {m6:.3e}; max fp32 {x32:.3e} x6 {x6:.3e}")
    assert m6 <= 1.25 * m32 + 1e-12 and x6 <= 2.0 * x32 + 1e-12, f"{what}: x6 against the fp32 streaming kernel"   # tests/test_gpu_x6.py's factors
    return (m32, x32), (m6, x6)


@pytest.mark.parametrize("scale", cases.SCALES)
@pytest.mark.parametrize("ntok,n_img,heads", cases.CASES)
def test_stream_attention_against_fp64(ntok, n_img, heads, scale):
    eng = engine()
    qkv, ref64, cpu32 = cases.case(ntok, n_img, heads, scale)
    what = f"attention ntok={ntok} {n_img}x{heads} scale {scale}"
    g32, g6 = _stream_both(qkv, n_img, ntok, heads)
    (m32, x32), (m6, x6) = _check_pair(what, g32, g6, ref64)
    if ntok == 197:   # each streaming kernel against its single-tile counterpart's error
        for mode, (m, x) in (("fp32", (m32, x32)), ("bf16x6", (m6, x6))):
            eng.set_precision(mode)
            ms, xs = _errs(eng.op_attention(qkv.cuda(), n_img, heads), ref64)
            print(f"{what} {mode}: single-tile mean {ms:.3e} max {xs:.3e}; streaming mean {m:.3e} max {x:.3e}")
            assert m <= 1.25 * ms + 1e-12 and x <= 2.0 * xs + 1e-12, f"{what} {mode}: streaming against the single-tile kernel"
    if ntok == 785:   # the fp32 streaming kernel against torch-CPU fp32's own distance from fp64
        ratio, gate = cases.parity_ratio(g32, ref64, cpu32), cases.parity_gate()
        print(f"{what}: fp32 streaming / torch-CPU fp32 error ratio {ratio:.3f} (gate {gate})")
        assert ratio <= gate, f"{what}: {ratio:.3f} x torch-CPU fp32's distance from fp64, gate {gate}"


@pytest.mark.parametrize("order", cases.KEY_ORDERS)
def test_stream_attention_constructed_key_orders(order):
    """ascending logits: the row maximum sits in the last key tile and moves at every tile; descending: it sits in the first."""
    qkv, ref64 = cases.order_case(order)
    g32, g6 = _stream_both(qkv, 1, 785, 3)
    _check_pair(f"attention 785 keys {order}", g32, g6, ref64)


def test_stream_attention_refuses_bad_arguments():
    eng = engine()
    with pytest.raises(ValueError):
        eng.op_attention_ex(torch.zeros((10, 192), device="cuda"), 1, 11, 1)
    with pytest.raises(RuntimeError, match="ntok=0"):
        eng._check(eng.lib.relax_op_attention_ex(eng.h, 1, 1, 1, 0, 1, None), "relax_op_attention_ex")


# ---- model level --------------------------------------------------------------------------------------------------------------------
def _fragments(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def _load8(name, adversarial=False):
    """synthetic patch-8 weights into the shared engine (the other GPU tests' weight cache is told that its model is gone)"""
    sd = _weights8(name, adversarial)
    key = f"vit8:{name}:{adversarial}"
    if gpu_common._weights.get("vit_loaded") != key:
        engine().load_vit(sd, name)
        gpu_common._weights["vit_loaded"] = key
    return sd


@functools.lru_cache(maxsize=None)
def _weights8(name, adversarial):
    return synth.vit_state_dict(name, patch=8, adversarial=adversarial)


@torch.no_grad()
def _cls_attention_ref(sd, x, heads, patch):
    """the last block's softmax(q_0 k^T / 8) [B, heads, ntok], with oracle.vit_ref.forward_tokens' operations up to there"""
    B = x.shape[0]
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
    t = torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1) + sd["pos_embed"]
    dim = t.shape[-1]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    for i in range(depth):
        p = f"blocks.{i}."
        y = F.layer_norm(t, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], vit_ref.LN_EPS)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, -1, 3, heads, 64).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * 0.125).softmax(dim=-1)
        if i == depth - 1:
            return attn[:, :, 0, :].numpy()
        t = t + F.linear((attn @ qkv[2]).transpose(1, 2).reshape(B, -1, dim), sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        y = F.layer_norm(t, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], vit_ref.LN_EPS)
        t = t + F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


@functools.lru_cache(maxsize=None)
def _model_reference(name, adversarial, n):
    """-> (fragments, tokens, pooled, CLS attention) of the oracle, once per model and weight set"""
    frags = _fragments(n, seed=5)
    tsd = vit_ref.to_torch_state_dict(_weights8(name, adversarial))
    x = vit_ref.preprocess_bgr_u8(frags)
    tok = vit_ref.forward_tokens(tsd, x, HEADS[name], patch=8).numpy()
    pooled = np.concatenate([tok.mean(axis=1), tok.max(axis=1), tok.std(axis=1)], axis=1).astype(np.float32)
    return frags, tok, pooled, _cls_attention_ref(tsd, x, HEADS[name], 8)


def _check_model(name, adversarial, n, precision):
    frags, tok, pooled, att = _model_reference(name, adversarial, n)
    _load8(name, adversarial)
    eng = engine()
    eng.set_precision(precision)
    g_tok, g_pool, g_att = eng.vit_features(frags, tokens=True, pooled=True, attention=True)
    what = f"{name}/8 {precision}{' adversarial' if adversarial else ''}"
    assert tuple(g_tok.shape) == (n, 784, tok.shape[2]) and tuple(g_att.shape) == (n, HEADS[name], 784)
    assert_close(g_tok, tok, f"{what} tokens")
    assert_close(g_pool, pooled, f"{what} pooled")
    assert_close(g_att, att[:, :, 1:], f"{what} CLS attention")
    row = eng.vit_attention(frags, with_cls=True)
    assert tuple(row.shape) == (n, HEADS[name], 785)
    assert float((row.sum(dim=2) - 1).abs().max()) <= 1e-5, f"{what}: attention rows do not sum to 1"
    assert torch.equal(row[:, :, 1:], g_att), f"{what}: vit_attention differs from vit_features(attention=True)"


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_vit_tiny_patch8_matches_oracle(precision):
    """the default precision runs vit_tiny (dim 192) on the bf16x6 forward, with the bf16x6 streaming attention"""
    _check_model("vit_tiny", False, 3, precision)


@pytest.mark.parametrize("adversarial", [False, True], ids=["regular", "adversarial"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x2"])
def test_vit_base_patch8_matches_oracle(precision, adversarial):
    """f16x2: the f16x2 forward with the bf16x6 streaming attention writing fp16 planes (the att_h2 = 0 branch, whatever att_h2 says)"""
    _check_model("vit_base", adversarial, 2, precision)


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def test_load_vit_infers_patch_size_and_geometry_reads_back():
    eng = engine()
    _load8("vit_tiny")
    assert (eng.vit_patch, eng.vit_ntok, eng.vit_npatch) == (8, 785, 784)
    assert eng.vit_geometry() == (8, 785, 192, 3)
    frags = _fragments(2, seed=9)
    tok8, _ = eng.vit_features(frags, tokens=True, pooled=False)
    assert tuple(tok8.shape) == (2, 784, 192)
    # patch 16 after patch 8 on the same handle: the old geometry is back
    gpu_common.vit_weights("vit_tiny")
    assert (eng.vit_patch, eng.vit_ntok, eng.vit_npatch) == (16, 197, 196) and eng.vit_geometry() == (16, 197, 192, 3)
    tok16, _ = eng.vit_features(frags, tokens=True, pooled=False)
    assert tuple(tok16.shape) == (2, 196, 192)
    assert_close(tok16, vit_ref.tokens(vit_ref.to_torch_state_dict(synth.vit_state_dict("vit_tiny")), frags, 3), "vit_tiny/16 after /8")


def test_mismatched_pos_embed_is_refused_with_both_counts():
    eng = engine()
    gpu_common.vit_weights("vit_tiny")
    sd = dict(synth.vit_state_dict("vit_tiny", patch=8))
    sd["pos_embed"] = synth.vit_state_dict("vit_tiny")["pos_embed"]          # 197 rows under an 8x8 patch embedding
    with pytest.raises(RuntimeError, match=r"197 tokens.*785 tokens"):
        eng.load_vit(sd, "vit_tiny")
    with pytest.raises(RuntimeError, match=r"785 tokens.*197 tokens"):       # a whole patch-8 checkpoint declared as patch 16
        eng.load_vit(synth.vit_state_dict("vit_tiny", patch=8), "vit_tiny", patch_size=16)
    sd = dict(synth.vit_state_dict("vit_tiny"))
    sd["patch_embed.proj.weight"] = synth.vit_state_dict("vit_tiny", patch=8)["patch_embed.proj.weight"]
    with pytest.raises(RuntimeError, match=r"patch_embed\.proj\.weight.*192 per output channel.*needs 768"):
        eng.load_vit(sd, "vit_tiny", patch_size=16)
    assert eng.vit_geometry() == (16, 197, 192, 3)                           # the refused loads left the loaded model alone
    assert tuple(eng.vit_features(_fragments(1, seed=2), tokens=True, pooled=False)[0].shape) == (1, 196, 192)


def test_overlays_refuse_a_patch8_model():
    eng = engine()
    _load8("vit_tiny")
    clip = torch.from_numpy(synth.synthetic_clip(1, 240, 320, clip_id=1)).cuda()
    with pytest.raises(ValueError, match="patch size 8"):
        eng.attention_overlays(clip)
    with pytest.raises(ValueError, match="patch size 8"):
        eng.attention_overlay(clip[:, 0], torch.zeros((1, 196, 2), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32),
                              torch.zeros((1, 196)))


def test_vit_generator_patch8_tokens():
    from relax_vqa_amd import runtime
    from relax_vqa_amd.extractor import visualise_vit_layer
    try:
        model = visualise_vit_layer.VitGenerator("vit_small", 8, None, random=True)
        frag = _fragments(1, seed=3)
        t = visualise_vit_layer.process_fragment_array(frag, model)
        assert t.shape == (784, 384)
        want = vit_ref.forward_tokens(vit_ref.to_torch_state_dict(synth.vit_state_dict("vit_small", patch=8)), vit_ref.preprocess_bgr_u8(frag), 6,
                                      patch=8).numpy()[0]
        assert_close(t, want, "VitGenerator(vit_small, 8) tokens")
        with pytest.raises(ValueError, match=r"16.*8|8.*16"):      # the injected weights are patch 8: a patch-16 generator on them is refused
            runtime.ensure_vit("vit_small", 16)
    finally:
        runtime.set_weights(vit=synth.vit_state_dict("vit_base"), vit_name="vit_base")   # what the other host-API tests run on


def test_extract_clip_with_a_patch8_vit():
    eng = engine()
    gpu_common.rn50_weights()
    _load8("vit_base")
    clip = torch.from_numpy(synth.synthetic_clip(2, 270, 480, clip_id=4)).cuda()
    out = eng.extract_clip(clip)
    assert tuple(out["vit"].shape) == (2, 4608)
    fr = eng.fragment_pairs(clip)                      # the fragments the clip path runs its backbones on, in its batch order
    _, pooled = eng.vit_features(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), tokens=False, pooled=True)
    assert torch.equal(out["vit"], torch.cat([pooled[:2], pooled[2:]], dim=1))
    rows = eng.clip_vectors([clip], resnet=False, vit=True)
    assert tuple(rows.shape) == (1, 4608)
