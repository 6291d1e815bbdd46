"""The ViT layer stack on the GPU (relax_vit_intermediate_layers: csrc/vit.hip's taps, csrc/vit_layers.hip's vit_norm_token_stats): every tap
against the restatement tests/vit_layers_ref.intermediate_layers (itself pinned to the reference's method by tests/test_vit_layers_cpu.py)
under the three arithmetics, its distance from an fp64 run beside the existing path's, the bit identities that tie the fused kernel to
layernorm_rows + vit_token_stats and the taps to each other, the refusals and the Python surface.

Shapes are the small ones at which the kernel takes another path: dim 192 (lanes 48..63 of a row wave hold nothing), 384 and 768; 1 patch
(three empty token groups), 6 and 15 patches (fewer rows than the 16 waves; a count no multiple of 4), 41 tokens at patch 8, 197 tokens
(more rows than waves, the single-tile attention)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import vit_ref
from tests import gpu_common, vit_canvas_ref, vit_layers_ref
from tests.gpu_common import assert_close, engine, synth

pytestmark = pytest.mark.gpu

HEADS = {"vit_tiny": 3, "vit_small": 6, "vit_base": 12}
DIMS = {"vit_tiny": 192, "vit_small": 384, "vit_base": 768}
DEPTH = 12
PRECISIONS = ["fp32", "bf16x6", "f16x2"]


@functools.lru_cache(maxsize=None)
def _weights(name, patch, adversarial):
    return synth.vit_state_dict(name, patch=patch, adversarial=adversarial)


def _load(name, patch=16, adversarial=False):
    """synthetic weights into the shared engine, through the other GPU tests' cache where it knows the model (patch 16)"""
    if patch == 16:
        return gpu_common.vit_weights(name, adversarial)
    key = f"vit{patch}:{name}:{adversarial}"
    if gpu_common._weights.get("vit_loaded") != key:
        engine().load_vit(_weights(name, patch, adversarial), name)
        gpu_common._weights["vit_loaded"] = key
    return _weights(name, patch, adversarial)


def _images(n, Hc, Wc):
    return np.random.default_rng(Hc * 1000 + Wc + 7).integers(0, 256, (n, Hc, Wc, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(name, patch, adversarial, n_img, Hc, Wc, n, fp64=False):
    """-> (images, [taps as numpy [n_img, ntok, dim]]) of the restatement, once per case"""
    imgs = _images(n_img, Hc, Wc)
    sd = _load(name, patch, adversarial)
    taps = vit_layers_ref.intermediate_layers(vit_ref.to_torch_state_dict(sd), vit_canvas_ref.preprocess_bgr_u8(imgs), HEADS[name], patch, n,
                                              dtype=torch.float64 if fp64 else torch.float32)
    return imgs, [t.numpy() for t in taps]


# ---- parity against the restatement ----------------------------------------------------------------------------------------------------
# (model, patch, adversarial, images, Hc, Wc, n)
PARITY_CASES = [
    ("vit_tiny", 16, False, 1, 16, 16, 3),       # 1 patch: three empty token groups, std 0; the one case with a single image
    ("vit_tiny", 16, False, 2, 32, 48, 3),       # 6 patches: 7 rows for 16 waves
    ("vit_tiny", 16, False, 2, 48, 80, 3),       # 15 patches: groups of 4, 4, 4, 3
    ("vit_tiny", 16, False, 2, 224, 224, 3),     # 197 tokens: the single-tile attention, 12-13 rows per wave
    ("vit_tiny", 8, False, 2, 64, 40, 3),
    ("vit_small", 16, False, 3, 224, 224, 12),
    ("vit_base", 16, False, 2, 224, 224, 4),
    ("vit_base", 16, True, 2, 224, 224, 4),
]


def _case_id(c):
    return f"{c[0]}-p{c[1]}{'-adv' if c[2] else ''}-{c[3]}x{c[4]}x{c[5]}-n{c[6]}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", PARITY_CASES, ids=[_case_id(c) for c in PARITY_CASES])
def test_taps_match_the_restatement(case, precision):
    """gpu_common.assert_close's bar (1e-3 relative, floor 1e-4 x the mean magnitude), as every ViT gate; f16x2 runs its own branch at dim
    768 only (the smaller models take bf16x6 under it)."""
    name, patch, adversarial, n_img, Hc, Wc, n = case
    _load(name, patch, adversarial)
    imgs, want = _reference(*case)
    eng = engine()
    eng.set_precision(precision)
    out = eng.vit_intermediate_layers(imgs, n=n, tokens=True, cls=True, pooled=True)
    ntok, dim = (Hc // patch) * (Wc // patch) + 1, DIMS[name]
    assert tuple(out["tokens"].shape) == (n, n_img, ntok, dim)
    assert tuple(out["cls"].shape) == (n, n_img, dim) and tuple(out["pooled"].shape) == (n, n_img, 3 * dim)
    assert len(want) == n
    for k in range(n):
        what = f"{_case_id(case)} {precision} tap {k} (block {DEPTH - n + k})"
        assert_close(out["tokens"][k], want[k], f"{what} tokens")
        assert_close(out["cls"][k], want[k][:, 0], f"{what} cls")
        assert_close(out["pooled"][k], vit_layers_ref.pooled(want[k]), f"{what} pooled")
    if ntok == 2:
        assert float(out["pooled"][:, :, 2 * dim:].abs().max()) == 0.0, "the std over one token is not 0"
        assert torch.equal(out["pooled"][:, :, :dim], out["pooled"][:, :, dim:2 * dim]), "mean and max over one token differ"


# ---- distance from fp64 ----------------------------------------------------------------------------------------------------------------
PARITY_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _record_parity():
    yield
    out = os.environ.get("RELAX_VIT_LAYERS_PARITY_OUT")
    if out and PARITY_SEEN:
        with open(out, "w") as f:
            json.dump({"what": "per tap: (|GPU - fp64| / |torch-CPU fp32 - fp64|), relative Frobenius distances over the tap's normed tokens "
                               "[N, ntok, dim]; 'final': the same ratio for vit_features' tokens (the existing path) in the same test; gate: "
                               "every tap <= 2 x final", "cases": PARITY_SEEN}, f, indent=1, sort_keys=True)


def _rel(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / np.linalg.norm(ref))


FP64_CASES = [("vit_small", 16, False, 3, 224, 224, 12), ("vit_base", 16, False, 2, 224, 224, 4)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", FP64_CASES, ids=[_case_id(c) for c in FP64_CASES])
def test_taps_are_as_far_from_fp64_as_the_final_tokens(case, precision):
    """The distance measure is the relative Frobenius norm over a tap's tokens (a maximum would hang on one element).  Yardstick of a tap: how far
    torch's own fp32 forward is from the fp64 one at that tap.  Gate (set before any run): a tap's ratio <= 2 x the ratio of the final tokens
    obtained through vit_features in this same test - a tap has passed through no more blocks than the final output; the factor 2 covers
    early-block rows whose pre-norm scale differs."""
    name, patch, adversarial, n_img, Hc, Wc, n = case
    _load(name, patch, adversarial)
    imgs, t32 = _reference(*case)
    _, t64 = _reference(*case, fp64=True)
    eng = engine()
    eng.set_precision(precision)
    got = eng.vit_intermediate_layers(imgs, n=n, tokens=True, cls=False, pooled=False)["tokens"].cpu().numpy()
    final = eng.vit_features(imgs, tokens=True, pooled=False)[0].cpu().numpy()
    final_ratio = _rel(final, t64[-1][:, 1:]) / _rel(t32[-1][:, 1:], t64[-1][:, 1:])
    ratios = [_rel(got[k], t64[k]) / _rel(t32[k], t64[k]) for k in range(n)]
    PARITY_SEEN[f"{_case_id(case)} {precision}"] = {"final": round(final_ratio, 4), "taps": [round(r, 4) for r in ratios],
                                                    "cpu_fp32_vs_fp64": [float(f"{_rel(t32[k], t64[k]):.3e}") for k in range(n)]}
    print(f"\n{_case_id(case)} {precision}: final {final_ratio:.3f}, taps " + " ".join(f"{r:.3f}" for r in ratios))
    for k, r in enumerate(ratios):
        assert r <= 2 * final_ratio, f"tap {k} (block {DEPTH - n + k}): ratio {r:.3f} against the final tokens' {final_ratio:.3f}"


# ---- bit identities --------------------------------------------------------------------------------------------------------------------
# (model, images, Hc, Wc): dim 768 (f16x2's own branch) at 197 tokens, dim 192 at 16 tokens and at 2, dim 384 at 7
BIT_CASES = [("vit_base", 3, 224, 224), ("vit_tiny", 3, 48, 80), ("vit_tiny", 3, 16, 16), ("vit_small", 3, 32, 48)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,n_img,Hc,Wc", BIT_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in BIT_CASES])
def test_bit_identities(name, n_img, Hc, Wc, precision):
    _load(name)
    eng = engine()
    eng.set_precision(precision)
    imgs = torch.from_numpy(_images(n_img, Hc, Wc)).cuda()
    before = eng.vit_features(imgs, tokens=True, pooled=True)
    full = eng.vit_intermediate_layers(imgs, n=DEPTH, tokens=True, cls=True, pooled=True)
    tok, cls, pooled = full["tokens"], full["cls"], full["pooled"]
    # the last tap is the forward's own norm: layernorm_rows + vit_token_stats against the fused kernel
    assert torch.equal(tok[-1][:, 1:], before[0]), "tokens[-1][:, 1:] differs from vit_features(tokens=True)"
    assert torch.equal(pooled[-1], before[1]), "pooled[-1] differs from vit_features(pooled=True)"
    for k in range(DEPTH):
        assert torch.equal(cls[k], tok[k][:, 0]), f"tap {k}: cls differs from tokens[:, 0]"
        assert torch.equal(pooled[k], eng.op_token_stats(tok[k][:, 1:].contiguous())), f"tap {k}: pooled differs from op_token_stats(tokens)"
    # outputs requested alone
    for key in ("tokens", "cls", "pooled"):
        alone = eng.vit_intermediate_layers(imgs, n=DEPTH, tokens=key == "tokens", cls=key == "cls", pooled=key == "pooled")
        assert list(alone) == [key] and torch.equal(alone[key], full[key]), f"{key} requested alone differs"
    # a second call
    again = eng.vit_intermediate_layers(imgs, n=DEPTH, tokens=True, cls=True, pooled=True)
    assert all(torch.equal(again[key], full[key]) for key in full), "a second call differs"
    # n = 4 is the last four taps of n = 12
    four = eng.vit_intermediate_layers(imgs, n=4, tokens=True, cls=True, pooled=True)
    for key in full:
        assert four[key].shape[0] == 4 and torch.equal(four[key], full[key][8:]), f"{key}: taps of n=4 differ from taps 8.. of n=12"
    # no row depends on its batch (with the GEMMs' tail split off, as in every batch-composition identity of this suite: the split cuts the
    # last tiles of a GEMM along K by the row count, engine.clip_vectors' docstring)
    eng.set_option("gemm_split_k", 0)
    try:
        batch = eng.vit_intermediate_layers(imgs, n=DEPTH, tokens=True, cls=True, pooled=True)
        for i in range(n_img):
            one = eng.vit_intermediate_layers(imgs[i:i + 1], n=DEPTH, tokens=True, cls=True, pooled=True)
            for key in full:
                assert torch.equal(one[key][:, 0], batch[key][:, i]), f"{key}: image {i} alone differs from image {i} of the batch"
    finally:
        eng.set_option("gemm_split_k", 1)
    # the taps leave nothing behind
    after = eng.vit_features(imgs, tokens=True, pooled=True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]), "vit_features changed after a tapped call"


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------
# (images, ntok, dim): every dim launch_layernorm's ViTs have; 2 and 4 tokens (empty token groups), 5 (one patch per group), 18 (more rows
# than waves by two), 785, and the limit 4097.  The image counts walk the launcher's channel slices (csrc/vit_layers.hip: tap_slices): few
# images share an image among 4 workgroups (dim 768), 3 (dim 384 / 192); 256 and 300 images among 2; 515 images run one workgroup per image;
# 13, 300 and 515 are no multiples of the 8 images a round of workgroup ids covers
OP_CASES = [(3, 2, 192), (2, 4, 384), (2, 5, 768), (3, 18, 192), (2, 197, 768), (2, 785, 384), (1, 4097, 768), (2, 4097, 192),
            (13, 18, 384), (256, 5, 768), (300, 6, 384), (515, 3, 192), (515, 9, 768)]


@pytest.mark.parametrize("n_img,ntok,dim", OP_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in OP_CASES])
def test_fused_kernel_is_layernorm_then_token_stats(n_img, ntok, dim):
    """bit for bit against the two launches it replaces, on rows with a mean and a scale of their own (the residual stream's are far from 0 / 1),
    and against numpy in fp64 to fp32 rounding"""
    eng = engine()
    g = torch.Generator().manual_seed(ntok * 1000 + dim)
    x = (torch.randn((n_img, ntok, dim), generator=g) * (1 + 3 * torch.rand((n_img, ntok, 1), generator=g)) + 2 * torch.randn((n_img, ntok, 1), generator=g)).cuda()
    gamma, beta = (1 + 0.2 * torch.randn(dim, generator=g)).cuda(), (0.3 * torch.randn(dim, generator=g)).cuda()
    y = eng.op_layernorm(x.reshape(-1, dim), gamma, beta, 1e-6).reshape(n_img, ntok, dim)
    want_pooled = eng.op_token_stats(y[:, 1:].contiguous())
    cls, pooled = eng.op_vit_norm_token_stats(x, gamma, beta, 1e-6)
    assert torch.equal(cls, y[:, 0]), "the CLS row differs from layernorm_rows'"
    assert torch.equal(pooled, want_pooled), "the statistics differ from vit_token_stats of layernorm_rows' output"
    assert torch.equal(eng.op_vit_norm_token_stats(x, gamma, beta, 1e-6, pooled=False)[0], cls)
    assert torch.equal(eng.op_vit_norm_token_stats(x, gamma, beta, 1e-6, cls=False)[1], pooled)
    x64 = x.double().cpu()
    y64 = torch.nn.functional.layer_norm(x64, (dim,), gamma.double().cpu(), beta.double().cpu(), 1e-6).numpy()
    assert_close(cls, y64[:, 0], "cls against fp64")
    assert_close(pooled, vit_layers_ref.pooled(y64), "pooled against fp64")


def test_fused_kernel_refuses_what_it_cannot_hold():
    eng = engine()
    z = torch.zeros((1, 2, 64), device="cuda")
    v = torch.zeros(1024, device="cuda")
    for shape, word in (((1, 1, 64), "ntok=1"), ((1, 4098, 64), "ntok=4098"), ((1, 2, 832), "dim=832"), ((1, 2, 96), "dim=96")):
        with pytest.raises(RuntimeError, match=word):
            eng.op_vit_norm_token_stats(z.new_zeros(shape), v, v, 1e-6)
    with pytest.raises(RuntimeError, match="bad arguments"):
        eng.op_vit_norm_token_stats(z, v, v, 1e-6, cls=False, pooled=False)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value():
    _load("vit_tiny")
    eng = engine()
    imgs = _images(1, 32, 32)
    with pytest.raises(RuntimeError, match=r"n_last=0\b"):
        eng.vit_intermediate_layers(imgs, n=0)
    with pytest.raises(RuntimeError, match=r"n_last=13\b.*\b12\b"):
        eng.vit_intermediate_layers(imgs, n=DEPTH + 1)
    with pytest.raises(RuntimeError, match=r"n_last=-1\b"):
        eng.vit_intermediate_layers(imgs, n=-1)
    with pytest.raises(ValueError, match="no output"):
        eng.vit_intermediate_layers(imgs, n=1, tokens=False, cls=False, pooled=False)
    rc = eng.lib.relax_vit_intermediate_layers(eng.h, C.c_void_p(16), 1, 32, 32, 1, None, None, None, None)
    assert rc != 0 and b"relax_vit_intermediate_layers: no output" in eng.lib.relax_last_error(eng.h)
    with pytest.raises(RuntimeError, match=r"\b15\b"):
        eng.vit_intermediate_layers(np.zeros((1, 15, 300, 3), dtype=np.uint8))
    out = torch.empty((1, 1, 192), dtype=torch.float32, device="cuda")
    rc = eng.lib.relax_vit_intermediate_layers(eng.h, C.c_void_p(16), 1, 15, 300, 1, None, out.data_ptr(), None, None)
    msg = eng.lib.relax_last_error(eng.h)
    assert rc != 0 and b"relax_vit_intermediate_layers" in msg and b"15" in msg, msg
    # and the engine still works
    assert tuple(eng.vit_intermediate_layers(imgs, n=2)["cls"].shape) == (2, 1, 192)


# ---- Python surface --------------------------------------------------------------------------------------------------------------------
def test_fragment_vit_layer_stack():
    _load("vit_tiny")
    eng = engine()
    dim = 192
    clip = torch.from_numpy(synth.synthetic_clip(2, 240, 320, clip_id=6)).cuda()
    assert torch.equal(eng.fragment_vit_layer_stack(clip, n=1), eng.fragment_vit_vectors(clip))
    rows = eng.fragment_vit_layer_stack(clip, n=4, cls=True)
    assert tuple(rows.shape) == (2, 2 * 4 * 3 * dim + 2 * 4 * dim) and rows.dtype == torch.float32
    # the layout: per fragment (original, then difference) the taps in block order, each cls | pooled
    fr = eng.fragment_pairs(clip, top_n=None, patch_size=16, target_size=224)
    for j, key in enumerate(("ori_frag", "diff_frag")):
        taps = eng.vit_intermediate_layers(fr[key], n=4, cls=True, pooled=True)
        block = rows[:, j * 16 * dim:(j + 1) * 16 * dim].reshape(2, 4, 4 * dim)
        for k in range(4):
            assert_close(block[:, k, :dim], taps["cls"][k].cpu().numpy(), f"{key} tap {k} cls columns")
            assert_close(block[:, k, dim:], taps["pooled"][k].cpu().numpy(), f"{key} tap {k} pooled columns")
    plain = eng.fragment_vit_layer_stack(clip, n=4)
    assert tuple(plain.shape) == (2, 2 * 4 * 3 * dim)
    assert torch.equal(plain[:, 9 * dim:12 * dim], eng.fragment_vit_vectors(clip)[:, :3 * dim]), "the last tap is not fragment_vit_vectors' pool"


def test_vit_generator_intermediate_layers():
    from relax_vqa_amd import runtime
    from relax_vqa_amd.extractor import visualise_vit_layer
    try:
        model = visualise_vit_layer.VitGenerator("vit_tiny", 16, None, random=True)
        img = _images(2, 48, 80)
        layers = model.get_intermediate_layers(img, n=3)
        assert isinstance(layers, list) and len(layers) == 3 and all(tuple(t.shape) == (2, 16, 192) for t in layers)
        eng = runtime.ensure_vit("vit_tiny", 16)
        want = eng.vit_intermediate_layers(img, n=3, tokens=True, cls=False, pooled=False)["tokens"]
        for k in range(3):
            assert torch.equal(layers[k], want[k])
        cls = model.cls_token(img)
        assert tuple(cls.shape) == (2, 192) and torch.equal(cls, want[-1][:, 0])
        assert len(model.get_intermediate_layers(img)) == 1
        none, tokens = model(img)                                           # __call__ and tokens are what they were
        assert none is None and torch.equal(tokens, want[-1][:, 1:])
    finally:
        runtime.set_weights(vit=synth.vit_state_dict("vit_base"), vit_name="vit_base")   # what the other host-API tests run on
