"""-m gpu: ResNet-50 on any accepted canvas (relax_resnet50_set_canvas; RelaxEngine.resnet50_features_canvas and the methods on top of it)
against oracle/resnet50_ref.py, which restates torchvision's model and takes any size.  The canvases are the smallest at which each piece can
go wrong: 64 x 64 (layer4 is 2 x 2, four stem tiles per image, layer1 at the back-to-back bound), 64 x 96 and 96 x 64 (the same pixels
transposed: any H / W swap), 96 x 160 (layer3 60 rows, layer4 15: no group of four), 288 x 512 (the whole-frame canvas), 448 x 448 (the
fragment canvas), 1024 x 64 (the limit on one side); 224 x 224 must be resnet50_features itself, launch for launch and bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import pooling_ref, resnet50_ref
from tests import stream_cases as sc
from tests.gpu_common import assert_close, engine, launches, rn50_weights, synth
from tests.test_gpu_stream_contract import run_held

pytestmark = pytest.mark.gpu

CANVASES = [(3, 64, 64), (2, 64, 96), (2, 96, 64), (2, 96, 160), (1, 288, 512), (1, 448, 448), (1, 1024, 64)]
_ref = {}


def _images(n, Hc, Wc, seed=0):
    """n uint8 [Hc,Wc,3] images: a synthetic frame tiled over the canvas (image content, not noise) plus a ramp that makes every tile differ"""
    out = []
    for i in range(n):
        f = synth.synthetic_pair(240, 320, 900 + 16 * seed + i)[0]
        f = np.tile(f, (-(-Hc // 240), -(-Wc // 320), 1))[:Hc, :Wc].astype(np.int32)
        ramp = (np.arange(Hc)[:, None] * 3 + np.arange(Wc)[None, :] * 5) // 16
        out.append(((f + ramp[..., None]) % 256).astype(np.uint8))
    return np.stack(out)


def _reference(adversarial, n, Hc, Wc, seed=0):
    """(images, taps fp32 [15], layer stack, pool) of the oracle: computed once per case and shared"""
    key = (adversarial, n, Hc, Wc, seed)
    if key not in _ref:
        tsd = resnet50_ref.to_torch_state_dict(synth.resnet50_state_dict(adversarial=adversarial) if adversarial else rn50_weights())
        imgs = _images(n, Hc, Wc, seed)
        taps, _ = resnet50_ref.forward_taps(tsd, resnet50_ref.preprocess_bgr_u8(imgs))
        _ref[key] = (imgs, [taps[name].numpy() for name in pooling_ref.RESNET50_TAPS], resnet50_ref.layer_stack_features(tsd, imgs),
                     resnet50_ref.pool_features(tsd, imgs))
    return _ref[key]


def _check_parity(got, ref, where):
    ls, pool, taps = got
    _, ref_taps, want_ls, want_pool = ref
    for i, name in enumerate(pooling_ref.RESNET50_TAPS):
        assert_close(taps[i], ref_taps[i], f"{where} {name}", channel_axis=1)
    off = 0
    for name, c in zip(pooling_ref.RESNET50_TAPS, pooling_ref.RESNET50_TAP_CHANNELS):
        assert_close(ls[:, off:off + c], want_ls[:, off:off + c], f"{where} layer-stack block {name}")
        off += c
    assert_close(pool[:, :2048], want_pool[:, :2048], f"{where} pool vector")
    assert_close(pool[:, 2048:], want_pool[:, 2048:], f"{where} pool stats (mean,max,std)")


def test_the_default_canvas_is_resnet50_features_itself(each_precision):
    rn50_weights()
    eng = engine()
    x = torch.from_numpy(_images(3, 224, 224)).cuda()
    (ls0, pool0, taps0), n0 = launches(eng, lambda: eng.resnet50_features(x, taps=range(15)))
    (ls1, pool1, taps1), n1 = launches(eng, lambda: eng.resnet50_features_canvas(x, taps=range(15)))
    assert n0 == n1 and sum(n0.values()) > 0, (n0, n1)
    assert torch.equal(ls0, ls1) and torch.equal(pool0, pool1)
    for t in range(15):
        assert torch.equal(taps0[t], taps1[t]), f"tap {t}"
    assert eng.resnet50_canvas() == (224, 224)


@pytest.mark.parametrize("case", CANVASES, ids=lambda c: "%dx%dx%d" % c)
def test_every_tap_and_both_rows_match_the_oracle(each_precision, case):
    n, Hc, Wc = case
    ref = _reference(False, n, Hc, Wc)
    rn50_weights()
    eng = engine()
    shapes, arena = eng.resnet50_canvas_geometry(Hc, Wc)
    got = eng.resnet50_features_canvas(torch.from_numpy(ref[0]).cuda(), taps=range(15))
    torch.cuda.synchronize()
    assert [tuple(got[2][t].shape[2:]) for t in range(15)] == shapes and arena > 0
    _check_parity(got, ref, f"{Hc}x{Wc}")
    assert eng.resnet50_canvas() == (224, 224)


def test_transposed_canvases_differ_and_each_matches_its_own_oracle(each_precision):
    """64 x 96 and 96 x 64 from the same pixels: a swap of H and W anywhere gives one of them the other's maps"""
    rn50_weights()
    eng = engine()
    a = _images(2, 64, 96, seed=3)
    b = np.ascontiguousarray(a.transpose(0, 2, 1, 3))
    tsd = resnet50_ref.to_torch_state_dict(rn50_weights())
    outs = []
    for imgs in (a, b):
        ls, pool, taps = eng.resnet50_features_canvas(torch.from_numpy(imgs).cuda(), taps=range(15))
        ref_taps, _ = resnet50_ref.forward_taps(tsd, resnet50_ref.preprocess_bgr_u8(imgs))
        for i, name in enumerate(pooling_ref.RESNET50_TAPS):
            assert_close(taps[i], ref_taps[name].numpy(), f"{imgs.shape[1:3]} {name}", channel_axis=1)
        outs.append((ls, pool))
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("adversarial", [True, "outliers"], ids=["adversarial", "outliers"])
def test_the_other_weight_sets_at_96x160(each_precision, adversarial):
    ref = _reference(adversarial, 2, 96, 160)
    rn50_weights(adversarial)
    try:
        got = engine().resnet50_features_canvas(torch.from_numpy(ref[0]).cuda(), taps=range(15))
        _check_parity(got, ref, f"96x160 {adversarial}")
    finally:
        rn50_weights()   # the shared engine goes back to the regular set


def test_same_bits_on_a_second_call_and_in_any_batch(each_precision):
    rn50_weights()
    eng = engine()
    x = torch.from_numpy(_images(3, 64, 96, seed=5)).cuda()
    first = eng.resnet50_features_canvas(x, taps=range(15))
    again = eng.resnet50_features_canvas(x, taps=range(15))
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert all(torch.equal(first[2][t], again[2][t]) for t in range(15))
    eng.set_option("gemm_split_k", 0)
    try:
        ls3, pool3, taps3 = eng.resnet50_features_canvas(x, taps=range(15))
        ls1, pool1, taps1 = eng.resnet50_features_canvas(x[1:2], taps=range(15))
        assert torch.equal(ls1[0], ls3[1]) and torch.equal(pool1[0], pool3[1]), "result depends on the batch"
        assert all(torch.equal(taps1[t][0], taps3[t][1]) for t in range(15))
    finally:
        eng.set_option("gemm_split_k", 1)


# ---- distance from fp64 ----------------------------------------------------------------------------------------------------------------
PARITY_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _record_parity():
    yield
    out = os.environ.get("RELAX_RESNET_CANVAS_PARITY_OUT")
    if out and PARITY_SEEN:
        with open(out, "w") as f:
            json.dump({"what": "per tap: |GPU - fp64| / |torch-CPU fp32 - fp64|, relative Frobenius distances over the tap [N,C,h,w] of "
                               "oracle/resnet50_ref.py run in fp64 and in fp32; gate: every ratio <= 2", "cases": PARITY_SEEN}, f, indent=1, sort_keys=True)


def _rel(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("case", [(2, 96, 160), (1, 448, 448)], ids=lambda c: "%dx%dx%d" % c)
def test_taps_are_as_close_to_fp64_as_torch_fp32_is(each_precision, case):
    """fp32-grade: a tap is at most twice as far from the fp64 oracle as torch's own CPU fp32 forward is (1.2e-6 - 1.4e-6 norm-relative on these
    weights).  The bound is the one tests/test_gpu_vit_layers.py and the flow tests hold their kernels to; it was set before any run."""
    n, Hc, Wc = case
    imgs, taps32, _, _ = _reference(False, n, Hc, Wc)
    tsd = resnet50_ref.to_torch_state_dict(rn50_weights())
    taps64, _ = resnet50_ref.forward_taps({k: v.double() for k, v in tsd.items()}, resnet50_ref.preprocess_bgr_u8(imgs).double())
    _, _, got = engine().resnet50_features_canvas(torch.from_numpy(imgs).cuda(), taps=range(15))
    ratios, cpu = [], []
    for i, name in enumerate(pooling_ref.RESNET50_TAPS):
        t64 = taps64[name].numpy()
        cpu.append(_rel(taps32[i], t64))
        ratios.append(_rel(got[i].cpu().numpy(), t64) / cpu[-1])
    PARITY_SEEN[f"{Hc}x{Wc} N={n} {each_precision}"] = {"taps": [round(r, 4) for r in ratios], "cpu_fp32_vs_fp64": [float(f"{c:.3e}") for c in cpu]}
    print(f"\n{Hc}x{Wc} {each_precision}: " + " ".join(f"{r:.3f}" for r in ratios))
    for name, r in zip(pooling_ref.RESNET50_TAPS, ratios):
        assert r <= 2.0, f"{name}: {r:.3f} x torch-CPU fp32's distance from fp64"


# ---- state -----------------------------------------------------------------------------------------------------------------------------
def test_the_canvas_is_224_again_after_a_call_that_raises():
    rn50_weights()
    eng = engine()
    x = torch.from_numpy(_images(1, 64, 96)).cuda()
    with pytest.raises(IndexError):
        eng.resnet50_features_canvas(x, taps=[99])
    assert eng.resnet50_canvas() == (224, 224)
    with pytest.raises(ValueError, match=r"canvas width 100 is not a multiple of 32 in \[64, 1024\] \(canvas 64 x 100\)"):
        eng.resnet50_features_canvas(torch.zeros((1, 64, 100, 3), dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="canvas height 230 "):
        eng.resnet50_clip_features_canvas(torch.zeros((2, 230, 224, 3), dtype=torch.uint8).cuda(), 1)
    assert eng.resnet50_canvas() == (224, 224)
    with pytest.raises(ValueError, match=r"fragments must be \[N,224,224,3\]"):       # the 224 methods keep their message
        eng.resnet50_features(x)


def test_a_refused_canvas_leaves_the_previous_one_and_names_the_value():
    rn50_weights()
    eng = engine()
    assert eng.lib.relax_resnet50_set_canvas(eng.h, 96, 160) == 0
    try:
        for Hc, Wc, words in ((96, 232, "canvas width 232 "), (0, 160, "canvas height 0 "), (-64, 64, "canvas height -64 "), (1056, 64, "canvas height 1056 ")):
            assert eng.lib.relax_resnet50_set_canvas(eng.h, Hc, Wc) != 0
            msg = eng.lib.relax_last_error(eng.h).decode()
            assert words in msg and f"(canvas {Hc} x {Wc})" in msg, msg
            assert eng.resnet50_canvas() == (96, 160)
    finally:
        assert eng.lib.relax_resnet50_set_canvas(eng.h, 224, 224) == 0
    eng.load_resnet50(rn50_weights())          # a load puts the default canvas back
    eng.lib.relax_resnet50_set_canvas(eng.h, 64, 64)
    eng.load_resnet50(rn50_weights())
    assert eng.resnet50_canvas() == (224, 224)


def test_clip_vectors_do_not_notice_a_canvas_call(each_precision):
    from tests.gpu_common import vit_weights
    rn50_weights()
    vit_weights("vit_base")
    eng = engine()
    clips = [torch.from_numpy(synth.synthetic_clip(2, 240, 320, clip_id=11)).cuda()]
    before = eng.clip_vectors(clips)
    eng.resnet50_features_canvas(torch.from_numpy(_images(1, 96, 160)).cuda())
    after = eng.clip_vectors(clips)
    assert torch.equal(before, after)


# ---- the methods on top ------------------------------------------------------------------------------------------------------------------
def _pair_clip():
    return torch.from_numpy(np.stack([np.stack(synth.synthetic_pair(240, 320, 40 + i)) for i in range(2)])).cuda()     # [2,2,240,320,3]


def test_fragment_resnet_vectors_and_fragment_canvas_vectors(each_precision):
    from tests.gpu_common import vit_weights
    rn50_weights()
    vit_weights("vit_base")
    eng = engine()
    clip = _pair_clip()
    # 224: the clip path's own row, bit for bit
    assert torch.equal(eng.fragment_resnet_vectors(clip), eng.extract_clip(clip, vit=False)["resnet"])
    # 448: ResNet-50 at that canvas on fragment_pairs' own fragments
    rows = eng.fragment_resnet_vectors(clip, target_size=448)
    assert tuple(rows.shape) == (2, 13120 + 2051) and rows.dtype == torch.float32
    fr = eng.fragment_pairs(clip, top_n=None, target_size=448)           # (every slot of the canvas, as the method cuts it)
    ls, pool = eng.resnet50_clip_features_canvas(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), 2)
    assert torch.equal(rows, torch.cat([ls, pool], dim=1))
    ref_ls = resnet50_ref.layer_stack_features(resnet50_ref.to_torch_state_dict(rn50_weights()), fr["ori_frag"].cpu().numpy())
    assert_close(rows[:, :13120], ref_ls, "448 fragment layer stack")
    both = eng.fragment_canvas_vectors(clip, 448)
    assert torch.equal(both, torch.cat([rows, eng.fragment_vit_vectors(clip, target_size=448)], dim=1))
    with pytest.raises(ValueError, match="canvas height 232 "):      # a fragment canvas at patch 8, not a ResNet-50 one
        eng.fragment_resnet_vectors(clip, patch_size=8, target_size=232)
    assert eng.resnet50_canvas() == (224, 224)


def test_whole_frame_resnet_canvas_is_the_features_of_a_pillow_resize(each_precision):
    from PIL import Image
    rn50_weights()
    eng = engine()
    frames = np.stack([synth.synthetic_pair(360, 640, 70 + i)[0] for i in range(2)])
    got = eng.whole_frame_resnet_canvas(torch.from_numpy(frames).cuda(), (288, 512))
    host = np.stack([np.asarray(Image.fromarray(f).resize((512, 288), Image.BILINEAR)) for f in frames])
    want = eng.resnet50_features_canvas(torch.from_numpy(host).cuda())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    by_side = eng.whole_frame_resnet_canvas(torch.from_numpy(frames).cuda(), 288)            # the shorter-side rule: 360 x 640 -> 288 x 512
    assert torch.equal(by_side[0], got[0])
    with pytest.raises(ValueError, match="canvas height 270 "):
        eng.whole_frame_resnet_canvas(torch.from_numpy(frames).cuda(), (270, 480))


# ---- stream ------------------------------------------------------------------------------------------------------------------------------
def test_a_canvas_call_stays_on_a_held_side_stream(each_precision):
    """One call at 96 x 160 on a non-blocking side stream that is held: the bits of the default stream's call, and the call returns while the
    stream is still blocked (the helper of tests/test_gpu_stream_contract.py)."""
    def make(seed):
        return {"images": torch.from_numpy(_images(2, 96, 160, seed=20 + seed)).cuda()}

    def call(eng, t):
        ls, pool, taps = eng.resnet50_features_canvas(t["images"], taps=(0, 7, 14))
        return ls, pool, taps[0], taps[7], taps[14]

    case = sc.Case("enqueue", make, call, precisions=sc.PRECISIONS, needs=("rn50",))
    rep = run_held(case, f"resnet50_features_canvas 96x160 {each_precision}")
    assert not rep.mismatch, f"outputs {rep.mismatch} on the held side stream differ from the default stream's"
    assert rep.still_held, "the call returned only after its stream's hold had run out: it waited"
