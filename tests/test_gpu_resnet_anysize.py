"""-m gpu: ResNet-50 on EVERY canvas size (relax_resnet50_set_canvas_ex with RELAX_RN_CANVAS_ANY; the any_size=True keyword of
RelaxEngine.resnet50_features_canvas and the methods on top of it) against oracle/resnet50_ref.py, which restates torchvision's model and takes
any size.  The canvases are the smallest that reach every new edge: 65 x 67 (all five maps odd, image bases at every byte alignment in a batch
of 5, a stem edge tile 1 pixel wide and 1 pixel high in the 33 x 34 output), 70 x 100, 95 x 98 (odd input width with an even 48-row stem map:
whole tiles one way, 3 tiles + 1 column the other), 230 x 232 (the patch-8 fragment canvas), 270 x 480 (1080p / 4), 1023 x 65 (the long side
near the limit): a partial tile in each direction, an odd pool input in each direction, an odd stride-2 input at each of layer2, layer3 and
layer4, and HW % 4 != 0 on every tap."""
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

CANVASES = [(5, 65, 67), (2, 70, 100), (2, 95, 98), (1, 230, 232), (1, 270, 480), (1, 1023, 65)]
ANY = 1                  # RELAX_RN_CANVAS_ANY
_ref = {}


def _images(n, Hc, Wc, seed=0):
    """n uint8 [Hc,Wc,3] images: a synthetic frame tiled over the canvas (image content, not noise) plus a ramp that makes every tile differ"""
    out = []
    for i in range(n):
        f = synth.synthetic_pair(240, 320, 700 + 16 * seed + i)[0]
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
        assert tuple(taps[i].shape) == ref_taps[i].shape, (where, name, tuple(taps[i].shape), ref_taps[i].shape)
        assert_close(taps[i], ref_taps[i], f"{where} {name}", channel_axis=1)
    off = 0
    for name, c in zip(pooling_ref.RESNET50_TAPS, pooling_ref.RESNET50_TAP_CHANNELS):
        assert_close(ls[:, off:off + c], want_ls[:, off:off + c], f"{where} layer-stack block {name}")
        off += c
    assert_close(pool[:, :2048], want_pool[:, :2048], f"{where} pool vector")
    assert_close(pool[:, 2048:], want_pool[:, 2048:], f"{where} pool stats (mean,max,std)")


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][t], b[2][t]) for t in a[2])


# ---- parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CANVASES, ids=lambda c: "%dx%dx%d" % c)
def test_every_tap_and_both_rows_match_the_oracle(each_precision, case):
    n, Hc, Wc = case
    ref = _reference(False, n, Hc, Wc)
    rn50_weights()
    eng = engine()
    shapes, arena = eng.resnet50_canvas_geometry(Hc, Wc, any_size=True)
    got = eng.resnet50_features_canvas(torch.from_numpy(ref[0]).cuda(), taps=range(15), any_size=True)
    torch.cuda.synchronize()
    assert [tuple(got[2][t].shape[2:]) for t in range(15)] == shapes and arena > 0
    _check_parity(got, ref, f"{Hc}x{Wc}")
    assert eng.resnet50_canvas() == (224, 224)


@pytest.mark.parametrize("adversarial", [True, "outliers"], ids=["adversarial", "outliers"])
def test_the_other_weight_sets_at_70x100(each_precision, adversarial):
    ref = _reference(adversarial, 2, 70, 100)
    rn50_weights(adversarial)
    try:
        got = engine().resnet50_features_canvas(torch.from_numpy(ref[0]).cuda(), taps=range(15), any_size=True)
        _check_parity(got, ref, f"70x100 {adversarial}")
    finally:
        rn50_weights()   # the shared engine goes back to the regular set


# ---- distance from fp64 ----------------------------------------------------------------------------------------------------------------
PARITY_SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _record_parity():
    yield
    out = os.environ.get("RELAX_RESNET_ANYSIZE_PARITY_OUT")
    if out and PARITY_SEEN:
        with open(out, "w") as f:
            json.dump({"what": "per tap: |GPU - fp64| / |torch-CPU fp32 - fp64|, relative Frobenius distances over the tap [N,C,h,w] of "
                               "oracle/resnet50_ref.py run in fp64 and in fp32, canvases under RELAX_RN_CANVAS_ANY; gate: every ratio <= 2",
                       "cases": PARITY_SEEN}, f, indent=1, sort_keys=True)


def _rel(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("case", [(5, 65, 67), (1, 230, 232)], ids=lambda c: "%dx%dx%d" % c)
def test_taps_are_as_close_to_fp64_as_torch_fp32_is(each_precision, case):
    """fp32-grade: a tap is at most twice as far from the fp64 oracle as torch's own CPU fp32 forward is - the gate of
    tests/test_gpu_resnet_canvas.py, set before any run."""
    n, Hc, Wc = case
    imgs, taps32, _, _ = _reference(False, n, Hc, Wc)
    tsd = resnet50_ref.to_torch_state_dict(rn50_weights())
    key = ("fp64", n, Hc, Wc)
    if key not in _ref:
        taps64, _ = resnet50_ref.forward_taps({k: v.double() for k, v in tsd.items()}, resnet50_ref.preprocess_bgr_u8(imgs).double())
        _ref[key] = [taps64[name].numpy() for name in pooling_ref.RESNET50_TAPS]
    _, _, got = engine().resnet50_features_canvas(torch.from_numpy(imgs).cuda(), taps=range(15), any_size=True)
    ratios, cpu = [], []
    for i, name in enumerate(pooling_ref.RESNET50_TAPS):
        t64 = _ref[key][i]
        cpu.append(_rel(taps32[i], t64))
        ratios.append(_rel(got[i].cpu().numpy(), t64) / cpu[-1])
    PARITY_SEEN[f"{Hc}x{Wc} N={n} {each_precision}"] = {"taps": [round(r, 4) for r in ratios], "cpu_fp32_vs_fp64": [float(f"{c:.3e}") for c in cpu]}
    print(f"\n{Hc}x{Wc} {each_precision}: " + " ".join(f"{r:.3f}" for r in ratios))
    for name, r in zip(pooling_ref.RESNET50_TAPS, ratios):
        assert r <= 2.0, f"{name}: {r:.3f} x torch-CPU fp32's distance from fp64"


# ---- bits ----------------------------------------------------------------------------------------------------------------------------------
def test_an_image_has_the_bits_it_gets_alone_and_a_second_call_the_bits_of_the_first(each_precision):
    """65 x 67, N = 5: image i starts at byte 13065 i - every alignment mod 4 - and alone it starts at the tensor's base.  The per-image maxima of
    the max-pool come from ragged blocks (and the convolutions' from integer atomics): a second call must post the same words."""
    rn50_weights()
    eng = engine()
    x = torch.from_numpy(_images(5, 65, 67, seed=5)).cuda()
    eng.set_option("gemm_split_k", 0)       # (the tail split cuts a GEMM along K by the batch size: tests/test_gpu_resnet_canvas.py does the same)
    try:
        first = eng.resnet50_features_canvas(x, taps=range(15), any_size=True)
        again = eng.resnet50_features_canvas(x, taps=range(15), any_size=True)
        assert _same(first, again), "a second call gave other bits"
        for i in range(5):
            ls1, pool1, taps1 = eng.resnet50_features_canvas(x[i:i + 1].clone(), taps=range(15), any_size=True)
            assert torch.equal(ls1[0], first[0][i]) and torch.equal(pool1[0], first[1][i]), f"rows of image {i} depend on the batch"
            for t in range(15):
                assert torch.equal(taps1[t][0], first[2][t][i]), f"tap {t} of image {i} depends on the batch"
            # the same image read in place, at its own (mis)alignment inside the batch
            ls2, pool2 = eng.resnet50_features_canvas(x[i:i + 1], any_size=True)
            assert torch.equal(ls2[0], first[0][i]) and torch.equal(pool2[0], first[1][i]), f"image {i} read in place"
    finally:
        eng.set_option("gemm_split_k", 1)
    again = eng.resnet50_features_canvas(x, taps=range(15), any_size=True)
    assert _same(again, eng.resnet50_features_canvas(x, taps=range(15), any_size=True)), "a second call gave other bits (tail split on)"


@pytest.mark.parametrize("canvas", [(96, 160), (224, 224)], ids=lambda c: "%dx%d" % c)
def test_an_old_canvas_under_the_new_rule_runs_the_old_launches(each_precision, canvas):
    rn50_weights()
    eng = engine()
    x = torch.from_numpy(_images(2, *canvas, seed=2)).cuda()
    old, n_old = launches(eng, lambda: eng.resnet50_features_canvas(x, taps=range(15)))
    new, n_new = launches(eng, lambda: eng.resnet50_features_canvas(x, taps=range(15), any_size=True))
    assert n_old == n_new and sum(n_old.values()) > 0, (n_old, n_new)
    assert _same(old, new)


# ---- state -----------------------------------------------------------------------------------------------------------------------------
def test_a_refused_ex_canvas_leaves_the_previous_one():
    rn50_weights()
    eng = engine()
    assert eng.lib.relax_resnet50_set_canvas_ex(eng.h, 65, 67, ANY) == 0
    try:
        assert eng.resnet50_canvas() == (65, 67)
        for Hc, Wc, flags, words in ((63, 67, ANY, "canvas height 63 is not in [64, 1024]"), (65, 1025, ANY, "canvas width 1025 is not in [64, 1024]"),
                                     (0, 64, ANY, "canvas height 0 "), (-65, 64, ANY, "canvas height -65 "), (64, 64, 2, "unknown bits 2"),
                                     (65, 67, 0, "canvas height 65 is not a multiple of 32 in [64, 1024]")):
            assert eng.lib.relax_resnet50_set_canvas_ex(eng.h, Hc, Wc, flags) != 0
            msg = eng.lib.relax_last_error(eng.h).decode()
            assert words in msg and f"(canvas {Hc} x {Wc})" in msg, msg
            assert eng.resnet50_canvas() == (65, 67)
        # the geometry entry: refused, and the outputs untouched
        taps = (np.zeros(30, np.int32) - 77)
        arena = np.zeros(1, np.int64) - 77
        import ctypes as C
        assert eng.lib.relax_resnet50_canvas_geometry_ex(63, 64, ANY, taps.ctypes.data_as(C.POINTER(C.c_int)), arena.ctypes.data_as(C.POINTER(C.c_int64))) != 0
        assert (taps == -77).all() and arena[0] == -77 and "canvas height 63 is not in [64, 1024] (canvas 63 x 64)" in eng.lib.relax_last_error(None).decode()
    finally:
        assert eng.lib.relax_resnet50_set_canvas(eng.h, 224, 224) == 0
    eng.lib.relax_resnet50_set_canvas_ex(eng.h, 65, 67, ANY)
    eng.load_resnet50(rn50_weights())          # a load puts the default canvas and the default rule back
    assert eng.resnet50_canvas() == (224, 224)
    with pytest.raises(ValueError, match=r"fragments must be \[N,224,224,3\]"):
        eng.resnet50_features(torch.zeros((1, 65, 67, 3), dtype=torch.uint8).cuda())


def test_the_default_canvas_and_rule_are_back_after_every_any_size_method():
    rn50_weights()
    eng = engine()
    x = torch.from_numpy(_images(1, 70, 100)).cuda()
    eng.resnet50_features_canvas(x, any_size=True)
    assert eng.resnet50_canvas() == (224, 224)
    with pytest.raises(IndexError):
        eng.resnet50_features_canvas(x, taps=[99], any_size=True)
    assert eng.resnet50_canvas() == (224, 224)
    eng.resnet50_clip_features_canvas(torch.cat([x, x]), 1, any_size=True)
    assert eng.resnet50_canvas() == (224, 224)
    with pytest.raises(ValueError, match=r"canvas width 1030 is not in \[64, 1024\] \(canvas 64 x 1030\)"):
        eng.resnet50_features_canvas(torch.zeros((1, 64, 1030, 3), dtype=torch.uint8).cuda(), any_size=True)
    assert eng.resnet50_canvas() == (224, 224)
    # the keyword does not stick: the next call without it is refused with today's words
    with pytest.raises(ValueError, match=r"canvas width 100 is not a multiple of 32 in \[64, 1024\] \(canvas 64 x 100\)"):
        eng.resnet50_features_canvas(torch.zeros((1, 64, 100, 3), dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="canvas height 70 is not a multiple of 32"):
        eng.resnet50_clip_features_canvas(torch.cat([x, x]), 1)
    assert eng.resnet50_canvas() == (224, 224)


def test_clip_vectors_do_not_notice_an_any_size_call(each_precision):
    from tests.gpu_common import vit_weights
    rn50_weights()
    vit_weights("vit_base")
    eng = engine()
    clips = [torch.from_numpy(synth.synthetic_clip(2, 240, 320, clip_id=11)).cuda()]
    before = eng.clip_vectors(clips)
    eng.resnet50_features_canvas(torch.from_numpy(_images(1, 65, 67)).cuda(), any_size=True)
    after = eng.clip_vectors(clips)
    assert torch.equal(before, after)


# ---- the methods on top ------------------------------------------------------------------------------------------------------------------
def test_fragment_resnet_vectors_on_the_patch_8_canvas_232(each_precision):
    from tests.gpu_common import vit_weights
    rn50_weights()
    vit_weights("vit_base")
    eng = engine()
    clip = torch.from_numpy(np.stack([np.stack(synth.synthetic_pair(240, 320, 40 + i)) for i in range(2)])).cuda()     # [2,2,240,320,3]
    rows = eng.fragment_resnet_vectors(clip, patch_size=8, target_size=232, any_size=True)
    assert tuple(rows.shape) == (2, 13120 + 2051) and rows.dtype == torch.float32
    fr = eng.fragment_pairs(clip, top_n=None, patch_size=8, target_size=232)
    ls, pool = eng.resnet50_clip_features_canvas(torch.cat([fr["ori_frag"], fr["diff_frag"]], dim=0), 2, any_size=True)
    assert torch.equal(rows, torch.cat([ls, pool], dim=1))
    ref_ls = resnet50_ref.layer_stack_features(resnet50_ref.to_torch_state_dict(rn50_weights()), fr["ori_frag"].cpu().numpy())
    assert_close(rows[:, :13120], ref_ls, "232 fragment layer stack")
    both = eng.fragment_canvas_vectors(clip, 232, patch_size=8, any_size=True)
    assert torch.equal(both[:, :13120 + 2051], rows) and both.shape[1] == 13120 + 2051 + 6 * eng.vit_dim
    with pytest.raises(ValueError, match="canvas height 232 is not a multiple of 32"):      # without the keyword: as before
        eng.fragment_resnet_vectors(clip, patch_size=8, target_size=232)
    assert eng.resnet50_canvas() == (224, 224)


def test_whole_frame_methods_at_270x480(each_precision):
    from PIL import Image
    from tests.gpu_common import vit_weights
    rn50_weights()
    vit_weights("vit_base")
    eng = engine()
    frames = np.stack([synth.synthetic_pair(360, 640, 70 + i)[0] for i in range(2)])
    dev = torch.from_numpy(frames).cuda()
    got = eng.whole_frame_resnet_canvas(dev, (270, 480), any_size=True)
    host = np.stack([np.asarray(Image.fromarray(f).resize((480, 270), Image.BILINEAR)) for f in frames])
    want = eng.resnet50_features_canvas(torch.from_numpy(host).cuda(), any_size=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="canvas height 270 "):
        eng.whole_frame_resnet_canvas(dev, (270, 480))
    both = eng.whole_frame_canvas_vectors(dev, (270, 480))
    _, pooled = eng.whole_frame_vit_canvas(dev, (270, 480))
    assert tuple(both.shape) == (2, 13120 + 2051 + 3 * eng.vit_dim)
    assert torch.equal(both, torch.cat([got[0], got[1], pooled], dim=1))
    # a frame at its own size: no resize, both backbones on the frame's bytes
    own = eng.whole_frame_canvas_vectors(dev[:1, :270, :480].contiguous(), (270, 480))
    ls, pool = eng.resnet50_features_canvas(dev[:1, :270, :480].contiguous(), any_size=True)
    assert torch.equal(own[:, :13120 + 2051], torch.cat([ls, pool], dim=1))
    assert eng.resnet50_canvas() == (224, 224)


# ---- stream ------------------------------------------------------------------------------------------------------------------------------
def test_an_any_size_call_stays_on_a_held_side_stream(each_precision):
    """One call at 65 x 67 on a non-blocking side stream that is held: the bits of the default stream's call, and the call returns while the
    stream is still blocked (the helper of tests/test_gpu_stream_contract.py)."""
    def make(seed):
        return {"images": torch.from_numpy(_images(3, 65, 67, seed=20 + seed)).cuda()}

    def call(eng, t):
        ls, pool, taps = eng.resnet50_features_canvas(t["images"], taps=(0, 7, 14), any_size=True)
        return ls, pool, taps[0], taps[7], taps[14]

    case = sc.Case("enqueue", make, call, precisions=sc.PRECISIONS, needs=("rn50",))
    rep = run_held(case, f"resnet50_features_canvas any-size 65x67 {each_precision}")
    assert not rep.mismatch, f"outputs {rep.mismatch} on the held side stream differ from the default stream's"
    assert rep.still_held, "the call returned only after its stream's hold had run out: it waited"
