"""VGG-16 backbone on the GPU against the restated torchvision network (tests/vgg16_restated.py): every tap, both feature vectors,
each arithmetic, batch invariance, the layer selectors, the four drivers' vgg16 branches and the weights policy."""
import numpy as np
import pytest
import torch
from PIL import Image

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import runtime, synth
from tests import vgg16_restated as vr
from tests.gpu_common import assert_close, engine

pytestmark = pytest.mark.gpu

PNG = "tests/golden/png_5636101558_3/5636101558_3"
_cache = {}


def _weights(adv):
    key = ("sd", adv)
    if key not in _cache:
        _cache[key] = synth.vgg16_state_dict(adversarial=adv)
    if _cache.get("loaded") != adv:
        engine().load_vgg16(_cache[key])
        _cache["loaded"] = adv
    return _cache[key]


def _frags():
    """A real fragment, a real residual fragment and two random ones of very different brightness (the scales are per image)."""
    ori = runtime.read_image_bgr(PNG + "_ori_frag.png")
    res = runtime.read_image_bgr(PNG + "_residual_imp.png")
    g = np.random.default_rng(9)
    rnd = g.integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    rnd[0] //= 16
    rnd[1] = 255 - rnd[1] // 8
    return np.ascontiguousarray(np.stack([ori, res, rnd[0], rnd[1]]))


def _ref(adv, dtype=torch.float32):
    key = ("ref", adv, dtype)
    if key not in _cache:
        m = vr.build(_weights(adv), dtype)
        t = vr.taps(m, vr.preprocess_bgr_u8(_frags()).to(dtype))
        _cache[key] = (t, *vr.features(t))
    return _cache[key]


def _close_to_fp64(got, r32, r64, what, channel_axis=None):
    """Element-wise against the fp64 restatement: rtol 1e-3 with the suite's floor (1e-4 x the tensor's / the channel's mean
    magnitude), raised to 4 x torch-CPU fp32's own largest error in the channel.  A value that cancels between inputs 50 - 100 x its
    size (the adversarial set) carries that much rounding in ANY fp32 arithmetic; no tolerance is widened beyond it."""
    got = got.detach().cpu().numpy().astype(np.float64)
    r64 = r64.numpy()
    noise = np.abs(r32.numpy().astype(np.float64) - r64)
    floor = 1e-4 * np.abs(r64).mean()
    if channel_axis is not None:
        axes = tuple(a for a in range(r64.ndim) if a != channel_axis)
        floor = np.maximum(floor, np.maximum(1e-4 * np.abs(r64).mean(axis=axes, keepdims=True), 4 * noise.max(axis=axes, keepdims=True)))
    else:
        floor = np.maximum(floor, 4 * noise.max())
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    worst = float((np.abs(got - r64) / (1e-3 * np.abs(r64) + floor)).max())
    assert worst <= 1.0, f"{what}: max err/bound {worst:.3g}, norm-rel {np.linalg.norm(got - r64) / np.linalg.norm(r64):.3e}"


@pytest.mark.parametrize("adv", [False, True], ids=["regular", "adversarial"])
def test_vgg16_every_tap_and_both_vectors(adv, each_precision, each_split_k):
    _weights(adv)
    eng = engine()
    ls, pool, taps = eng.vgg16_features(torch.from_numpy(_frags()).cuda(), taps=range(15))
    rt, rls, rpool = _ref(adv)
    rt64, rls64, rpool64 = _ref(adv, torch.float64)
    for i in range(15):
        if not adv:
            assert_close(taps[i], rt[i].numpy(), f"{each_precision} tap {i}", channel_axis=1)
        _close_to_fp64(taps[i], rt[i], rt64[i], f"{each_precision} tap {i}", channel_axis=1)
    if not adv:
        assert_close(ls, rls.numpy(), f"{each_precision} layer stack", channel_axis=1)
        assert_close(pool, rpool.numpy(), f"{each_precision} pool")
    _close_to_fp64(ls, rls, rls64, f"{each_precision} layer stack", channel_axis=1)
    _close_to_fp64(pool, rpool, rpool64, f"{each_precision} pool")
    ls2, pool2 = eng.vgg16_features(torch.from_numpy(_frags()).cuda())          # outputs do not depend on what else is asked for
    assert torch.equal(ls, ls2) and torch.equal(pool, pool2)


@pytest.mark.parametrize("adv", [False, True], ids=["regular", "adversarial"])
def test_vgg16_error_against_fp64_no_larger_than_torch_fp32(adv):
    """Every tap's norm-relative error against an fp64 run of the restatement stays within the 1e-3 bar, and within 2.5 x that of
    torch-CPU fp32 (the reference's own arithmetic).  The convolution taps stay within 1.5 x; fc1's 25088-long sums accumulate in
    another order than torch's blocked ones (1.6 x under f16x2, 1.9 x under bf16x6 measured there, at 3 - 4e-6)."""
    _weights(adv)
    eng = engine()
    t32, _, _ = _ref(adv)
    t64, _, _ = _ref(adv, torch.float64)
    f = torch.from_numpy(_frags()).cuda()
    for mode in ("f16x2", "bf16x6"):
        eng.set_precision(mode)
        _, _, taps = eng.vgg16_features(f, layer_stack=False, pool=False, taps=range(15))
        for i in range(15):
            r = t64[i].numpy()
            e_gpu = np.linalg.norm(taps[i].cpu().numpy().astype(np.float64) - r) / np.linalg.norm(r)
            e_cpu = np.linalg.norm(t32[i].numpy().astype(np.float64) - r) / np.linalg.norm(r)
            assert e_gpu <= 1e-3, f"{mode} tap {i}: {e_gpu:.3e}"
            assert e_gpu <= (1.5 if i < 13 else 2.5) * e_cpu + 1e-7, f"{mode} tap {i}: {e_gpu:.3e} against torch fp32 {e_cpu:.3e}"


@pytest.mark.parametrize("mode", ["f16x2", "bf16x6", "fp32"])
def test_vgg16_rows_are_batch_invariant(mode):
    """With the tail split off, an image's rows are the same bits alone and inside a batch of 37 (two chunks of images, N not a
    multiple of any tile)."""
    _weights(False)
    eng = engine()
    eng.set_precision(mode)
    eng.set_option("gemm_split_k", 0)
    try:
        g = np.random.default_rng(21)
        batch = g.integers(0, 256, (37, 224, 224, 3), dtype=np.uint8)
        ls, pool = eng.vgg16_features(torch.from_numpy(batch).cuda())
        for j in (0, 33):
            ls1, pool1 = eng.vgg16_features(torch.from_numpy(batch[j:j + 1]).cuda())
            assert torch.equal(ls1[0], ls[j]) and torch.equal(pool1[0], pool[j]), f"{mode}: image {j}"
    finally:
        eng.set_option("gemm_split_k", 1)


@pytest.fixture
def registered():
    """VGG-16 weights registered with the runtime for one test, unregistered again afterwards (the suite runs in one session)."""
    sd = _weights(False)
    runtime.set_weights(vgg16=sd)
    _cache["loaded"] = False
    yield sd
    runtime._state["vgg"] = None


def test_vgg16_layer_selectors(registered):
    from relax_vqa_amd.extractor import visualise_vgg, visualise_vgg_layer
    rt, rls, rpool = _ref(False)
    frag = _frags()[0]
    fc1 = visualise_vgg_layer.process_fragment_array(frag, "fc1")
    assert_close(fc1, rt[13][0].numpy(), "fc1 selector")
    fc2 = visualise_vgg_layer.process_fragment_array(frag, "fc2")
    assert fc2.shape == (4096,)
    assert_close(np.asarray(fc2), rt[14][0].numpy(), "fc2 selector")
    assert_close(fc2.pooled, rpool[0].numpy(), "fc2 pooled")
    c = visualise_vgg_layer.process_fragment_array(frag, 21)
    assert_close(c, rt[9][0].numpy(), "features[21] selector", channel_axis=0)
    acts = visualise_vgg.process_fragment_array(frag, [0, 28])
    assert list(acts) == [0, 28]
    assert_close(acts[28], rt[12][0].numpy(), "features[28] in a stack", channel_axis=0)
    with pytest.raises(ValueError):
        visualise_vgg_layer.process_fragment_array(frag, 3)      # a ReLU, not a convolution


def test_vgg16_driver_branches(registered):
    from relax_vqa_amd import main_fragment_layerstack as mls
    from relax_vqa_amd import main_fragment_pool as mfp
    from relax_vqa_amd import main_layer_stack as ml
    from relax_vqa_amd import main_residual_fragment as mrf
    _, rls, rpool = _ref(False)
    ori, res = _frags()[0], _frags()[1]
    _, _, a = mls.get_deep_feature("vgg16", "v", ori, "original", "layer_stack")
    assert_close(mls.process_video_feature([a], "vgg16", "layer_stack"), rls[:1].numpy(), "main_fragment_layerstack layer stack",
                 channel_axis=1)
    _, _, p = mls.get_deep_feature("vgg16", "v", res, "original", "pool")
    assert_close(mls.process_video_feature([p], "vgg16", "pool"), rpool[1:2].numpy(), "main_fragment_layerstack pool")
    _, _, p = mfp.get_deep_feature("vgg16", "v", res, "original", "pool")
    assert_close(mfp.process_video_feature([p], "vgg16"), rpool[1:2].numpy(), "main_fragment_pool pool")
    _, _, p = mrf.get_deep_feature("vgg16", "v", res, "original", "pool")
    assert_close(mrf.process_video_feature([p], "vgg16"), rpool[1:2].numpy(), "main_residual_fragment pool")
    # whole frame: PIL-exact bilinear resize to 224^2 on the GPU, then the layer stack
    frame = runtime.read_image_bgr(PNG + ".png")
    rn_in = np.ascontiguousarray(np.asarray(Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).resize((224, 224), Image.BILINEAR))[..., ::-1])
    m = vr.build(_weights(False))
    want_ls, _ = vr.features(vr.taps(m, vr.preprocess_bgr_u8(rn_in[None])))
    _, _, w = ml.get_deep_feature("vgg16", "v", frame, "original")
    assert_close(ml.process_video_feature([w], "vgg16"), want_ls.numpy(), "main_layer_stack whole frame", channel_axis=1)


def test_vgg16_not_implemented_after_reset(registered):
    from relax_vqa_amd import main_fragment_layerstack as mls
    saved = dict(runtime._state)
    try:
        runtime.reset_weights()
        with pytest.raises(NotImplementedError, match="RELAX_VGG16_WEIGHTS"):
            mls.get_deep_feature("vgg16", "v", np.zeros((224, 224, 3), np.uint8), "original", "pool")
    finally:
        runtime._state.update(saved)


def test_vgg16_load_errors_are_runtime_errors():
    eng = engine()
    sd = dict(_weights(False))
    _cache["loaded"] = None
    missing = {k: v for k, v in sd.items() if k != "features.26.weight"}
    with pytest.raises(RuntimeError, match="features.26.weight"):
        eng.load_vgg16(missing)
    wrong = dict(sd)
    wrong["classifier.0.bias"] = sd["classifier.0.bias"][:100]
    with pytest.raises(RuntimeError, match="classifier.0.bias"):
        eng.load_vgg16(wrong)
    with pytest.raises(RuntimeError, match="relax_load_vgg16 first"):
        eng.vgg16_features(torch.from_numpy(_frags()[:1]).cuda())
