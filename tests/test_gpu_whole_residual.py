"""The fragment-free ablation rows on the GPU (engine.whole_residual_features / whole_residual_vectors / whole_frame_pool_features and
the drivers main_residual / main_layer): the whole residual image of a pair, resized and pooled.

The engine rows are bit-equal to the backbones called on the host-made, Pillow-resized residual images with the same batch (same input
bytes, same launches); one oracle anchor per backbone holds them to the suite's standing tolerance under every arithmetic."""
import numpy as np
import pytest
import torch
from PIL import Image

import relax_vqa_amd  # noqa: F401
from oracle import fragment_ref, resnet50_ref, vit_ref
from relax_vqa_amd import main_layer, main_residual, runtime, synth
from relax_vqa_amd.engine import RN50_POOL_DIM, VGG16_POOL_DIM
from tests import vgg16_restated as vr
from tests.gpu_common import assert_close, engine, rn50_weights, vit_weights

pytestmark = pytest.mark.gpu

VIT, DIM, HEADS = "vit_tiny", 192, 3
_cache = {}


def _clip():
    """T = 2 pairs at 270 x 480 with their host-made difference images and Pillow resizes (made once, never written to)."""
    if "clip" not in _cache:
        g = np.random.default_rng(11)
        frames = g.integers(0, 256, (2, 2, 270, 480, 3), dtype=np.uint8)
        frames[:, 1, 40:200, 100:300] = frames[:, 0, 36:196, 90:290]        # a moved block: a residual with structure, and a flow
        d = fragment_ref.absdiff(frames[:, 1], frames[:, 0])
        _cache["clip"] = (frames, *_pil(d))
    return _cache["clip"]


def _pil(images):
    return (np.stack([np.asarray(Image.fromarray(im).resize((224, 224), Image.BILINEAR)) for im in images]),
            np.stack([np.asarray(Image.fromarray(im).resize((224, 224), Image.LANCZOS)) for im in images]))


def _vgg_weights():
    if "vgg" not in _cache:
        _cache["vgg"] = synth.vgg16_state_dict()
        engine().load_vgg16(_cache["vgg"])
    return _cache["vgg"]


def _eng():
    rn50_weights()
    vit_weights(VIT)
    _vgg_weights()
    return engine()


def _backbones(eng, bil, lan):
    """The three pool outputs on given input bytes (host arrays or device tensors)."""
    return {"resnet": eng.resnet50_features(torch.as_tensor(bil).cuda(), layer_stack=False, pool=True)[1],
            "vit": eng.vit_features(torch.as_tensor(lan).cuda(), tokens=False, pooled=True)[1],
            "vgg16": eng.vgg16_features(torch.as_tensor(bil).cuda(), layer_stack=False, pool=True)[1]}


def _assert_same_rows(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32, k
        assert torch.equal(got[k], want[k]), f"{k}: rows differ from the backbone on the host-made images"


def test_frame_diff_rows_equal_the_backbones_on_host_made_residuals():
    eng = _eng()
    frames, bil, lan = _clip()
    got = eng.whole_residual_features(torch.from_numpy(frames).cuda(), "frame_diff", vgg16=True)
    assert tuple(got["resnet"].shape) == (2, 2051) and tuple(got["vit"].shape) == (2, 3 * DIM) and tuple(got["vgg16"].shape) == (2, 4099)
    _assert_same_rows(got, _backbones(eng, bil, lan))
    only = eng.whole_residual_features(torch.from_numpy(frames).cuda(), resnet=False, vit=True)
    assert list(only) == ["vit"] and torch.equal(only["vit"], got["vit"])


def test_optical_flow_rows_with_and_without_given_flow_images():
    eng = _eng()
    frames = torch.from_numpy(_clip()[0]).cuda()
    flow_img = eng.optical_flow(frames)[1]
    want = _backbones(eng, *eng.resize_frames(flow_img))
    _assert_same_rows(eng.whole_residual_features(frames, "optical_flow", vgg16=True), want)
    _assert_same_rows(eng.whole_residual_features(frames, "optical_flow", vgg16=True, flow_images=flow_img), want)
    # a given flow image is what gets pooled, whatever the frames say
    other = eng.whole_residual_features(torch.zeros_like(frames), "optical_flow", vgg16=True, flow_images=flow_img)
    _assert_same_rows(other, want)


def _oracle_rows():
    """fp32 oracle rows of the first pair's resized residual: oracle/resnet50_ref, oracle/vit_ref, tests/vgg16_restated."""
    if "oracle" not in _cache:
        _, bil, lan = _clip()
        rn = resnet50_ref.pool_features(resnet50_ref.to_torch_state_dict(rn50_weights()), bil[:1])
        vt = vit_ref.pool_features(vit_ref.to_torch_state_dict(vit_weights(VIT)), lan[:1], heads=HEADS)
        m = vr.build(_vgg_weights())
        vg = vr.features(vr.taps(m, vr.preprocess_bgr_u8(bil[:1])))[1].numpy()
        _cache["oracle"] = {"resnet": rn, "vit": vt, "vgg16": vg}
    return _cache["oracle"]


def test_oracle_anchor_per_backbone(each_precision):
    eng = _eng()
    want = _oracle_rows()
    got = eng.whole_residual_features(torch.from_numpy(_clip()[0][:1]).cuda(), "frame_diff", vgg16=True)
    for k in ("resnet", "vit", "vgg16"):
        assert_close(got[k], want[k], f"{each_precision} whole-residual {k}")


def test_whole_frame_pool_rows_are_the_leading_pool_columns():
    eng = _eng()
    whole = torch.from_numpy(np.ascontiguousarray(_clip()[0][:, 0])).cuda()
    got = eng.whole_frame_pool_features(whole, vgg16=True)
    want = _backbones(eng, *eng.resize_frames(whole))
    assert tuple(got["resnet"].shape) == (2, 2048) and tuple(got["vgg16"].shape) == (2, 4096) and tuple(got["vit"].shape) == (2, 3 * DIM)
    assert torch.equal(got["resnet"], want["resnet"][:, :RN50_POOL_DIM - 3])
    assert torch.equal(got["vgg16"], want["vgg16"][:, :VGG16_POOL_DIM - 3])
    assert torch.equal(got["vit"], want["vit"])
    assert list(eng.whole_frame_pool_features(whole, resnet=False, vit=False, vgg16=True)) == ["vgg16"]


@pytest.mark.parametrize("residual_name", ["frame_diff", "optical_flow"])
def test_vectors_of_two_clips_of_different_resolution_and_length(residual_name):
    eng = _eng()
    g = np.random.default_rng(12)
    clips = [torch.from_numpy(_clip()[0]).cuda(), torch.from_numpy(g.integers(0, 256, (3, 2, 100, 130, 3), dtype=np.uint8)).cuda()]
    out, rows = eng.whole_residual_vectors(clips, residual_name, vgg16=True, per_frame=True)
    assert tuple(out.shape) == (2, 2051 + 3 * DIM + 4099) and [tuple(r.shape) for r in rows] == [(2, out.shape[1]), (3, out.shape[1])]
    assert torch.equal(out, eng.whole_residual_vectors(clips, residual_name, vgg16=True))
    for i in range(2):
        assert torch.equal(out[i], eng.rows_mean(rows[i])), f"clip {i}: row is not the mean of its per-frame rows"
    # the per-frame rows are the backbones' rows of the one batch of 5 images, in the column order resnet | vit | vgg16
    if residual_name == "frame_diff":
        ins = [eng.residual_resize(c)[:2] for c in clips]
    else:
        ins = [eng.resize_frames(eng.optical_flow(c)[1]) for c in clips]
    want = _backbones(eng, torch.cat([b for b, _ in ins]), torch.cat([l for _, l in ins]))
    got = torch.cat(rows)
    assert torch.equal(got[:, :2051], want["resnet"])
    assert torch.equal(got[:, 2051:2051 + 3 * DIM], want["vit"])
    assert torch.equal(got[:, 2051 + 3 * DIM:], want["vgg16"])
    # a subset keeps the order of those requested
    sub, sub_rows = eng.whole_residual_vectors(clips, residual_name, resnet=False, vit=True, vgg16=True, per_frame=True)
    assert tuple(sub.shape) == (2, 3 * DIM + 4099)
    assert torch.equal(torch.cat(sub_rows)[:, :3 * DIM], want["vit"]) and torch.equal(torch.cat(sub_rows)[:, 3 * DIM:], want["vgg16"])


def test_unknown_names_and_empty_requests_raise():
    eng = _eng()
    frames = torch.from_numpy(_clip()[0]).cuda()
    with pytest.raises(ValueError):
        eng.whole_residual_features(frames, "residual")
    with pytest.raises(ValueError):
        eng.whole_residual_vectors([frames], "flow")
    with pytest.raises(ValueError):
        eng.whole_residual_features(frames, resnet=False, vit=False)


@pytest.fixture(scope="module")
def driver_engine():
    """The drivers run on the process-wide engine of relax_vqa_amd.runtime with the ViT-B the reference names."""
    eng = runtime.set_weights(resnet50=rn50_weights(), vit=synth.vit_state_dict("vit_base"), vit_name="vit_base", vgg16=_vgg_weights())
    yield eng
    runtime._state["vgg"] = None        # VGG-16 weights stay opt-in for whoever uses the runtime next


@pytest.mark.parametrize("network,key,width", [("resnet50", "resnet", 2051), ("vit", "vit", 2304), ("vgg16", "vgg16", 4099)])
@pytest.mark.parametrize("residual_name", ["frame_diff", "optical_flow"])
def test_main_residual_driver_reproduces_the_engine_rows(driver_engine, network, key, width, residual_name):
    frames = _clip()[0]
    acts = [main_residual.process_pair(frames[t, 0], frames[t, 1], network, residual_name) for t in range(2)]
    rows = main_residual.process_video_feature(acts, network)
    assert rows.shape == (2, width) and rows.dtype == np.float32
    for t in range(2):
        want = driver_engine.whole_residual_features(torch.from_numpy(frames[t:t + 1]).cuda(), residual_name, resnet=key == "resnet",
                                                     vit=key == "vit", vgg16=key == "vgg16")[key]
        assert np.array_equal(rows[t], want[0].cpu().numpy()), f"{network} {residual_name} pair {t}"
    if residual_name == "frame_diff":       # the path-free form of get_deep_feature on the residual image itself
        d = fragment_ref.absdiff(frames[0, 1], frames[0, 0])
        _, _, act = main_residual.get_deep_feature(network, "v", d, "original", "pool")
        assert np.array_equal(main_residual.process_video_feature([act], network)[0], rows[0])


@pytest.mark.parametrize("network,key,width", [("resnet50", "resnet", 2048), ("vit", "vit", 2304), ("vgg16", "vgg16", 4096)])
def test_main_layer_driver_reproduces_the_engine_rows(driver_engine, network, key, width):
    frames = _clip()[0]
    acts = [main_layer.get_deep_feature(network, "v", frames[t, 0], "original", "pool")[2] for t in range(2)]
    rows = main_layer.process_video_feature(acts, network)
    assert rows.shape == (2, width) and rows.dtype == np.float32
    for t in range(2):
        want = driver_engine.whole_frame_pool_features(torch.from_numpy(frames[t:t + 1, 0].copy()).cuda(), resnet=key == "resnet",
                                                       vit=key == "vit", vgg16=key == "vgg16")[key]
        assert np.array_equal(rows[t], want[0].cpu().numpy()), f"{network} frame {t}"


def test_last_layer_is_refused_like_the_fragment_driver(driver_engine):
    frames = _clip()[0]
    act = main_residual.process_pair(frames[0, 0], frames[0, 1], "resnet50", "frame_diff", "last_layer")
    assert act.shape == (2048, 7, 7)
    with pytest.raises(NotImplementedError):
        main_residual.process_video_feature([act], "resnet50")
    with pytest.raises(NotImplementedError):
        main_layer.process_video_feature([act], "resnet50")
