"""The pooling of the fragment-free drivers (relax_vqa_amd.main_residual / main_layer: process_video_feature) on recorded
activations against tests/golden/whole_residual.npz - what the reference's own two functions return for the same arrays
(tools/make_whole_residual_golden.py) -, their widths, their refusals and their reference-shaped signatures.  No GPU."""
import inspect
import os

import numpy as np
import pytest

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import main_layer, main_residual

NETWORKS = ["resnet50", "vgg16", "vit"]
DIM = 192


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "whole_residual.npz"))


def test_fixture_holds_only_the_documented_arrays(golden):
    assert sorted(golden.files) == sorted(f"{p}_{n}" for p in ("act", "residual", "layer") for n in NETWORKS)
    assert golden["act_resnet50"].shape == (2, 2048, 1, 1) and golden["act_vgg16"].shape == (2, 4096)
    assert golden["act_vit"].shape == (2, 196, DIM)


@pytest.mark.parametrize("network", NETWORKS)
def test_pooling_equals_the_reference_to_the_last_bit(golden, network):
    acts = list(golden[f"act_{network}"])
    for module, tag in ((main_residual, "residual"), (main_layer, "layer")):
        got = module.process_video_feature(acts, network)
        want = golden[f"{tag}_{network}"]
        assert got.dtype == want.dtype and got.shape == want.shape, f"{tag} {network}"
        assert np.array_equal(got, want), f"{tag} {network}: differs from the reference's pooling"


def test_widths(golden):
    rows = {n: main_residual.process_video_feature(list(golden[f"act_{n}"]), n) for n in NETWORKS}
    assert [rows[n].shape for n in NETWORKS] == [(2, 2051), (2, 4099), (2, 3 * DIM)]
    rows = {n: main_layer.process_video_feature(list(golden[f"act_{n}"]), n) for n in NETWORKS}
    assert [rows[n].shape for n in NETWORKS] == [(2, 2048), (2, 4096), (2, 3 * DIM)]
    # whole residual = whole frame | mean, max, std for the CNNs; the same row for the ViT
    for n in ("resnet50", "vgg16"):
        a = np.squeeze(golden[f"act_{n}"])
        got = main_residual.process_video_feature(list(golden[f"act_{n}"]), n)
        assert np.array_equal(got[:, :-3], a) and np.array_equal(got[:, -3], a.mean(axis=1)) and np.array_equal(got[:, -2], a.max(axis=1))


def test_a_pooled_vector_carried_by_the_activation_is_used():
    class Act(np.ndarray):
        pooled = None
    a = np.zeros((2048, 1, 1), dtype=np.float32).view(Act)
    a.pooled = np.arange(2051, dtype=np.float32)
    assert np.array_equal(main_residual.process_video_feature([a], "resnet50")[0], a.pooled)
    t = np.zeros((196, DIM), dtype=np.float32).view(Act)
    t.pooled = np.arange(3 * DIM, dtype=np.float32)
    assert np.array_equal(main_residual.process_video_feature([t], "vit")[0], t.pooled)
    assert np.array_equal(main_layer.process_video_feature([t], "vit")[0], t.pooled)


def test_unknown_names_raise_before_anything_runs():
    img = np.zeros((32, 48, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        main_residual.process_pair(img, img, "resnet50", "residual")
    with pytest.raises(ValueError):
        main_residual.process_pair(img, img, "resnet50", "frame_diff", "layer_stack")
    with pytest.raises(ValueError):
        main_residual.get_deep_feature("resnet50", "v", img, "original", "avgpool")
    with pytest.raises(ValueError):
        main_layer.get_deep_feature("vgg16", "v", img, "original", "fc1")
    with pytest.raises(NotImplementedError):
        main_layer.get_deep_feature("alexnet", "v", img, "original", "pool")
    with pytest.raises(NotImplementedError):        # a 'last_layer' map is not pooled (the reference's result is ragged)
        main_residual.process_video_feature([np.zeros((2048, 7, 7), dtype=np.float32)], "resnet50")


def test_reference_names_and_arity():
    def params(f):
        return list(inspect.signature(f).parameters)
    for m in (main_residual, main_layer):
        assert params(m.get_deep_feature) == ["network_name", "video_name", "image_path", "qp", "layer_name"]
        assert params(m.process_video_feature) == ["video_feature", "network_name"]
    assert params(main_residual.flow_to_rgb) == ["flow"]
    assert params(main_residual.process_pair) == ["img_original", "img_next", "network_name", "residual_name", "layer_name"]
    assert inspect.signature(main_residual.process_pair).parameters["layer_name"].default == "pool"
