"""VGG-16 backbone, the parts that need no GPU: the restated oracle (shapes, the in-place ReLU quirk), the host logic of the loader
(fc1 column permutation, key and shape refusal) and the synthetic weights' keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import synth
from tests import vgg16_restated as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    return synth.vgg16_state_dict()


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.relax_host_vgg16_check_keys.restype = C.c_int
    return lib


def _small_input(seed=0, n=1):
    g = np.random.default_rng(seed)
    return vr.preprocess_bgr_u8(g.integers(0, 256, (n, 224, 224, 3), dtype=np.uint8))


def test_restated_net_tap_shapes_and_feature_sizes(sd):
    m = vr.build(sd)
    t = vr.taps(m, _small_input())
    assert len(t) == 15
    for (c, s), a in zip(vr.TAP_SHAPES, t[:13]):
        assert tuple(a.shape) == (1, c, s, s)
    assert tuple(t[13].shape) == (1, 4096) and tuple(t[14].shape) == (1, 4096)
    ls, pool = vr.features(t)
    assert ls.shape[1] == 4224 == vr.LAYER_STACK_DIM and pool.shape[1] == 4099 == vr.POOL_DIM


def test_hooked_taps_are_post_relu(sd):
    """torchvision's ReLU(inplace=True) rectifies the hooked conv output before the reference reads it: the tap is relu(conv), and on
    weights with negative pre-activations (the adversarial set's mixed-sign biases) that differs from the raw convolution."""
    sd_adv = synth.vgg16_state_dict(adversarial=True)
    m = vr.build(sd_adv)
    x = _small_input(1)
    t = vr.taps(m, x)
    raw = torch.nn.functional.conv2d(x, m.features[0].weight, m.features[0].bias, padding=1)
    assert (raw < 0).any()
    assert torch.equal(t[0], torch.relu(raw))
    assert not torch.equal(t[0], raw)
    assert (t[13] >= 0).all() and (t[14] >= 0).all()


def test_fc1_column_permutation_fp64(host_lib):
    """classifier.0's weight, permuted from the NCHW flatten (c*49 + y*7 + x) to the NHWC one, times the NHWC flatten of pool5 equals
    torchvision's product on the NCHW flatten (fp64)."""
    g = np.random.default_rng(5)
    rows = 64
    w = g.standard_normal((rows, 512 * 49)).astype(np.float32)
    x = g.standard_normal((512, 7, 7)).astype(np.float32)
    wp = np.full_like(w, np.nan)
    host_lib.relax_host_vgg16_fc1_to_nhwc(w.ctypes.data_as(C.c_void_p), rows, 512, 49, wp.ctypes.data_as(C.c_void_p))
    want = w.astype(np.float64) @ x.reshape(-1).astype(np.float64)
    got = wp.astype(np.float64) @ x.transpose(1, 2, 0).reshape(-1).astype(np.float64)
    assert np.isfinite(wp).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9)
    assert not np.allclose(w.astype(np.float64) @ x.transpose(1, 2, 0).reshape(-1), want)   # (the order matters)


def _check(lib, sd):
    names = [k.encode() for k in sd]
    arrays = [np.ascontiguousarray(v, dtype=np.float32) for v in sd.values()]
    n = len(names)
    err = C.create_string_buffer(256)
    rc = lib.relax_host_vgg16_check_keys((C.c_void_p * n)(*[a.ctypes.data for a in arrays]), (C.c_char_p * n)(*names),
                                         (C.c_int64 * n)(*[a.size for a in arrays]), n, err, 256)
    return rc, err.value.decode()


def test_loader_refuses_missing_keys_and_wrong_shapes(host_lib, sd):
    assert _check(host_lib, sd) == (0, "")
    extra = dict(sd)
    extra["classifier.6.weight"] = np.zeros((1000, 4096), np.float32)      # ignored, as ResNet's fc.*
    assert _check(host_lib, extra)[0] == 0
    missing = {k: v for k, v in sd.items() if k != "features.17.bias"}
    rc, msg = _check(host_lib, missing)
    assert rc == -1 and "features.17.bias" in msg
    wrong = dict(sd)
    wrong["classifier.3.weight"] = sd["classifier.3.weight"][:4095]
    rc, msg = _check(host_lib, wrong)
    assert rc == -1 and "classifier.3.weight" in msg
    bad_conv = dict(sd)
    bad_conv["features.5.weight"] = np.zeros((128, 32, 3, 3), np.float32)
    rc, msg = _check(host_lib, bad_conv)
    assert rc == -1 and "features.5.weight" in msg


@pytest.mark.parametrize("adversarial", [False, True])
def test_synthetic_state_dict_matches_torchvision_keys(adversarial):
    sd = synth.vgg16_state_dict(adversarial=adversarial)
    want = {k: tuple(v.shape) for k, v in vr.VGG16().state_dict().items() if not k.startswith("classifier.6.")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(v.dtype == np.float32 for v in sd.values())
