"""The host half of the any-size resize (include/relax_hip.h: relax_resize_table, relax_resize_output_size; csrc/host_logic.cpp) and its
yardstick: the tables against oracle/resize_ref.precompute_coeffs, the tables the 224 entries read inside the 24 bits the kernels multiply
in, the output size against the rule transforms.Resize(int) applies to a PIL image, and oracle/resize_ref.resize against PIL.Image.resize
at every case the GPU tests use."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import relax_vqa_amd  # noqa: F401
from oracle import resize_ref
from relax_vqa_amd import _lib
from tests import resize_any_cases as cases

MAX_OUT, MAX_IN = 2048, 16384


def _table(lib, in_size, out_size, filt):
    ksize = C.c_int(0)
    assert lib.relax_resize_table(in_size, out_size, filt, None, None, C.byref(ksize)) == 0, lib.relax_last_error(None)
    bounds = np.full((out_size, 2), -7, np.int32)
    coeffs = np.full((out_size, ksize.value), -7, np.int32)
    k2 = C.c_int(0)
    assert lib.relax_resize_table(in_size, out_size, filt, bounds.ctypes.data, coeffs.ctypes.data, C.byref(k2)) == 0
    assert k2.value == ksize.value
    return bounds, coeffs


@pytest.mark.parametrize("filt", [resize_ref.BILINEAR, resize_ref.LANCZOS], ids=["bilinear", "lanczos"])
@pytest.mark.parametrize("in_size,out_size", cases.TABLE_PAIRS)
def test_table_equals_the_oracle(in_size, out_size, filt):
    bounds, coeffs = _table(_lib.load(), in_size, out_size, filt)
    want_b, want_c = resize_ref.precompute_coeffs(in_size, out_size, filt)
    assert coeffs.shape == want_c.shape, "ksize"
    assert np.array_equal(bounds, want_b)
    assert np.array_equal(coeffs, want_c)


@pytest.mark.parametrize("filt", [resize_ref.BILINEAR, resize_ref.LANCZOS], ids=["bilinear", "lanczos"])
def test_tables_to_224_stay_inside_24_bits(filt):
    """The kernels multiply on the 24-bit multiplier and the device table refuses a coefficient outside it: for the 224 entries it never
    does.  224 -> 224 is the identity (one 2^22 per sample), which is why a skipped pass and an identity pass give the same bytes."""
    lib = _lib.load()
    for in_size in cases.IN_SIZES_224:
        _, coeffs = _table(lib, in_size, 224, filt)
        assert int(np.abs(coeffs.astype(np.int64)).max()) < 1 << 23, in_size
    bounds, coeffs = _table(lib, 224, 224, filt)
    for i in range(224):
        assert bounds[i, 0] <= i < bounds[i, 0] + bounds[i, 1], i      # the 2^22 sits on sample i itself
        row = np.zeros(coeffs.shape[1], np.int32)
        row[i - bounds[i, 0]] = 1 << 22
        assert np.array_equal(coeffs[i], row), i


def test_table_refusals_name_the_value():
    lib = _lib.load()
    k = C.c_int(0)
    for args, name in (((0, 5, 0), "in_size=0"), ((MAX_IN + 1, 5, 0), f"in_size={MAX_IN + 1}"), ((5, 0, 1), "out_size=0"),
                       ((5, MAX_OUT + 1, 1), f"out_size={MAX_OUT + 1}"), ((5, 5, 2), "filt=2")):
        assert lib.relax_resize_table(*args, None, None, C.byref(k)) != 0
        assert name in lib.relax_last_error(None).decode()
    assert lib.relax_resize_table(5, 5, 0, None, None, None) != 0


def _python_rule(h, w, size):
    """torchvision's _compute_resized_output_size for an int size, restated"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def _output_size(lib, h, w, size):
    oh, ow = C.c_int(-1), C.c_int(-1)
    rc = lib.relax_resize_output_size(h, w, size, C.byref(oh), C.byref(ow))
    return rc, oh.value, ow.value


def test_output_size_equals_the_python_rule():
    lib = _lib.load()
    dims = [1, 2, 3, 7, 37, 53, 224, 240, 270, 333, 480, 540, 720, 1080, 1920, 2160, 3840, 4097, MAX_IN]
    n = 0
    for h in dims:
        for w in dims:
            for size in (1, 2, 7, 64, 224, 270, 448, 1000, MAX_OUT):   # squares, W < H, W > H, size above the shorter side
                want = _python_rule(h, w, size)
                rc, oh, ow = _output_size(lib, h, w, size)
                if max(want) > MAX_OUT:
                    assert rc != 0 and f"size={size}" in lib.relax_last_error(None).decode(), (h, w, size)
                else:
                    assert (rc, oh, ow) == (0,) + want, (h, w, size)
                    n += 1
    assert n > 1000
    assert _output_size(lib, 1080, 1920, 270) == (0, 270, 480)
    assert _output_size(lib, 1920, 1080, 270) == (0, 480, 270)
    assert _output_size(lib, 500, 500, 224) == (0, 224, 224)
    assert _output_size(lib, 100, 333, 224) == (0, 224, 745)


def test_output_size_refusals_name_the_value():
    lib = _lib.load()
    for (h, w, size), name in (((0, 5, 5), "H=0"), ((5, -1, 5), "W=-1"), ((5, 5, 0), "size=0"), ((5, 5, MAX_OUT + 1), f"size={MAX_OUT + 1}"),
                               ((MAX_IN + 1, 5, 5), f"H={MAX_IN + 1}"), ((10, 100, 1000), "size=1000")):
        assert _output_size(lib, h, w, size)[0] != 0
        assert name in lib.relax_last_error(None).decode(), (h, w, size)
    assert lib.relax_resize_output_size(5, 5, 5, None, None) != 0


@pytest.mark.parametrize("hw,out,n", cases.CASES + [((20, 16), (224, 224), 1), ((270, 480), (224, 224), 1)]
                         + [((5, w), (224, 224), 2) for w in cases.WIDEST_224],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_oracle_is_pillow_at_the_gpu_cases(hw, out, n):
    f = cases.frames(hw, n)[0]
    for filt, pil in ((resize_ref.BILINEAR, Image.BILINEAR), (resize_ref.LANCZOS, Image.LANCZOS)):
        want = np.asarray(Image.fromarray(f).resize((out[1], out[0]), pil))
        assert np.array_equal(resize_ref.resize(f, out[0], out[1], filt), want), (hw, out, filt)
