"""Two pieces of the model loaders that are host logic (csrc/host_logic.cpp), checked without a GPU:
conv_hoelder - l1max / bmax of a folded convolution, the constants every per-image fp16 scale of the f16x2 ResNet-50 and VGG-16 rests on -
bit for bit against its definition, and read_bn - the four BatchNorm keys of a state dict folded into scale / shift, or a message naming
the key.  Then the same calls from a stand-alone program under AddressSanitizer + UBSan (tests/host_logic_san_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relax-vqa_amd", "csrc")
SHAPES = [(1, 32), (3, 64), (64, 224), (5, 4608)]   # (cout, k); 224: the stem's padded K
BN_KEYS = ("weight", "bias", "running_mean", "running_var")
f32p = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", os.path.join(CSRC, "host_logic.cpp"), "-o", str(out)],
                   check=True)
    return C.CDLL(str(out))


def _p(a):
    return a.ctypes.data_as(f32p) if a is not None else None


def hoelder(lib, rows, bias):
    l1, bm = C.c_float(-1.0), C.c_float(-1.0)
    lib.relax_host_conv_hoelder(_p(rows), _p(bias), rows.shape[0], rows.shape[1], C.byref(l1), C.byref(bm))
    return np.float32(l1.value), np.float32(bm.value)


def want_l1max(rows):
    return max(np.float32(np.cumsum(np.abs(row.astype(np.float64)))[-1] * (1 + 1e-6)) for row in rows)


@pytest.mark.parametrize("cout,k", SHAPES)
def test_conv_hoelder_is_its_definition_bit_for_bit(host_lib, cout, k):
    rng = np.random.default_rng(1000 * cout + k)
    # magnitudes over several binades, so the double sum's rounding to float is not trivially exact
    rows = (rng.standard_normal((cout, k)) * np.exp2(rng.integers(-12, 4, (cout, k)))).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    want = want_l1max(rows)
    l1, bm = hoelder(host_lib, rows, bias)
    assert l1.tobytes() == want.tobytes(), (l1, want)
    assert bm.tobytes() == np.abs(bias).max().tobytes()
    l1, bm = hoelder(host_lib, rows, None)             # the raw stem: no bias
    assert l1.tobytes() == want.tobytes() and bm.tobytes() == np.float32(0).tobytes()
    l1, bm = hoelder(host_lib, np.zeros((cout, k), np.float32), bias)
    assert l1.tobytes() == np.float32(0).tobytes() and bm.tobytes() == np.abs(bias).max().tobytes()


def bn_dict(rng, channels=3, prefix="layer1.0.bn2"):
    sd = {f"{prefix}.{k}": rng.standard_normal(channels).astype(np.float32) for k in BN_KEYS}
    sd[f"{prefix}.running_var"] = np.abs(sd[f"{prefix}.running_var"]) + np.float32(0.1)
    return sd


def read_bn(lib, sd, prefix, channels, eps=1e-5):
    names = [k.encode() for k in sd]
    arrays = [np.ascontiguousarray(v, np.float32) for v in sd.values()]
    n = len(names)
    ptrs = (f32p * n)(*[_p(a) for a in arrays])
    cnames = (C.c_char_p * n)(*names)
    numels = (C.c_int64 * n)(*[a.size for a in arrays])
    scale, shift = np.full(channels, np.nan, np.float32), np.full(channels, np.nan, np.float32)
    err = C.create_string_buffer(512)
    rc = lib.relax_host_read_bn(ptrs, cnames, numels, n, prefix.encode(), channels, C.c_float(eps), _p(scale), _p(shift), err, 512)
    return rc, scale, shift, err.value.decode()


def test_read_bn_equals_fold_bn_of_the_same_arrays(host_lib):
    prefix = "layer1.0.bn2"
    sd = bn_dict(np.random.default_rng(3), prefix=prefix)
    rc, scale, shift, err = read_bn(host_lib, sd, prefix, 3)
    assert rc == 0 and err == ""
    g, b, mu, var = (sd[f"{prefix}.{k}"] for k in BN_KEYS)
    want_scale, want_shift = np.empty(3, np.float32), np.empty(3, np.float32)
    host_lib.relax_host_fold_bn(_p(g), _p(b), _p(mu), _p(var), C.c_float(1e-5), 3, _p(want_scale), _p(want_shift))
    assert scale.tobytes() == want_scale.tobytes() and shift.tobytes() == want_shift.tobytes()
    s64 = g.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)    # fold_bn itself: eval-mode BatchNorm, to fp32 rounding
    np.testing.assert_allclose(scale, s64, rtol=1e-6)
    np.testing.assert_allclose(shift, b - mu * s64, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("key", BN_KEYS)
def test_read_bn_names_a_missing_key(host_lib, key):
    prefix = "layer1.0.bn2"
    sd = bn_dict(np.random.default_rng(4), prefix=prefix)
    del sd[f"{prefix}.{key}"]
    rc, _, _, err = read_bn(host_lib, sd, prefix, 3)
    assert rc == -1 and err == f"state dict: missing key '{prefix}.{key}'"


def test_read_bn_names_a_mis_sized_key(host_lib):
    prefix = "layer1.0.bn2"
    sd = bn_dict(np.random.default_rng(5), prefix=prefix)
    sd[f"{prefix}.running_mean"] = np.zeros(4, np.float32)
    rc, _, _, err = read_bn(host_lib, sd, prefix, 3)
    assert rc == -1 and err == f"state dict: key '{prefix}.running_mean' has 4 elements, expected 3"


def test_sanitizer_program_runs_clean(tmp_path):
    """tests/host_logic_san_main.cpp + csrc/host_logic.cpp under AddressSanitizer + UBSan: a plain child process, nothing preloaded."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    san = ["-fsanitize=address,undefined"]
    probe = ["-x", "c++", "-", "-o", os.devnull]
    if subprocess.run([cxx, *san, *probe], input="int main(){}", capture_output=True, text=True).returncode != 0:
        pytest.skip(f"{cxx} -fsanitize=address,undefined cannot link on this machine")
    # (the sanitizer runtimes linked statically where the compiler can, as csrc/Makefile's SAN_STATIC does: the program has no dependency on a shared libasan)
    static = ["-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *san, *static, *probe], input="int main(){}", capture_output=True, text=True).returncode == 0:
        san += static
    exe = str(tmp_path / "host_logic_san")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I", CSRC, *san, "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "host_logic_san_main.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_logic_san: OK" in res.stdout
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr
