"""ViT geometry as host logic (csrc/host_logic.cpp: vit_geometry, the arena sizes, the streaming attention kernel's plan), the synthetic
patch-8 weights, the patch-8 oracle against the reference's own VisionTransformer(patch_size=8), and the argument checks of
VitGenerator - all without a GPU."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import relax_vqa_amd  # noqa: F401
from relax_vqa_amd import synth
from oracle import vit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    return C.CDLL(str(out))


def _geometry(lib, patch):
    out, err = (C.c_int * 5)(), C.create_string_buffer(256)
    rc = lib.relax_host_vit_geometry(patch, out, err, 256)
    return list(out) if rc == 0 else err.value.decode()


def _arena(lib, dim, ntok, npatch, patch_k):
    out = (C.c_int64 * 2)()
    lib.relax_host_vit_arena_floats(dim, ntok, npatch, patch_k, out)
    return list(out)


def _plan(lib, n_img, heads, ntok, arith):
    out, err = (C.c_int * 5)(), C.create_string_buffer(256)
    rc = lib.relax_host_att_stream_plan(n_img, heads, ntok, arith, out, err, 256)
    return dict(zip(("qblock", "qblocks", "key_tiles", "lds_bytes", "items"), out)) if rc == 0 else err.value.decode()


def test_vit_geometry(host_lib):
    assert _geometry(host_lib, 16) == [16, 14, 196, 197, 768]
    assert _geometry(host_lib, 8) == [8, 28, 784, 785, 192]
    for p in (7, 12, 32, 0, -8):
        msg = _geometry(host_lib, p)
        assert isinstance(msg, str) and str(p) in msg and "8 or 16" in msg, (p, msg)


def test_patch16_arena_sizes_are_the_constants_they_replace(host_lib):
    """floats per image of the two arena layouts for the three model widths, written out: 196 * 768 patches + 196 dim + 197 dim * (2 + 3 + 4)
    under fp32; 1.5 x the patches, 196 dim, 197 dim * (1 + 1.5 + 3 + 1 + 6) under bf16x6 / f16x2"""
    assert _arena(host_lib, 768, 197, 196, 768) == [1662720, 2267520]
    assert _arena(host_lib, 384, 197, 196, 768) == [906624, 1246656]
    assert _arena(host_lib, 192, 197, 196, 768) == [528576, 736224]
    for dim in (192, 384, 768):
        assert _arena(host_lib, dim, 197, 196, 768) == [196 * 768 + 196 * dim + 197 * dim * 9,
                                                        196 * 768 * 3 // 2 + 196 * dim + 197 * dim * 5 + 197 * dim * 3 // 2 + 197 * dim * 6]
    # ViT-B/8: 33.5 MB per image, 3.7 times ViT-B/16's 9.1 MB
    b8, b16 = max(_arena(host_lib, 768, 785, 784, 192)) * 4, max(_arena(host_lib, 768, 197, 196, 768)) * 4
    assert b8 == 33455616 and b16 == 9070080 and 3.6 < b8 / b16 < 3.8


@pytest.mark.parametrize("arith", [0, 1], ids=["fp32", "bf16x6"])
@pytest.mark.parametrize("ntok", [1, 32, 33, 197, 785])
def test_stream_plan_invariants(host_lib, ntok, arith):
    p = _plan(host_lib, 3, 12, ntok, arith)
    assert p["qblock"] in (64, 128)
    covered = np.zeros(ntok, dtype=np.int64)          # every query belongs to exactly one query block
    for b in range(p["qblocks"]):
        lo, hi = b * p["qblock"], min(ntok, (b + 1) * p["qblock"])
        assert lo < hi, "an empty query block"
        covered[lo:hi] += 1
    assert (covered == 1).all()
    assert p["key_tiles"] == -(-ntok // 32)
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert p["items"] == 3 * 12 * p["qblocks"]


def test_stream_plan_refusals(host_lib):
    for args in ((0, 12, 785, 0), (1, 0, 785, 1), (1, 12, 0, 1), (1, 12, 785, 2)):
        assert isinstance(_plan(host_lib, *args), str), args
    assert "2^31" in _plan(host_lib, 1, 12, 300000, 0)          # one image's qkv rows must stay inside a buffer resource
    assert "work items" in _plan(host_lib, 2 ** 20, 4096, 129, 1)


def _dict_hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def test_synthetic_patch8_weights():
    sd8 = synth.vit_state_dict("vit_tiny", patch=8)
    assert sd8["pos_embed"].shape == (1, 785, 192) and sd8["patch_embed.proj.weight"].shape == (192, 3, 8, 8)
    # the patch-16 draws did not move: the hash of the dict as it was before `patch` reached pos_embed
    sd16 = synth.vit_state_dict("vit_tiny", patch=16)
    assert sd16["pos_embed"].shape == (1, 197, 192)
    assert _dict_hash(sd16) == "49dd7a3909c09f2e2ff0a705d507f47177837e59381cbfab230821cea006e802"
    assert _dict_hash(synth.vit_state_dict("vit_tiny")) == _dict_hash(sd16)


def test_patch8_oracle_matches_the_reference_class(golden_dir):
    """tests/golden/vit_patch8_tiny.npz: the reference's VisionTransformer(patch_size=8) on the same weights and fragments
    (tools/make_vit_patch8_golden.py)"""
    z = np.load(os.path.join(golden_dir, "vit_patch8_tiny.npz"))
    frags = np.random.default_rng(int(z["seed"])).integers(0, 256, (int(z["n_img"]), 224, 224, 3), dtype=np.uint8)
    tsd = vit_ref.to_torch_state_dict(synth.vit_state_dict("vit_tiny", patch=8))
    tok = vit_ref.forward_tokens(tsd, vit_ref.preprocess_bgr_u8(frags), 3, patch=8).numpy()
    assert tok.shape == (2, 784, 192)
    pooled = np.concatenate([tok.mean(axis=1), tok.max(axis=1), tok.std(axis=1)], axis=1)
    assert pooled.shape == (2, 576) and z["pooled"].shape == (2, 576)
    np.testing.assert_allclose(pooled, z["pooled"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(tok[:, z["token_rows"]], z["tokens"], rtol=1e-5, atol=1e-5)


def test_vit_generator_argument_checks():
    from relax_vqa_amd.extractor import visualise_vit_layer
    for p in (7, 12, 32):
        with pytest.raises(ValueError, match="8 and 16"):
            visualise_vit_layer.VitGenerator("vit_base", p, None)
    with pytest.raises(ValueError, match="No model found"):
        visualise_vit_layer.VitGenerator("vit_huge", 8, None)


def test_ctypes_table_has_the_new_entry_points():
    from relax_vqa_amd import _lib
    for name in ("relax_load_vit_ex", "relax_vit_geometry", "relax_op_attention_ex"):
        assert name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["relax_load_vit_ex"][1]) == len(_lib.PROTOTYPES["relax_load_vit"][1]) + 1
