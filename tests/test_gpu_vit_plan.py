"""csrc/vit.hip's forward runs what host::vit_plan says (tests/test_vit_plan_cpu.py checks the plan itself): the contraction launches the
profiler counts per kind are those the plan's routes imply, and the arena holds the plan's layout.  ViT-B/16 and ViT-B/8, N = 2, canvases
96 x 160 and 224 x 224, tail split off, on an engine of its own (the arena of a fresh handle is the observable).

Counts (the same on the commit before the one forward: profiles/vit_one_forward_digest_parent.json): the patch-embed GEMM and four GEMMs per
block, 1 + 4 depth launches, in the kind of the forward's arithmetic - fp32 / bf16x3 kind 0, bf16x6 kind 3, f16x2 kinds 7 and 9 -, the
patch-embed GEMM in kind 3 for patch 8 under f16x2; a forward for the CLS attention alone ends behind the last block's qkv GEMM:
1 + 4 (depth - 1) + 1.  The attention kernels are not contraction launches of the profiler."""
import numpy as np
import pytest
import torch

from relax_vqa_amd.engine import VIT_CONFIGS, RelaxEngine
from tests import large_batch_cases, vit_plan_cases as vp
from tests.gpu_common import ROUTE_KINDS, launches, synth

pytestmark = pytest.mark.gpu

N = 2
CANVASES = ((96, 160), (224, 224))
SETTINGS = ({"gemm_precision": 0}, {"gemm_precision": 2}, {"gemm_precision": 3}, {"gemm_precision": 3, "att_h2": 0},
            {"gemm_precision": 3, "att_h2_stream": 0})
KIND = {vp.F32: (0,), vp.X6: (3,), vp.H2: (7, 9)}          # read kinds a launch of an arithmetic is counted in (gpu_common.ROUTE_KINDS)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return large_batch_cases.host_library(tmp_path_factory.mktemp("host"))


@pytest.fixture(scope="module", params=[16, 8], ids=["patch16", "patch8"])
def model(request):
    """(a fresh engine with ViT-B of the patch size loaded, the model's plan arguments)"""
    eng = RelaxEngine(0)
    eng.set_option("gemm_split_k", 0)
    eng.load_vit(synth.vit_state_dict("vit_base", patch=request.param), "vit_base")
    dim, depth, heads = VIT_CONFIGS["vit_base"]
    yield eng, dict(dim=dim, depth=depth, heads=heads, patch=request.param, patch_k=3 * request.param ** 2)
    eng.close()


def _set(eng, opts):
    for key, value in {"att_h2": 1, "att_h2_stream": 1, **opts}.items():
        eng.set_option(key, value)
    return {"precision": opts["gemm_precision"], "att_h2": opts.get("att_h2", 1), "att_h2_stream": opts.get("att_h2_stream", 1)}


def _images(Hc, Wc):
    return torch.from_numpy(np.random.default_rng(Hc + Wc).integers(0, 256, (N, Hc, Wc, 3), dtype=np.uint8)).cuda()


def _expected(p, depth):
    want = dict.fromkeys(ROUTE_KINDS, 0)
    gemms = 4 * (depth - 1) + 1 if p["attention_only"] else 4 * depth
    for arith, count in ((p["patch_embed"], 1), (p["arith"], gemms)):
        for kind in KIND[arith]:
            want[kind] += count
    return want


def test_the_arena_holds_the_plans_layout(model, host_lib):
    """First test of the module for each model: the handle has run nothing yet.  The f16x2 forward with the tail split off takes no other
    workspace, so "workspace_mib" (every workspace of the handle, whole MiB) is the arena: plan.floats x 4 x N bytes; relax_reserve for N
    images and a second forward then allocate nothing more."""
    eng, m = model
    assert eng.get_option("workspace_mib") == 0
    o = _set(eng, {"gemm_precision": 3})
    img = _images(224, 224)
    ntok = eng.vit_canvas_geometry(224, 224)[2]
    p = vp.plan(host_lib, **o, **m, ntok=ntok, npatch=ntok - 1)
    eng.vit_features(img)
    torch.cuda.synchronize()
    assert eng.get_option("workspace_mib") == (p["floats"] * 4 * N) >> 20
    eng.reserve(N)                                          # (sized for ResNet-50 too, loaded or not: at least the ViT's share)
    reserved = eng.get_option("workspace_mib")
    assert reserved >= (p["floats"] * 4 * N) >> 20
    eng.vit_features(img)
    torch.cuda.synchronize()
    assert eng.get_option("workspace_mib") == reserved


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_launches_are_the_plans(model, host_lib, canvas):
    eng, m = model
    img = _images(*canvas)
    ntok = eng.vit_canvas_geometry(*canvas)[2]
    seen = set()
    for opts in SETTINGS:
        o = _set(eng, opts)
        runs = ((dict(tokens=1, pooled=1, cls_attention=1), lambda: eng.vit_features(img, tokens=True, attention=True)),
                (dict(tokens=0, pooled=0, cls_attention=1), lambda: eng.vit_attention(img)),
                (dict(tokens=0, pooled=0, n_last=3), lambda: eng.vit_intermediate_layers(img, n=3)))
        for rq, fn in runs:
            p = vp.plan(host_lib, **o, **m, ntok=ntok, npatch=ntok - 1, **rq)
            _, counts = launches(eng, fn)
            assert counts == _expected(p, m["depth"]), (opts, rq, p)
            seen.add((p["arith"], p["patch_embed"], p["attention_only"]))
    h2_embed = vp.X6 if m["patch"] == 8 else vp.H2
    assert seen == {(a, e, only) for a, e in ((vp.F32, vp.F32), (vp.X6, vp.X6), (vp.H2, h2_embed)) for only in (0, 1)}
