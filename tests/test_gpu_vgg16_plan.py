"""csrc/vgg16.hip's forward runs what host::vgg_plan says (tests/test_vgg16_plan_cpu.py checks the plan itself): the contraction launches the
profiler counts per kind are those the plan's routes imply, the arena holds the plan's layout, and an image's rows do not depend on which
chunk of 32 it falls into.  Synthetic weights, tail split off, on an engine of its own (the arena of a fresh handle is the observable).

Counts: conv1_1 and the pools are no contraction launches; the other 12 convolutions and, where the classifier runs, fc1 and fc2 are one
launch each in the kind of their route - fp32 kind 0, bf16x6 kind 3, f16x2 kind 7 (all of the convolution form: none in kind 9)."""
import ctypes as C

import numpy as np
import pytest
import torch

from relax_vqa_amd.engine import RelaxEngine
from tests import large_batch_cases, vgg_plan_cases as vp
from tests.gpu_common import ROUTE_KINDS, launches, synth

pytestmark = pytest.mark.gpu

N = 2


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return large_batch_cases.host_library(tmp_path_factory.mktemp("host"))


@pytest.fixture(scope="module")
def eng():
    e = RelaxEngine(0)
    e.set_option("gemm_split_k", 0)
    e.load_vgg16(synth.vgg16_state_dict())
    yield e
    e.close()


def _images(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)).cuda()


def test_the_arena_holds_the_plans_layout(eng, host_lib):
    """First test of the module: the handle has run nothing yet.  The f16x2 forward with the tail split off takes no other workspace, so
    "workspace_mib" (every workspace of the handle, whole MiB) is the arena: plan.floats x 4 x N bytes; relax_reserve for N images and a
    second forward then allocate nothing more."""
    assert eng.get_option("workspace_mib") == 0
    eng.set_option("gemm_precision", 3)
    img = _images(N, 1)
    _, _, arena = vp.plan(host_lib, 3, (N, 1, 1, 0))
    eng.vgg16_features(img)
    torch.cuda.synchronize()
    assert eng.get_option("workspace_mib") == (arena["floats"] * 4 * N) >> 20
    # relax_reserve sizes the arena for ResNet-50 at its canvas too, loaded or not: the larger of the two shares and nothing beyond it
    sizes = (C.c_int64 * 8)()
    assert host_lib.relax_host_rn_canvas_geometry(224, 224, None, sizes, None, 0) == 0
    eng.reserve(N)
    reserved = eng.get_option("workspace_mib")
    assert reserved == (max(arena["floats"], sizes[6], sizes[7]) * 4 * N) >> 20 == (arena["floats"] * 4 * N) >> 20
    eng.vgg16_features(img)
    torch.cuda.synchronize()
    assert eng.get_option("workspace_mib") == reserved


@pytest.mark.parametrize("precision", [0, 2, 3])
def test_launches_are_the_plans(eng, host_lib, precision):
    eng.set_option("gemm_precision", precision)
    img = _images(N, 2)
    try:
        for ls, pool in ((1, 1), (0, 1), (1, 0)):
            head, rows, _ = vp.plan(host_lib, precision, (N, ls, pool, 0))
            want = dict.fromkeys(ROUTE_KINDS, 0)
            for q in rows:
                if q.route in vp.ROUTE_KIND:
                    want[vp.ROUTE_KIND[q.route]] += 1
            assert sum(want.values()) == (14 if pool else 12) and head["classifier"] == pool
            _, counts = launches(eng, lambda: eng.vgg16_features(img, layer_stack=bool(ls), pool=bool(pool)))
            assert counts == want, (precision, ls, pool)
    finally:
        eng.set_option("gemm_precision", 3)


@pytest.mark.parametrize("precision", [3, 0])
def test_rows_do_not_depend_on_the_chunk(eng, precision):
    """N = 33 is one chunk of 32 images and one of 1: the last image of the first chunk, the only one of the second and image 0 give the same
    bits alone - layer stack, pool vector, a convolution tap (NCHW export), one in front of a pool, fc1 and fc2."""
    eng.set_option("gemm_precision", precision)
    taps = (0, 3, 13, 14)
    try:
        batch = _images(33, 3)
        ls, pool, t = eng.vgg16_features(batch, taps=taps)
        for i in (0, 31, 32):
            ls1, pool1, t1 = eng.vgg16_features(batch[i:i + 1].contiguous(), taps=taps)
            assert torch.equal(ls1[0], ls[i]) and torch.equal(pool1[0], pool[i]), (precision, i)
            for k in taps:
                assert torch.equal(t1[k][0], t[k][i]), (precision, i, k)
    finally:
        eng.set_option("gemm_precision", 3)
