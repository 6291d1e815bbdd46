"""host::vit_plan (csrc/host_logic.cpp), the routes and the arena layout that csrc/vit.hip's one forward executes, without a GPU: every route
field against its rule on a grid of options, models, token counts and requests, and the arena's slots - their order, alignment, the one
declared alias, their total."""
import ctypes as C
import itertools

import pytest

from tests import large_batch_cases, vit_plan_cases as vp

DEPTH = 12
TOKEN_COUNTS = (2, 61, 197, 198, 785, 4097)
REQUESTS = (dict(tokens=1, pooled=0), dict(tokens=0, pooled=1), dict(tokens=0, pooled=0, cls_attention=1), dict(tokens=0, pooled=1, cls_attention=1),
            dict(tokens=0, pooled=0, n_last=1), dict(tokens=0, pooled=0, n_last=DEPTH))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return large_batch_cases.host_library(tmp_path_factory.mktemp("host"))


@pytest.fixture(scope="module")
def grid(host_lib):
    """[(arguments, plan)] of every grid point, planned once"""
    points = []
    for precision, att_h2, att_h2_stream, dim, patch, ntok, rq in itertools.product((0, 1, 2, 3), (0, 1), (0, 1), (192, 256, 384, 768), (8, 16),
                                                                                    TOKEN_COUNTS, REQUESTS):
        kw = dict(precision=precision, att_h2=att_h2, att_h2_stream=att_h2_stream, dim=dim, depth=DEPTH, heads=dim // 64, patch=patch,
                  patch_k=3 * patch * patch, ntok=ntok, npatch=ntok - 1, **rq)
        points.append((kw, vp.plan(host_lib, **kw)))
    return points


def test_every_route_field_follows_its_rule(grid):
    seen_attention, seen_h2_embed = set(), set()
    for kw, p in grid:
        want = vp.expected_routes(kw["precision"], kw["att_h2"], kw["att_h2_stream"], kw["dim"], kw["patch"], kw["ntok"], kw["tokens"], kw["pooled"],
                                  kw.get("cls_attention", 0), kw.get("n_last", 0))
        assert {k: p[k] for k in vp.ROUTES} == want, kw
        seen_attention.add(p["attention"])
        if p["arith"] == vp.H2:
            seen_h2_embed.add(p["patch_embed"])
    assert seen_attention == set(vp.ATTENTION)              # each of the six attention kernels
    assert seen_h2_embed == {vp.X6, vp.H2}                  # both patch-embed routes under f16x2 (patch 8 / patch 16)


def test_arena_slots(host_lib, grid):
    """dim is a multiple of 64 (64-d heads) and patch_k = 3 p^2 a multiple of 64 (p = 8, 16), so the 3/2 floats per value of a plane slot
    are whole and every slot starts on a multiple of 4 floats (16 bytes) whatever the token count."""
    seen = set()
    for kw, p in grid:
        planes = p["arith"] != vp.F32
        seen.add(planes)
        td, pk, pe = kw["ntok"] * kw["dim"], kw["npatch"] * kw["patch_k"], kw["npatch"] * kw["dim"]
        order = ("patches", "embedded", "residual", "operand", "qkv", "final", "hidden") if planes else \
                ("patches", "embedded", "residual", "operand", "qkv", "hidden")
        size = {"patches": pk * 3 // 2 if planes else pk, "embedded": pe, "residual": td, "operand": td * 3 // 2 if planes else td, "qkv": 3 * td,
                "final": td, "hidden": 6 * td if planes else 4 * td}
        at = 0
        for s in order:                                     # the stated order, each slot of its stated size: none overlaps the next
            assert p[s] == at and at % 4 == 0, (kw, s, p)
            at += size[s]
        assert p["floats"] == at, (kw, p)                   # the last slot's end
        if not planes:
            assert p["final"] == p["operand"], (kw, p)      # the one declared alias
        assert vp.slot_sizes(p) == size, (kw, p)
        totals = (C.c_int64 * 2)()
        host_lib.relax_host_vit_arena_floats(kw["dim"], kw["ntok"], kw["npatch"], kw["patch_k"], totals)
        assert p["floats"] == totals[int(planes)] and totals[1] > totals[0], (kw, list(totals))
    assert seen == {False, True}


def test_the_totals_are_the_written_out_constants(host_lib):
    """tests/test_vit_geometry_cpu.py's constants, from the plan"""
    for dim, want in ((768, (1662720, 2267520)), (384, (906624, 1246656)), (192, (528576, 736224))):
        got = tuple(vp.plan(host_lib, precision=p, dim=dim, heads=dim // 64)["floats"] for p in (0, 2))
        assert got == want
    assert vp.plan(host_lib, patch=8, patch_k=192, ntok=785, npatch=784)["floats"] * 4 == 33455616
