"""ResNet-50 on any accepted canvas, the host half (csrc/host_logic.cpp: rn_canvas_geometry, rn_plan with a canvas): which canvases are taken
and what is said about the others, the map of every tap, the arena, and that every block runs a launch form whose kernel takes that block's
maps.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from tests import rn_schedule_checks as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP_CHANNELS = (64, 256, 256, 256, 512, 512, 512, 512, 1024, 1024, 1024, 1024, 2048, 2048, 2048)
CANVASES = ((64, 64), (64, 96), (96, 64), (96, 160), (288, 512), (448, 448), (1024, 64))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points (plain g++, no HIP), as tests/test_resnet_schedule_cpu.py builds it."""
    out = tmp_path_factory.mktemp("host_canvas") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.relax_host_rn_plan.restype = C.c_int
    lib.relax_host_rn_plan_canvas.restype = C.c_int
    lib.relax_host_rn_canvas_geometry.restype = C.c_int
    return lib


def geometry(lib, Hc, Wc):
    """([(h, w)] * 15, sizes dict), or the message of a refused canvas (and then nothing was written)."""
    taps = (C.c_int * 30)(*([-77] * 30))
    sizes = (C.c_int64 * 8)(*([-77] * 8))
    err = C.create_string_buffer(256)
    if lib.relax_host_rn_canvas_geometry(Hc, Wc, taps, sizes, err, 256) != 0:
        assert all(v == -77 for v in taps) and all(v == -77 for v in sizes), "a refused canvas must leave no geometry"
        return err.value.decode()
    names = ("x0", "big", "t1", "t2", "gap_ws", "block_max", "floats_f32", "floats_x6")
    return [(taps[2 * t], taps[2 * t + 1]) for t in range(15)], dict(zip(names, sizes))


def plan_canvas(lib, opts, req, Hc, Wc, max_slots=rc.IMG_SLOTS):
    n = 4 + 16 * len(rc.FIELDS)
    out = (C.c_int * n)(*([-77] * n))
    err = C.create_string_buffer(256)
    if lib.relax_host_rn_plan_canvas((C.c_int * 6)(*opts), (C.c_int * 5)(*req), Hc, Wc, max_slots, out, err, 256) != 0:
        assert all(v == -77 for v in out), "a refused plan must leave no plan"
        return err.value.decode()
    return list(out)


def all_options():
    for precision in (2, 3):
        for flags in itertools.product((0, 1), repeat=5):
            yield (precision,) + flags


def test_the_default_canvas_has_todays_tap_shapes_and_arena(host_lib):
    taps, sizes = geometry(host_lib, 224, 224)
    assert taps == [(s, s) for s in (112, 56, 56, 56, 28, 28, 28, 28, 14, 14, 14, 14, 7, 7, 7)]
    # the constants csrc/resnet50.hip carved its arena from before the canvas was an argument
    want = dict(x0=224 * 224 * 4, big=112 * 112 * 64, t1=56 * 56 * 128, t2=56 * 56 * 64, gap_ws=196 * 256, block_max=256)
    assert {k: sizes[k] for k in want} == want
    assert sizes["floats_f32"] == want["x0"] + 3 * want["big"] + want["t1"] + want["t2"] + want["gap_ws"] + 2048
    assert sizes["floats_x6"] == (want["x0"] + 3 * want["big"] + 2 * (want["big"] * 3 // 2) + (want["t1"] + want["t2"]) * 3 // 2 + want["gap_ws"] + 2048
                                  + 3 * 64 + 256)


@pytest.mark.parametrize("bad", (0, 32, 63, 100, 230, 1056, -64))
def test_a_refused_canvas_names_the_offending_value(host_lib, bad):
    for Hc, Wc, axis in ((bad, 224, "height"), (224, bad, "width"), (bad, bad, "height")):
        msg = geometry(host_lib, Hc, Wc)
        assert isinstance(msg, str) and f"canvas {axis} {bad} " in msg and f"(canvas {Hc} x {Wc})" in msg, msg
        assert "multiple of 32 in [64, 1024]" in msg
        # the plan refuses it with the same words, before it plans anything
        assert plan_canvas(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["clip"], Hc, Wc) == msg


def test_the_accepted_ends_and_every_tap_of_the_test_canvases(host_lib):
    for Hc, Wc in ((64, 64), (1024, 1024), (64, 1024)) + CANVASES:
        taps, sizes = geometry(host_lib, Hc, Wc)
        want = [(Hc // 2, Wc // 2)] + [(Hc // d, Wc // d) for d, n in ((4, 3), (8, 4), (16, 4), (32, 3)) for _ in range(n)]
        assert taps == want, (Hc, Wc)
        assert all(h >= 2 and w >= 2 for h, w in taps)
        assert (taps[0][0] * taps[0][1]) % 256 == 0                                   # whole stem tiles per image
        assert all(h % 2 == 0 and w % 2 == 0 for h, w in taps[:12])                   # every map in front of a stride is even
        # the workspace holds the two-stage mean's partial sums and every table of group sums a fused mean can write
        groups = [h * w // (16 if h * w % 16 == 0 else 4) * c for (h, w), c in zip(taps, TAP_CHANNELS) if h * w % 4 == 0]
        assert sizes["gap_ws"] == max([16 * 2048] + groups), (Hc, Wc)
        assert sizes["block_max"] >= taps[1][0] * taps[1][1] * 16 // 256 and sizes["block_max"] % 64 == 0
        assert all(v % 4 == 0 for v in sizes.values())                                # every carving stays 16-byte aligned


def test_the_plan_at_224_is_todays_int_for_int(host_lib):
    cases = 0
    for opts in all_options():
        for req in rc.REQUESTS.values():
            n = 4 + 16 * len(rc.FIELDS)
            out = (C.c_int * n)()
            err = C.create_string_buffer(256)
            assert host_lib.relax_host_rn_plan((C.c_int * 6)(*opts), (C.c_int * 5)(*req), rc.IMG_SLOTS, out, err, 256) == 0
            assert plan_canvas(host_lib, opts, req, 224, 224) == list(out), (opts, req)
            cases += 1
    assert cases == 320


def _check_forms(o, Hc, Wc, where):
    """Every block's form against the restated preconditions of its kernels, on that block's maps."""
    stem = dict(zip(("conv1_h2", "pool_f32", "s_stem", "n_slots"), o[:4]))
    blocks = [rc.Block(o[4 + i * len(rc.FIELDS):4 + (i + 1) * len(rc.FIELDS)]) for i in range(16)]
    # ---- slot budget: every slot below n_slots is handed out exactly once
    assert 0 <= stem["n_slots"] <= rc.IMG_SLOTS, where
    owned = [stem["s_stem"]] + [getattr(q, f) for q in blocks for f in ("s_c1", "s_t1", "s_t1m", "s_t2", "s_out", "s_dr_out")]
    assert sorted(s for s in owned if s >= 0) == list(range(stem["n_slots"])), where
    h, w = Hc // 4, Wc // 4
    if stem["s_stem"] >= 0:                     # layers.hip: per-image maxima need whole 256-thread blocks (4 channels per thread) per image
        assert (h * w * 16) % 256 == 0, where
    prev_form, prev_sample = (rc.F32 if stem["pool_f32"] else rc.SP3), rc.NO_SAMPLE
    for b, q in enumerate(blocks):
        stride, has_down = rc.GEOM[b][3], rc.GEOM[b][4]
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        at = (where, b, (ho, wo))
        assert (q.in_form, q.in_sample) == (prev_form, prev_sample), at
        if q.form in (rc.B2B, rc.B2BX2, rc.B2BDOWN):        # gemm_x6.hip: images of >= 256 pixels, a multiple of 16
            assert ho * wo >= 256 and (ho * wo) % 16 == 0 and q.in_form == rc.F32, at
        assert (q.form == rc.B2BDOWN) == (q.in_sample == rc.SAMPLE_H2), at
        if q.in_sample == rc.SAMPLE_SP3:
            assert q.form in (rc.X6, rc.EARLY) and has_down, at
        if q.fuse_mean:                                      # gemm_x6.hip / gemm_h2.hip: the fused spatial mean needs Ho*Wo % 4 == 0
            assert (ho * wo) % 4 == 0, at
        if q.form == rc.H2FORM and q.fuse_mean:              # (groups of 4 rows there; the finishing kernel reads groups of 16 where it can)
            assert (ho * wo) % 16 != 0, at
        if q.out_sample != rc.NO_SAMPLE:                     # gemm_x6.hip: the stride-2 plane output goes with even maps
            assert ho % 2 == 0 and wo % 2 == 0 and q.form in (rc.B2B, rc.B2BX2, rc.B2BDOWN), at
        if q.want_mean and not q.fuse_mean:
            assert q.need32, at                              # the mean of such a map is taken from the fp32 copy
        assert q.rows32 % (ho * wo) == 0, at
        prev_form, prev_sample = q.out_form, q.out_sample
        h, w = ho, wo
    assert (h, w) == (Hc // 32, Wc // 32)
    return stem, blocks


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: "%dx%d" % c)
def test_every_form_fits_its_blocks_maps(host_lib, canvas):
    Hc, Wc = canvas
    for opts in all_options():
        fixed = None
        for name, req in rc.REQUESTS.items():
            o = plan_canvas(host_lib, opts, req, Hc, Wc)
            assert isinstance(o, list), o
            stem, blocks = _check_forms(o, Hc, Wc, (canvas, opts, name))
            forms = [q.form for q in blocks]
            fixed = fixed or forms
            assert forms == fixed                            # the forms do not look at the request
            msg = plan_canvas(host_lib, opts, req, Hc, Wc, stem["n_slots"] - 1)
            assert isinstance(msg, str) and "%d per-image scale slots used" % stem["n_slots"] in msg


def test_the_smallest_canvas_keeps_layer1_back_to_back_and_not_layer2(host_lib):
    o = plan_canvas(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["layer stack + pool"], 64, 64)
    _, blocks = _check_forms(o, 64, 64, "64x64 default")
    assert [q.form for q in blocks[:3]] == [rc.B2BX2, rc.B2B, rc.B2B]           # 16 x 16 = 256 rows per image: the bound itself
    assert all(q.form == rc.EARLY for q in blocks[3:7])                         # 8 x 8
    assert all(q.form == rc.H2FORM for q in blocks[7:])
    assert blocks[2].out_sample == rc.SAMPLE_SP3 and blocks[3].in_sample == rc.SAMPLE_SP3
    # layer4's 2 x 2 maps: 4 rows per image, the fused mean's smallest group
    assert all(q.fuse_mean for q in blocks[13:])
    # 96 x 160: layer2 is 12 x 20 = 240 rows (below the bound), layer4 3 x 5 = 15 rows (no group of 4): the mean from the fp32 copy
    o = plan_canvas(host_lib, (3, 1, 1, 1, 1, 1), rc.REQUESTS["layer stack + pool"], 96, 160)
    _, blocks = _check_forms(o, 96, 160, "96x160 default")
    assert [q.form for q in blocks[:7]] == [rc.B2BX2, rc.B2B, rc.B2B] + [rc.EARLY] * 4
    assert not any(q.fuse_mean for q in blocks[13:]) and all(q.need32 for q in blocks[13:])
