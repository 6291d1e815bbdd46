"""The launch schedule of a Farneback chunk is host logic (csrc/host_logic.cpp: flow_schedule; csrc/flow.hip's flow_chunk executes it): the
pyramid route of every level, how the coarser flow arrives, the iteration route with its bands and row segments, the ping-pong of the two flow
buffers, the carve of the workspace and the algorithmic bytes.  Checked here without a GPU: against the independent restatement of
tests/flow_param_space.py (route, segment_rows, box_band) field by field, on the flag sets, for invariants over a grid of sizes and
parameters, and for the bytes in closed form."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from tests import flow_flag_cases as gc
from tests import flow_param_cases as pc
from tests import flow_param_space as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEVELS, MAX_ITERS = 8, 10
HEAD = "n_levels iterations gray_form result gray tmp blur I R M flowA flowB mm pyr0 pyr1 pyr2 pyr3 arena_bytes".split()
LEVEL = "h w ksize pyramid resize up start poly_n poly_bands poly_seg iteration bands out_cols seg segments um_gx um_rows".split()
PER_LEVEL = len(LEVEL) + 3 * MAX_ITERS
PYRAMID = ("fused", "sampled", "sampled-wide", "gauss3_v4", "gauss_pass")
UP = (None, "resize_area_f32x2", "fused_x2", "resize_linear_f32<2>")
ITERATION = ("flow_iteration", "update_matrices_k+box_solve_fused", "update_matrices_k+box_solve_any", "update_matrices_k+gauss_solve_any")
GRAY = ("none", "flow_gray_v4", "flow_gray")
REGIONS = {"gray": 2, "tmp": 2, "blur": 2, "I": 2, "R": 10, "M": 5, "flowA": 2, "flowB": 2}      # floats per pixel and pair
FOUR_OPTIONS = list(itertools.product((1, 0), (1, 0)))      # (flow_fused, flow_pyramid_fused)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """csrc/host_logic.cpp alone with its test entry points, built into a temporary directory (plain g++, no HIP)."""
    out = tmp_path_factory.mktemp("host") / "libhost.so"
    src = os.path.join(ROOT, "relax-vqa_amd", "csrc", "host_logic.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DRELAX_HOST_TEST_API", src, "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    lib.relax_host_flow_schedule.restype = C.c_int
    lib.relax_host_flow_chunk_pairs.restype = C.c_int
    lib.relax_host_flow_chunk_pairs.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int]
    return lib


def torch_facts(H, W):
    """(pair_stride % 4 == 0, both frames 4-byte aligned, arena 16-byte aligned) of a contiguous uint8 [T, 2, H, W, 3] tensor on a 16-byte boundary"""
    return int(2 * H * W * 3 % 4 == 0), int(H * W * 3 % 4 == 0), 1


def schedule(lib, params, H, W, P=1, image=True, flow=True, init=False, facts=None, fused=1, pyramid_fused=1, seg_rows=0):
    """dict of the schedule (levels: a list of dicts, coarsest first, each with its `steps` [(in, out, minmax)] and scale, sigma, it_bytes,
    bytes), or the refusal's message (and then nothing was written)."""
    n_i, n_d = len(HEAD) + (MAX_LEVELS + 1) * PER_LEVEL, 1 + 4 * (MAX_LEVELS + 1)
    iout, dout = (C.c_int64 * n_i)(*([-77] * n_i)), (C.c_double * n_d)(*([-77.0] * n_d))
    err = C.create_string_buffer(256)
    par = (C.c_double * 2)(params["pyr_scale"], params["poly_sigma"])
    ipar = (C.c_int * 5)(params["levels"], params["winsize"], params["iterations"], params["poly_n"], params.get("flags", 0))
    req = (C.c_int * 9)(H, W, P, int(image), int(flow), int(init), *(facts or torch_facts(H, W)))
    rc = lib.relax_host_flow_schedule(par, ipar, req, (C.c_int * 3)(fused, pyramid_fused, seg_rows), iout, dout, err, 256)
    if rc != 0:
        assert rc == -1 and iout[0] == -77 and dout[0] == -77.0, "a refused schedule must leave no schedule"
        return err.value.decode()
    io, do = list(iout), list(dout)
    sc = dict(zip(HEAD, io))
    sc["bytes"] = do[0]
    sc["levels"] = []
    for i in range(sc["n_levels"] + 1):
        base = len(HEAD) + i * PER_LEVEL
        lv = dict(zip(LEVEL, io[base:]))
        steps = io[base + len(LEVEL):base + PER_LEVEL]
        lv["steps"] = [tuple(steps[3 * j:3 * j + 3]) for j in range(sc["iterations"])]
        lv.update(zip(("scale", "sigma", "it_bytes", "bytes"), do[1 + 4 * i:]))
        sc["levels"].append(lv)
    return sc


# ---- a. the independent restatement says the same, field by field ---------------------------------------------------------------------
def assert_route_agrees(lib, params, H, W, where):
    for fused, pyramid_fused in FOUR_OPTIONS:
        sc = schedule(lib, params, H, W, fused=fused, pyramid_fused=pyramid_fused)
        assert isinstance(sc, dict), (where, sc)
        try:
            r = sp.route(params, H, W, fused=bool(fused), pyramid_fused=bool(pyramid_fused))
        except ValueError:      # the table's route() stops at the wide kernels: the schedule must take them there
            assert "sampled-wide" in {PYRAMID[lv["pyramid"]] for lv in sc["levels"]}, where
            continue
        assert len(r) == sc["n_levels"] + 1, where
        for want, lv in zip(r, sc["levels"]):
            got = {"h": lv["h"], "w": lv["w"], "pyramid": PYRAMID[lv["pyramid"]], "up": UP[lv["up"]], "poly": lv["poly_n"],
                   "poly_bands": lv["poly_bands"], "iteration": ITERATION[lv["iteration"]], "bands": lv["bands"], "seg": lv["seg"],
                   "segments": lv["segments"]}
            assert got == {k: want[k] for k in got}, (where, fused, pyramid_fused, want["k"])
            assert lv["out_cols"] == sp.box_band(params["winsize"]) and lv["poly_bands"] == -(-lv["w"] // sp.POLY_BAND[lv["poly_n"]])
            assert lv["resize"] == (want["pyramid"] in ("gauss3_v4", "gauss_pass") and (lv["h"], lv["w"]) != (H, W))
            assert (lv["um_gx"], lv["um_rows"]) == (-(-lv["w"] // 256), -(-lv["h"] // 8))


def test_route_agrees_with_the_schedule_on_every_group_and_set(host_lib):
    for g in sp.GROUPS:
        assert_route_agrees(host_lib, g["params"], g["H"], g["W"], g["id"])
    wide = 0
    for name, (params, sizes) in pc.SETS.items():
        for H, W in sizes:
            assert_route_agrees(host_lib, params, H, W, name)
            wide += any(lv["pyramid"] == PYRAMID.index("sampled-wide") for lv in schedule(host_lib, params, H, W, pyramid_fused=0)["levels"])
    assert wide == 2      # deep4 and deep5


def test_segment_rows_over_a_grid_and_forced(host_lib):
    for win, bands, H in itertools.product((3, 9, 15, 33, 63), (1, 2, 3, 8, 16), (16, 29, 30, 31, 45, 135, 256, 271, 1080, 2160)):
        W = (bands - 1) * sp.box_band(win) + 17      # `bands` bands of the window's kernel
        p = {**pc.LITERAL, "levels": 0, "winsize": win}
        for fused in (1, 0):
            lv = schedule(host_lib, p, H, W, fused=fused)["levels"][0]
            assert (lv["bands"], lv["seg"], lv["segments"]) == (bands, sp.segment_rows(bands, H, win), -(-H // sp.segment_rows(bands, H, win))), (win, bands, H)
        for forced in (1, win, win + 1, 4 * win, 100):
            lv = schedule(host_lib, p, H, W, seg_rows=forced)["levels"][0]
            assert lv["seg"] == -(-forced // win) * win and lv["segments"] == -(-H // lv["seg"]), (win, forced)


# ---- b. the flag sets -------------------------------------------------------------------------------------------------------------------
def test_the_flag_bits_choose_their_kernels_whatever_flow_fused_says(host_lib):
    for name, (params, sizes) in gc.SETS.items():
        for (H, W), (fused, pyramid_fused) in itertools.product(sizes, FOUR_OPTIONS):
            sc = schedule(host_lib, params, H, W, init=bool(params["flags"] & 4), fused=fused, pyramid_fused=pyramid_fused)
            plain = schedule(host_lib, {**params, "flags": 0}, H, W, fused=fused, pyramid_fused=pyramid_fused)
            ups = [UP[lv["up"]] for lv in sc["levels"]]
            assert ups[0] == ("resize_area_f32x2" if params["flags"] & 4 else None) and "resize_area_f32x2" not in ups[1:] and None not in ups[1:], name
            assert ups[1:] == [UP[lv["up"]] for lv in plain["levels"]][1:]
            for lv, lv0 in zip(sc["levels"], plain["levels"]):
                if params["flags"] & 256:
                    assert ITERATION[lv["iteration"]] == "update_matrices_k+gauss_solve_any", (name, fused)
                    assert (lv["out_cols"], lv["seg"]) == (gc.TILE_W, gc.TILE_H) and (lv["bands"], lv["segments"]) == (-(-lv["w"] // gc.TILE_W), -(-lv["h"] // gc.TILE_H))
                else:
                    assert lv["iteration"] == lv0["iteration"] and (lv["bands"], lv["seg"]) == (lv0["bands"], lv0["seg"])
                assert lv["pyramid"] == lv0["pyramid"] and lv["poly_seg"] == lv0["poly_seg"]
    lit = {**pc.LITERAL, "flags": 256}
    assert {lv["iteration"] for f in (0, 1) for lv in schedule(host_lib, lit, 256, 264, fused=f)["levels"]} == {ITERATION.index("update_matrices_k+gauss_solve_any")}


# ---- c. invariants over a grid ------------------------------------------------------------------------------------------------------------
SIZES = [(16, 16), (31, 33), (33, 64), (97, 131), (128, 128), (256, 264), (540, 960), (1080, 1920), (2160, 3840), (2200, 2200), (16, 2200), (2200, 16)]
GRID_SCALES = (0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95)
GRID_WINDOWS, GRID_ITERATIONS, GRID_PAIRS = (3, 9, 15, 33, 63), (1, 2, 3, 10), (1, 2, 32)


def check_invariants(sc, H, W, P, image, up_x2):
    HW = H * W
    # the arena: disjoint regions in this order, the magnitude range behind them, all inside the arena's bytes
    at = 0
    for name, per_pixel in REGIONS.items():
        assert sc[name] == at, name
        at += per_pixel * P * HW
    assert sc["mm"] == at and 4 * at + 8 * P <= sc["arena_bytes"] == (108 * HW + 16) * P
    assert sc["blur"] % 4 == 0      # gauss3_v4's 16-byte stores, given the arena's base
    # pyramid_fused's outputs: level k holds 2 P frames of (H / 2^k) x (W / 2^k) floats where it is put
    assert [sc["pyr0"], sc["pyr1"], sc["pyr2"]] == [sc["blur"], sc["I"], sc["tmp"]] and sc["pyr3"] == sc["tmp"] + 2 * P * (HW // 16)
    assert sc["pyr3"] + 2 * P * (HW // 64) <= sc["blur"]
    # the ping-pong
    result = None
    for i, lv in enumerate(sc["levels"]):
        steps = lv["steps"]
        assert lv["start"] == (0 if result is None else 1 - result)
        if UP[lv["up"]] == "fused_x2":
            assert i > 0 and steps[0][0] == result and steps[0][1] != result, "the x 2 read never reads the buffer it writes"
        else:
            assert steps[0][0] == lv["start"] and (i == 0) == (UP[lv["up"]] in (None, "resize_area_f32x2"))
        assert (UP[lv["up"]] == "fused_x2") == (i > 0 and up_x2)
        for a, b in zip(steps, steps[1:]):
            assert b[0] == a[1], "an iteration reads what the previous one wrote"
        if ITERATION[lv["iteration"]] == "flow_iteration":
            assert all(s[0] != s[1] for s in steps), "flow_iteration never works in place"
        else:
            assert all(s[0] == s[1] for s in steps[1:]) and steps[0][1] == lv["start"]
        minmax = [s[2] for s in steps]
        assert minmax == [0] * (len(steps) - 1) + [int(image and i == sc["n_levels"])], "the magnitude range rides on the last iteration of level 0"
        result = steps[-1][1]
    assert sc["result"] == result
    assert sc["bytes"] >= sum(lv["bytes"] for lv in sc["levels"]) > 0


def test_every_accepted_plan_gets_a_schedule_with_its_invariants(host_lib):
    import relax_vqa_amd  # noqa: F401
    schedules = 0
    for (H, W), ps, levels in itertools.product(SIZES, GRID_SCALES, range(MAX_LEVELS + 1)):
        try:
            plan = sp.plan(H, W, ps, levels)
        except RuntimeError as e:
            msg = schedule(host_lib, {**pc.LITERAL, "pyr_scale": ps, "levels": levels}, H, W)
            assert msg == str(e).split(": ", 1)[1], "flow_plan's refusal, word for word"
            continue
        for k, (win, iters) in enumerate(itertools.product(GRID_WINDOWS, GRID_ITERATIONS)):
            p = {**pc.LITERAL, "pyr_scale": ps, "levels": levels, "winsize": win, "iterations": iters, "poly_n": 5 + 2 * (k % 2), "flags": 256 * (k % 3 == 0)}
            image, fused, pyramid_fused = bool((k + levels) % 2), (k // 2) % 2, (k // 4) % 2
            per_pair = []
            for P in GRID_PAIRS:
                sc = schedule(host_lib, p, H, W, P=P, image=image, fused=fused, pyramid_fused=pyramid_fused)
                assert isinstance(sc, dict), ("flow_plan accepts it, the schedule must", H, W, p, sc)      # the in-loop refusals are unreachable
                assert [(lv["h"], lv["w"], lv["ksize"], lv["sigma"]) for lv in sc["levels"]] == list(plan)
                check_invariants(sc, H, W, P, image, ps == 0.5)
                assert sc["bytes"] == pytest.approx(P * per_pair[0][1], rel=1e-14) if per_pair else True
                per_pair.append(([{k_: v for k_, v in lv.items() if k_ not in ("poly_seg", "bytes", "it_bytes")} for lv in sc["levels"]], sc["bytes"] / P, sc["gray_form"], sc["result"]))
                schedules += 1
            assert all(q[0] == per_pair[0][0] and q[2:] == per_pair[0][2:] for q in per_pair), "apart from poly_expansion's rows per block a pair's schedule does not depend on P"
    assert schedules > 30000


def test_poly_expansion_rows_per_block_follow_the_launch(host_lib):
    """64 rows, 16 fewer while bands x segments x 2 P stays under 2048 blocks."""
    for (H, W), P in itertools.product(((97, 131), (256, 264), (1080, 1920), (2160, 3840)), GRID_PAIRS):
        for lv in schedule(host_lib, pc.LITERAL, H, W, P=P)["levels"]:
            seg = 64
            while seg > 16 and lv["poly_bands"] * -(-lv["h"] // seg) * P * 2 < 2048:
                seg -= 16
            assert lv["poly_seg"] == seg


def test_the_two_gigabyte_refusal_starts_where_forty_bytes_per_pixel_reach_it(host_lib):
    first = -(-(2 ** 31 - 1) // 40)      # the first HW with HW * 40 >= 2^31 - 1

    def frame(hw, step):      # the nearest H x W = hw' from hw on in direction `step` with both sides >= 16 and H within reach of one level
        while True:
            for W in range(4096, 8192):
                if hw % W == 0:
                    return hw // W, W
            hw += step

    H, W = frame(first - 1, -1)
    assert first - 64 < H * W < first and isinstance(schedule(host_lib, {**pc.LITERAL, "levels": 0}, H, W), dict)
    H, W = frame(first, 1)
    assert first <= H * W < first + 64
    assert schedule(host_lib, {**pc.LITERAL, "levels": 0}, H, W) == f"frames of {W} x {H} exceed the 2 GB a buffer resource addresses (40 bytes per pixel)"


def test_gray_form_and_the_vector_kernels_follow_the_facts(host_lib):
    sc = schedule(host_lib, pc.LITERAL, 256, 264)
    assert GRAY[sc["gray_form"]] == "none" and {PYRAMID[lv["pyramid"]] for lv in sc["levels"]} == {"fused"}
    for facts in ((0, 1, 1), (1, 0, 1)):      # a pair stride or a frame off the 4-byte grid: no pyramid_fused, no flow_gray_v4
        sc = schedule(host_lib, pc.LITERAL, 256, 264, facts=facts)
        assert GRAY[sc["gray_form"]] == "flow_gray" and [PYRAMID[lv["pyramid"]] for lv in sc["levels"]] == ["sampled", "sampled", "gauss3_v4", "gauss3_v4"]
    sc = schedule(host_lib, pc.LITERAL, 256, 264, facts=(1, 1, 0))      # the arena off the 16-byte grid: pyramid_fused still (it asks 4 bytes of the frames)
    assert GRAY[sc["gray_form"]] == "none"
    sc = schedule(host_lib, pc.LITERAL, 256, 264, facts=(1, 1, 0), pyramid_fused=0)
    assert GRAY[sc["gray_form"]] == "flow_gray" and [PYRAMID[lv["pyramid"]] for lv in sc["levels"]] == ["sampled", "sampled", "gauss_pass", "gauss_pass"]
    assert GRAY[schedule(host_lib, pc.LITERAL, 256, 264, pyramid_fused=0)["gray_form"]] == "flow_gray_v4"
    assert GRAY[schedule(host_lib, pc.LITERAL, 97, 131, facts=(1, 1, 1))["gray_form"]] == "flow_gray"      # an odd pixel count


def test_chunk_pairs(host_lib):
    """What 32 GB hold at 112 bytes per pixel and pair - no less than the carve's 108 per pixel + 16 per pair -, capped by flow_max_pairs and T."""
    f = host_lib.relax_host_flow_chunk_pairs
    assert f(1080, 1920, 32, 0, 1000) == (32 << 30) // (1080 * 1920 * 112) == 147 and f(1080, 1920, 32, 0, 32) == 32
    assert f(1080, 1920, 32, 2, 3) == 2 and f(1080, 1920, 1, 0, 3) == 3 and f(2160, 3840, 1, 0, 3) == 1 and f(7000, 7000, 1, 0, 3) == 1
    for H, W in SIZES:
        for T in (1, 3, 32, 100000):
            chunk = f(H, W, 32, 0, T)
            arena = schedule(host_lib, {**pc.LITERAL, "levels": 0}, H, W, P=chunk)["arena_bytes"]
            assert 1 <= chunk <= T and (arena <= 32 << 30 or chunk == 1)


# ---- d. the bytes in closed form ---------------------------------------------------------------------------------------------------------
def test_stage_bytes_in_closed_form(host_lib):
    for (H, W), P in itertools.product(((256, 264), (1080, 1920), (2160, 3840)), (1, 2, 32)):
        HW = H * W
        levels = [(H >> k) * (W >> k) for k in range(4)]      # exact: sides are multiples of 8
        want = 2 * P * HW * (3 + 4 * (1 + 1 / 4 + 1 / 16 + 1 / 64))      # the frames, the four level inputs
        want += sum(2 * P * hw * 24 for hw in levels)                    # poly_expansion: 24 B per pixel and frame
        want += sum(3 * P * hw * 56 for hw in levels)                    # flow_iteration: 56 B per pixel and iteration
        sc = schedule(host_lib, pc.LITERAL, H, W, P=P, image=False)
        assert sc["bytes"] == want == sp.stage_bytes(pc.LITERAL, H, W, P, image=False)
        with_image = schedule(host_lib, pc.LITERAL, H, W, P=P)
        assert with_image["bytes"] == want + 11 * P * HW == sp.stage_bytes(pc.LITERAL, H, W, P)
        assert [lv["it_bytes"] for lv in sc["levels"]] == [56 * P * hw for hw in reversed(levels)]
    # the two-kernel route: 68 + 28 B per pixel and iteration in place of 56
    sc = schedule(host_lib, pc.LITERAL, 256, 264, P=2, fused=0)
    assert sc["bytes"] == sp.stage_bytes(pc.LITERAL, 256, 264, 2, fused=False) == sp.stage_bytes(pc.LITERAL, 256, 264, 2) + 2 * 3 * 40 * sum((256 >> k) * (264 >> k) for k in range(4))
    assert [lv["it_bytes"] for lv in sc["levels"]] == [68 * 2 * (256 >> k) * (264 >> k) for k in (3, 2, 1, 0)]
    # a per-level pyramid with resize_linear_f32<2> between the levels and box_solve_any: written out for 79 x 246, one pair, one iteration
    p = dict(pyr_scale=0.8, levels=4, winsize=9, iterations=1, poly_n=5, poly_sigma=1.2)
    sizes = [(h, w) for h, w, _, _ in sp.plan(79, 246, 0.8, 4)]
    assert sizes == [(32, 101), (40, 126), (51, 157), (63, 197), (79, 246)]
    HW, hws = 79 * 246, [h * w for h, w in sizes]
    want = 2 * HW * 7 + 11 * HW                                                      # gray; the image
    want += sum(2 * (4 * HW + 4 * hw) for hw in hws) + 2 * 8 * HW * 3                  # five blurs (+ the full-size blur kept for the resize at 0.8, 0.64, 0.512)
    want += sum(8 * (a + b) for a, b in zip(hws, hws[1:]))                            # four pyramid steps
    want += sum(2 * hw * 24 + hw * (68 + 28) for hw in hws)
    assert [PYRAMID[lv["pyramid"]] for lv in schedule(host_lib, p, 79, 246)["levels"]] == ["sampled", "gauss_pass", "gauss_pass", "gauss_pass", "gauss_pass"]
    assert schedule(host_lib, p, 79, 246)["bytes"] == want == sp.stage_bytes(p, 79, 246, 1)
    # every group of the table, every option
    for g, (fused, pyramid_fused) in itertools.product(sp.GROUPS, FOUR_OPTIONS):
        sc = schedule(host_lib, g["params"], g["H"], g["W"], P=3, fused=fused, pyramid_fused=pyramid_fused)
        assert sc["bytes"] == sp.stage_bytes(g["params"], g["H"], g["W"], 3, fused=bool(fused), pyramid_fused=bool(pyramid_fused)), g["id"]
