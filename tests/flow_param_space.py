"""Farneback's six parameters in combination, at their limits and at the band and segment edges of the kernels they select: the fixed
table of cases shared by tests/test_flow_param_space_cpu.py, tests/test_gpu_flow_param_space.py and tools/flow_param_space_parity.py.

tests/flow_param_cases.py moves one parameter at a time away from the literal set; every parameter switches a different launch of
flow_chunk (csrc/flow.hip), so those sets reach a small part of the dispatch lattice.  The groups here are constructed so that the
launches meet: poly_expansion<7> before box_solve_any, resize_linear_f32<2> before update_matrices_k<false> + box_solve_any, pyramid_fused
before box_solve_any, the sampled pyramid kernels at pyr_scale 0.6, 0.7 and 0.8, nine-level pyramids at pyr_scale 0.95, ten iterations,
one iteration per level on every route, widths one column either side of every kernel's band, heights one row either side of a row
segment, frames shorter than the window.  A group is (parameters, H, W) and runs in one GPU call; a case is a group and a content
(flow_param_cases.SMOOTH / SECOND / THIRD through pair_case).  Sizes follow from the parameters and are the smallest that still reach the
code.  What stays outside: the 39- and 79-tap wide pyramid kernels in combination (deep4 / deep5 of flow_param_cases.py run them alone),
2160p frames, and poly_sigma outside 1.1 .. 2.0.

route() restates, as a pure function of (parameters, H, W), which launches flow_chunk takes (the conditions of csrc/flow.hip, on the level
sizes relax_flow_plan returns); the coverage assertions of tests/test_flow_param_space_cpu.py count on it.  It is a table in the tests, not a
probe of the binary: tests/test_flow_schedule_cpu.py holds it, field by field, to the schedule flow_chunk executes (host::flow_schedule,
csrc/host_logic.cpp), so a condition that changes there without changing here fails on the CPU."""
import ctypes as C
import functools

import numpy as np

from tests import flow_param_cases as pc

SEED = 20240607
PYR_SCALES = (0.5, 0.6, 0.7, 0.8, 0.95)
LEVELS = (0, 1, 2, 3, 4, 8)
WINSIZES = (5, 7, 9, 13, 15, 17, 21, 31, 45, 61, 63)      # and 3 in one case, bits only
ITERATIONS = (1, 2, 3, 10)
POLY_NS = (5, 7)
POLY_SIGMAS = (1.1, 1.2, 1.5, 2.0)
CONTENTS = {"smooth": pc.SMOOTH, "second": pc.SECOND, "rotzoom": pc.THIRD}

POLY_BAND = {5: 246, 7: 242}       # output columns per block of poly_expansion<N>: 256 - 2 N
FUSED_BAND = 240                   # box_solve_fused and flow_iteration (FUSE_OUT, IT_OUT)
MAX_GAUSS, GH_SEG = 32, 1280       # past either, the wide instantiations of the sampled pyramid kernels: out of scope here


def box_band(winsize):
    """Output columns per block of the case's box kernel."""
    return FUSED_BAND if winsize == 15 else (256 - 2 * (winsize // 2)) & ~3


def height_classes(winsize):
    return {"16": 16, "2w-1": 2 * winsize - 1, "2w": 2 * winsize, "2w+1": 2 * winsize + 1, "4w+1": 4 * winsize + 1}


def min_side(pyr_scale, k):
    """The smallest side whose level k is still used: side * pyr_scale^k >= 32 (128 for two levels at 0.5, 44 for six at 0.95)."""
    n = 16
    while n * pyr_scale ** k < 32:
        n += 1
    return n


# ---- the table ---------------------------------------------------------------------------------------------------------------------
# (pyr_scale, levels, winsize, iterations, poly_n, H, W, what the group is there for).  poly_sigma and which groups carry the rot-zoom pair
# as a third content are drawn from default_rng(SEED); everything else is constructed.  oc = box_band(winsize), pb = POLY_BAND[poly_n].
# A ninth entry names the contents where the drawn ones miss an input condition of tests/test_flow_param_space_cpu.py - a content is replaced,
# the bits-only group is not widened.  Measured: winsize 5 at 0.8 under the noisy shift, max |fp32 - fp64| 1.02e-3; winsize 13 at 0.6 under it,
# 1.1e-2; winsize 13 on 25 rows under the smooth shift, 1.66e-3; winsize 45 on 91 rows, mean |fp32 - fp64| 9.2e-8 under the smooth shift and
# 8.1e-8 under the rot-zoom; winsize 63 under the rot-zoom, max |flow| 0.6 px.
_ROWS = [
    # -- the sixteen combinations of (pyr_scale 0.5 or not, winsize 15 or not, poly_n, one iteration or more), each on a pyramid
    (0.5, 2, 15, 1, 5, 128, 239, "flow_iteration<true,true> on two levels; W = oc - 1"),
    (0.5, 1, 15, 2, 5, 64, 240, "W = oc"),
    (0.5, 2, 15, 1, 7, 128, 241, "poly7 into flow_iteration, one iteration; W = oc + 1 = pb - 1"),
    (0.5, 1, 15, 10, 7, 64, 242, "ten iterations ping-pong on flow_iteration; W = pb"),
    (0.5, 3, 9, 1, 5, 256, 264, "pyramid_fused into box_solve_any<true>, one iteration per level"),
    (0.5, 2, 21, 3, 5, 128, 473, "W = 2 oc + 1: level 1 is exactly one band wide"),
    (0.5, 1, 13, 1, 7, 64, 243, "poly7 into box_solve_any; W = oc - 1 = pb + 1"),
    (0.5, 4, 31, 2, 7, 256, 264, "pyramid_fused + poly7 + box_solve_any; the fourth level is cut by the 32-pixel stop"),
    (0.8, 4, 15, 1, 5, 79, 246, "resize_linear_f32<2> into flow_iteration<false,true>; sampled level at 0.8^4; W = pb"),
    (0.6, 2, 15, 3, 5, 89, 245, "sampled level at 0.36; W = pb - 1"),
    (0.7, 2, 15, 1, 7, 66, 241, "sampled level at 0.49, poly7; W = oc + 1 = pb - 1"),
    (0.95, 8, 15, 2, 7, 49, 240, "nine levels of 3-tap blur + resize; W = oc"),
    (0.7, 2, 7, 1, 5, 66, 247, "resize_linear_f32<2> into update_matrices_k<false> + box_solve_any<true>; W = oc - 1 = pb + 1"),
    (0.6, 2, 17, 2, 5, 89, 240, "W = oc (17: the same 240 columns as the fused kernels, another kernel)"),
    (0.8, 4, 5, 1, 7, 79, 253, "smallest gated window, poly7 wider than the window; W = oc + 1", ("smooth", "rotzoom")),
    (0.95, 8, 45, 3, 7, 181, 212, "nine levels under a 45-pixel window; H = 4 w + 1, W = oc"),
    # -- every pyr_scale with a window under, at and over 15
    (0.6, 3, 13, 2, 5, 149, 244, "two sampled levels (0.36, 0.216); W = oc", ("smooth", "rotzoom")),
    (0.7, 4, 61, 2, 5, 134, 197, "three sampled levels; the window wider than every coarse level is high; W = oc + 1"),
    (0.8, 2, 63, 3, 5, 127, 191, "largest window; H = 2 w + 1, W = oc - 1", ("smooth", "second")),
    (0.95, 8, 9, 10, 5, 49, 249, "ten iterations on box_solve_any over nine levels; W = oc + 1"),
    # -- heights at a row segment's edge, windows under 15
    (0.5, 0, 9, 3, 5, 16, 248, "H = 16; W = oc"),
    (0.5, 1, 13, 2, 7, 25, 245, "H = 2 w - 1; W = oc + 1; levels = 1 is dead at this height", ("rotzoom", "second")),
    (0.5, 0, 9, 2, 5, 18, 497, "H = 2 w; W = 2 oc + 1: three bands, the last one column wide"),
    (0.5, 0, 13, 3, 5, 27, 246, "H = 2 w + 1: a second segment of one row; W = pb"),
    (0.8, 2, 13, 1, 7, 53, 242, "H = 4 w + 1 on three levels; W = pb"),
    # -- the same, windows over 15; frames shorter than the window
    (0.5, 0, 31, 2, 5, 16, 224, "H = 16 < winsize; W = oc"),
    (0.95, 4, 21, 3, 5, 41, 235, "H = 2 w - 1 on five levels; W = oc - 1"),
    (0.95, 1, 17, 1, 5, 34, 241, "H = 2 w on two levels; W = oc + 1"),
    (0.5, 2, 45, 2, 7, 91, 213, "H = 2 w + 1; W = oc + 1; the second level is cut by the 32-pixel stop", ("second",)),
    (0.7, 3, 31, 2, 5, 125, 449, "H = 4 w + 1; W = 2 oc + 1 with resize_linear_f32<2>"),
    (0.5, 0, 21, 10, 7, 16, 236, "H = 16 < winsize, ten iterations; W = oc"),
    # -- the rest of the widths
    (0.5, 3, 15, 2, 5, 128, 481, "W = 2 oc + 1 on the fused kernels: three bands"),
    (0.5, 1, 3, 2, 5, 64, 252, "smallest window: bits only", ("smooth",)),
]


COMBINATION_ROWS = 16


def _id(p, H, W):
    return f"s{p['pyr_scale']:g}-l{p['levels']}-w{p['winsize']}-i{p['iterations']}-n{p['poly_n']}-g{p['poly_sigma']:g}-{H}x{W}"


def _build():
    g = np.random.default_rng(SEED)
    # poly_sigma in a drawn order: 1.5 or 2.0 on the sixteen combination rows, where poly_n must be live (dead_parameters), every value after them
    wide = [POLY_SIGMAS[2 + i] for i in g.permutation(np.arange(COMBINATION_ROWS) % 2)]
    sigmas = wide + [POLY_SIGMAS[i] for i in g.permutation(np.arange(len(_ROWS) - COMBINATION_ROWS) % len(POLY_SIGMAS))]
    third = g.random(len(_ROWS)) < 0.3
    groups = []
    for i, (ps, lv, win, it, pn, H, W, why, *named) in enumerate(_ROWS):
        params = dict(zip(pc.KEYS, (ps, lv, win, it, pn, 1.2 if win == 3 else float(sigmas[i]))))      # (3: flow_param_cases.py's win3 set)
        contents = named[0] if named else ["smooth", "second"] + (["rotzoom"] if third[i] and win >= 15 else [])
        groups.append({"id": _id(params, H, W), "params": params, "H": H, "W": W, "contents": tuple(contents), "why": why})
    return groups


GROUPS = _build()
GROUP_IDS = [g["id"] for g in GROUPS]
BY_ID = {g["id"]: g for g in GROUPS}
CASES = [(g["id"], c) for g in GROUPS for c in g["contents"]]      # (group id, content name)


def case_id(case):
    return f"{case[0]}-{case[1]}"


def pair_of(case):
    """The flow_cases.make_pair case of a table case."""
    g = BY_ID[case[0]]
    return pc.pair_case((g["H"], g["W"]), CONTENTS[case[1]])


def batch_of(group):
    """The pairs of a group's one GPU call, in the order of its contents."""
    return [pc.pair_case((group["H"], group["W"]), CONTENTS[c]) for c in group["contents"]]


def reference(case):
    """-> (float64 oracle, float32 oracle) of a table case under its own parameters, computed once"""
    return pc.reference(BY_ID[case[0]]["params"], pair_of(case))


# Cases outside the parity gate: finite, inside the absolute bound of test_flow_on_small_and_odd_frames (the 3-pixel window: finite), and every bit check.  Each
# states which input condition of tests/test_flow_param_space_cpu.py it misses; that test asserts that it does miss it.
BITS_ONLY = {
    (g["id"], "smooth"): "not well posed: a 3 x 3 window leaves the 2 x 2 system nearly singular in flat regions (max |fp32 - fp64| 6.4e-3)"
    for g in GROUPS if g["params"]["winsize"] == 3
}
BITS_ONLY_SHARE = 0.10


# ---- the plan and the restated dispatch ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan(H, W, pyr_scale, levels):
    """relax_flow_plan (no GPU): ((h, w, ksize, sigma), ...) coarsest first"""
    from relax_vqa_amd import _lib
    lib = _lib.load()
    n = C.c_int(-1)
    hwk = (C.c_int32 * 27)()
    sig = (C.c_double * 9)()
    rc = lib.relax_flow_plan(H, W, pyr_scale, levels, C.byref(n), C.cast(hwk, C.c_void_p), C.cast(sig, C.c_void_p))
    if rc != 0:
        raise RuntimeError(lib.relax_last_error(None).decode())
    return tuple((hwk[3 * i], hwk[3 * i + 1], hwk[3 * i + 2], sig[i]) for i in range(n.value + 1))


def segment_rows(bands, h, winsize):
    """flow_segment_rows with flow_seg_rows = 0"""
    for mult in (18, 9, 6, 4, 3):
        if bands * -(-h // (mult * winsize)) >= 16:
            return mult * winsize
    return 2 * winsize


def route(params, H, W, fused=True, pyramid_fused=True):
    """The launches of flow_chunk per level, coarsest first, for torch's 16-byte aligned contiguous frames: a list of dicts
         k           the level (0: full size); scale = pyr_scale^k
         h, w        its size
         pyramid     how the level's input is made: 'fused' (pyramid_fused, all levels in one launch), 'sampled' (gauss_h_sampled +
                     gauss_v_sampled_resize), 'gauss3_v4' or 'gauss_pass' (+ resize_linear_f32<1> below full size)
         ratio       W / w of a sampled level
         up          how the coarser flow arrives: None (coarsest: zeros), 'fused_x2' (read inside the first matrix update) or 'resize_linear_f32<2>'
         poly        5 or 7; poly_bands
         iteration   'flow_iteration', 'update_matrices_k+box_solve_fused' or 'update_matrices_k+box_solve_any'
         bands, seg  columns bands and rows per block of the box kernel; segments = ceil(h / seg)"""
    ps, win = params["pyr_scale"], params["winsize"]
    pl = plan(H, W, ps, params["levels"])
    used = len(pl) - 1
    pyr = pyramid_fused and used == 3 and ps == 0.5 and H % 8 == 0 and W % 8 == 0
    out = []
    for i, (h, w, ksize, _) in enumerate(pl):
        k = used - i
        sampled = ps ** k < 0.5
        if ksize > MAX_GAUSS or (sampled and 129.0 * W / w + ksize + 4 > GH_SEG):
            raise ValueError(f"level {k} of {H} x {W} at pyr_scale {ps} takes the wide pyramid kernels: out of this table's scope")
        if pyr:
            pyramid = "fused"
        elif sampled:
            pyramid = "sampled"
        else:
            pyramid = "gauss3_v4" if W % 4 == 0 else "gauss_pass"      # (scale >= 1/2: three taps)
        if win != 15:
            iteration = "update_matrices_k+box_solve_any"
        else:
            iteration = "flow_iteration" if fused else "update_matrices_k+box_solve_fused"
        bands = -(-w // box_band(win))
        seg = segment_rows(bands, h, win)
        out.append({"k": k, "h": h, "w": w, "pyramid": pyramid, "ratio": W / w if sampled else None,
                    "up": None if i == 0 else ("fused_x2" if ps == 0.5 else "resize_linear_f32<2>"),
                    "poly": params["poly_n"], "poly_bands": -(-w // POLY_BAND[params["poly_n"]]),
                    "iteration": iteration, "bands": bands, "seg": seg, "segments": -(-h // seg)})
    return out


def stage_bytes(params, H, W, pairs, image=True, **options):
    """The algorithmic bytes of the Farneback stage (relax_profile_read kind 6) of `pairs` pairs, in closed form over route(): every kernel's
    inputs read once and outputs written once.  Per pixel of a frame: 3 bytes read and 4 written for the gray plane, or, under pyramid_fused,
    the four level inputs written with it (4 x (1 + 1/4 + 1/16 + 1/64)); per level and frame 4 HW read and 4 hw written by the blur (+ the
    full-size blur written and read again, 8 HW, where a resize follows it), and 24 hw of poly_expansion (4 in, 5 coefficients out); per level
    and pair 8 (coarser + this size) for resize_linear_f32<2>, and per iteration 56 hw (flow_iteration: 2 x 5 floats of R twice, the flow in
    and out) or 68 + 28 hw (update_matrices_k with M written, then the solve: M read, flow written); 11 HW for the image (flow read, 3 written)."""
    r = route(params, H, W, **options)
    HW = H * W
    total = 2 * pairs * HW * ((3 + 4 * (1 + 1 / 4 + 1 / 16 + 1 / 64)) if r[0]["pyramid"] == "fused" else 7)
    for i, lv in enumerate(r):
        hw = lv["h"] * lv["w"]
        if lv["up"] == "resize_linear_f32<2>":
            total += 8 * pairs * (r[i - 1]["h"] * r[i - 1]["w"] + hw)
        if lv["pyramid"] != "fused":
            total += 2 * pairs * (4 * HW + 4 * hw + (8 * HW if lv["k"] >= 1 and lv["pyramid"] != "sampled" else 0))
        total += 2 * pairs * hw * 24
        total += params["iterations"] * pairs * hw * (56 if lv["iteration"] == "flow_iteration" else 68 + 28)
    return total + (11 * pairs * HW if image else 0)


def group_route(group, **options):
    return route(group["params"], group["H"], group["W"], **options)


def used_levels(group):
    return len(plan(group["H"], group["W"], group["params"]["pyr_scale"], group["params"]["levels"])) - 1


def route_word(group):
    """One line for the record: the level sizes and the distinct launches of the group's route."""
    r = group_route(group)
    pyramid = "+".join(sorted({lv["pyramid"] for lv in r}))
    up = "+".join(sorted({lv["up"] for lv in r if lv["up"]})) or "none"
    sizes = " ".join(f"{lv['h']}x{lv['w']}" for lv in r)
    return f"pyramid {pyramid}; up {up}; poly_expansion<{r[0]['poly']}>; {r[0]['iteration']}; levels {sizes}; seg {r[-1]['seg']} x {r[-1]['bands']} bands"


# ---- the four binary factors and the neighbours of a parameter -------------------------------------------------------------------------
def factors(params):
    return (params["pyr_scale"] == 0.5, params["winsize"] == 15, params["poly_n"], params["iterations"] == 1)


def winsize_class(winsize):
    return "15" if winsize == 15 else ("under" if winsize < 15 else "over")


def dead_parameters(group):
    """The parameters whose value cannot show in the group's result, by construction: `levels` and pyr_scale where the 32-pixel stop leaves no level, and
    poly_n where poly_sigma is under 1.5 - the taps 6 and 7 from the centre of the separable Gaussian carry exp(-18 / sigma^2) of its weight,
    under 4e-6 at 1.2 (flow_param_cases.py's poly7 set has sigma 1.5 for that reason).  A case does not count for the coverage of a parameter that is dead in it."""
    return ({"levels", "pyr_scale"} if used_levels(group) == 0 else set()) | ({"poly_n"} if group["params"]["poly_sigma"] < 1.5 else set())


def neighbours(group):
    """{parameter: the group's parameters with that one replaced by a neighbour inside the accepted range}: winsize +- 2, poly_n 5 <-> 7,
    iterations +- 1, pyr_scale +- 0.05, one used level fewer, poly_sigma +- 0.1 (the upper neighbour where there is one).  No entry for
    `levels` where no level is used."""
    p = group["params"]
    out = {
        "winsize": {**p, "winsize": p["winsize"] + 2 if p["winsize"] < 63 else 61},
        "poly_n": {**p, "poly_n": 12 - p["poly_n"]},
        "iterations": {**p, "iterations": p["iterations"] + 1 if p["iterations"] < 10 else 9},
        "pyr_scale": {**p, "pyr_scale": round(p["pyr_scale"] + 0.05, 2) if p["pyr_scale"] < 0.95 else 0.9},
        "poly_sigma": {**p, "poly_sigma": round(p["poly_sigma"] + 0.1, 2)},
    }
    if used_levels(group) > 0:
        out["levels"] = {**p, "levels": used_levels(group) - 1}
    return out


def live_case(gid):
    """The case of a group on which a wrong parameter is looked for: the noisy texture where the group has it gated - on the smooth one a wide
    window converges to the same flow from one level fewer."""
    gated = [c for c in BY_ID[gid]["contents"] if (gid, c) not in BITS_ONLY]
    return (gid, "second" if "second" in gated else gated[0])
