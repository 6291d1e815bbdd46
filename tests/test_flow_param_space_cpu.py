"""The table of tests/flow_param_space.py is what it claims, without a GPU: which launches of flow_chunk its cases reach (counted on the
restated dispatch, flow_param_space.route), relax_flow_plan against the oracle's pyramid arithmetic on every case, the input conditions of
the parity gate of tests/test_gpu_flow_param_space.py from the two oracles alone, and every parameter live where its coverage is counted:
the oracle with a neighbouring value lies far outside the gate."""
import collections
import itertools
import math

import numpy as np
import pytest

import relax_vqa_amd  # noqa: F401
from oracle import flow_ref
from tests import flow_cases as fc
from tests import flow_param_cases as pc
from tests import flow_param_space as sp

UNIT_FLOOR = 1e-7      # mean |fp32 oracle - fp64 oracle|: under it the unit of the parity ratio is rounding of the oracle's last steps alone
MIN_FLOW = 1.0         # px
GATED = [c for c in sp.CASES if c not in sp.BITS_ONLY]


def _groups_of(cases):
    return [sp.BY_ID[c[0]] for c in cases]


# ---- the table's shape ---------------------------------------------------------------------------------------------------------------
def test_the_table_is_fixed_small_and_inside_the_accepted_ranges():
    assert 60 <= len(sp.CASES) <= 90 and len(set(sp.CASES)) == len(sp.CASES) and len(set(sp.GROUP_IDS)) == len(sp.GROUPS)
    again = sp._build()
    assert [g["id"] for g in again] == sp.GROUP_IDS and [g["contents"] for g in again] == [g["contents"] for g in sp.GROUPS]
    fused_pyramids = 0
    for g in sp.GROUPS:
        p, H, W = g["params"], g["H"], g["W"]
        assert set(p) == set(pc.KEYS) and p["pyr_scale"] in sp.PYR_SCALES and p["levels"] in sp.LEVELS and p["iterations"] in sp.ITERATIONS
        assert p["poly_n"] in sp.POLY_NS and p["poly_sigma"] in sp.POLY_SIGMAS and (p["winsize"] in sp.WINSIZES or p["winsize"] == 3)
        assert 1 <= len(g["contents"]) <= 3 and set(g["contents"]) <= set(sp.CONTENTS) and len(set(g["contents"])) == len(g["contents"])
        oc, pb, win = sp.box_band(p["winsize"]), sp.POLY_BAND[p["poly_n"]], p["winsize"]
        fused_pyramid = sp.group_route(g)[0]["pyramid"] == "fused"
        fused_pyramids += fused_pyramid
        if fused_pyramid:      # the smallest frame pyramid_fused takes
            assert (H, W) == (256, 264) and win != 15
            continue
        assert H <= 256 and W in (oc - 1, oc, oc + 1, 2 * oc + 1, pb - 1, pb, pb + 1), g["id"]
        # a height class of the window, or the smallest height at which the levels the group uses are used
        used = sp.used_levels(g)
        assert H in sp.height_classes(win).values() or (used > 0 and H == sp.min_side(p["pyr_scale"], used)), g["id"]
    assert 2 <= fused_pyramids <= 4
    assert sum(g["params"]["winsize"] == 3 for g in sp.GROUPS) == 1


def test_no_case_needs_the_wide_pyramid_kernels():
    for g in sp.GROUPS:
        sp.group_route(g)      # raises where a level would take the 39- or 79-tap instantiations (flow_param_cases.py's deep4 / deep5)
        assert all(lv[2] <= 19 for lv in sp.plan(g["H"], g["W"], g["params"]["pyr_scale"], g["params"]["levels"])), g["id"]


def test_the_restated_dispatch_on_the_sets_whose_routes_are_documented():
    """flow_param_cases.SETS says in words what each set runs; route() must say the same."""
    lit = sp.route(pc.LITERAL, 256, 264)
    assert [lv["pyramid"] for lv in lit] == ["fused"] * 4 and [(lv["h"], lv["w"]) for lv in lit] == [(32, 33), (64, 66), (128, 132), (256, 264)]
    assert [lv["up"] for lv in lit] == [None, "fused_x2", "fused_x2", "fused_x2"] and {lv["iteration"] for lv in lit} == {"flow_iteration"}
    assert lit[-1]["bands"] == 2 and lit[-1]["seg"] == 30 and lit[-1]["segments"] == 9
    assert {lv["iteration"] for lv in sp.route(pc.LITERAL, 256, 264, fused=False)} == {"update_matrices_k+box_solve_fused"}
    assert [lv["pyramid"] for lv in sp.route(pc.LITERAL, 256, 264, pyramid_fused=False)] == ["sampled", "sampled", "gauss3_v4", "gauss3_v4"]
    small = sp.route(pc.LITERAL, 97, 131)
    assert [lv["pyramid"] for lv in small] == ["gauss_pass", "gauss_pass"] and small[-1]["seg"] == 30
    s08 = sp.route(pc.SETS["scale08"][0], 97, 131)
    assert len(s08) == 5 and s08[0]["pyramid"] == "sampled" and s08[0]["ratio"] != round(s08[0]["ratio"])
    assert [lv["up"] for lv in s08] == [None] + ["resize_linear_f32<2>"] * 4
    w33 = sp.route(pc.SETS["win33"][0], 256, 264)
    assert len(w33) == 1 and w33[0]["bands"] == 2 and w33[0]["iteration"] == "update_matrices_k+box_solve_any" and sp.box_band(33) == 224
    assert [sp.box_band(w) for w in (9, 33, 63, 15)] == [248, 224, 192, 240]
    assert sp.route(pc.SETS["poly7"][0], 256, 264)[-1]["poly_bands"] == 2 and sp.route(pc.LITERAL, 97, 246)[-1]["poly_bands"] == 1


def test_segment_rows_restates_flow_segment_rows():
    """A multiple of the window: 18, 9, 6, 4 or 3 windows where that still gives 16 blocks, else 2."""
    assert sp.segment_rows(8, 2160, 15) == 270 and sp.segment_rows(2, 1080, 15) == 135 and sp.segment_rows(3, 540, 15) == 90
    assert sp.segment_rows(2, 256, 15) == 30      # 2 bands x 6 segments of 45 rows: still under 16 blocks
    assert sp.segment_rows(1, 128, 15) == 30 and sp.segment_rows(2, 264, 5) == 30 and sp.segment_rows(1, 16, 63) == 126


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_every_combination_of_the_four_binary_factors_occurs_twice_on_a_pyramid():
    seen = collections.Counter(sp.factors(g["params"]) for g in _groups_of(GATED) if sp.used_levels(g) >= 1 and not sp.dead_parameters(g))
    for combo in itertools.product((True, False), (True, False), sp.POLY_NS, (True, False)):
        assert seen[combo] >= 2, (combo, seen[combo])


def test_every_value_of_every_axis_occurs():
    for key, values in [("pyr_scale", sp.PYR_SCALES), ("winsize", sp.WINSIZES + (3,)), ("iterations", sp.ITERATIONS), ("poly_n", sp.POLY_NS),
                        ("poly_sigma", sp.POLY_SIGMAS)]:
        assert {g["params"][key] for g in sp.GROUPS} == set(values), key
    # `levels` counts where it is live: the 32-pixel stop does not cut it (a cut value asks for the same pyramid as a smaller one)
    assert {g["params"]["levels"] for g in sp.GROUPS if sp.used_levels(g) == g["params"]["levels"]} == set(sp.LEVELS)
    assert {g["params"]["levels"] for g in sp.GROUPS} == set(sp.LEVELS)


def test_every_pyr_scale_meets_a_window_under_at_and_over_15():
    seen = {(g["params"]["pyr_scale"], sp.winsize_class(g["params"]["winsize"])) for g in sp.GROUPS if g["params"]["winsize"] != 3}
    assert seen == set(itertools.product(sp.PYR_SCALES, ("under", "15", "over")))


def test_the_routes_no_other_test_runs_occur():
    routes = {g["id"]: sp.group_route(g) for g in sp.GROUPS}

    def count(pred):
        return sum(pred(g, routes[g["id"]]) for g in _groups_of(sp.CASES))
    any_ = "update_matrices_k+box_solve_any"
    assert count(lambda g, r: r[0]["pyramid"] == "fused" and r[0]["iteration"] == any_) >= 2
    assert count(lambda g, r: g["params"]["poly_n"] == 7 and r[0]["iteration"] == any_ and len(r) > 1) >= 2
    assert count(lambda g, r: r[-1]["up"] == "resize_linear_f32<2>" and r[0]["iteration"] == any_) >= 2
    assert count(lambda g, r: r[-1]["up"] == "resize_linear_f32<2>" and g["params"]["poly_n"] == 7) >= 2
    assert count(lambda g, r: r[-1]["up"] == "resize_linear_f32<2>" and r[0]["iteration"] == any_ and g["params"]["iterations"] == 1) >= 2
    assert count(lambda g, r: g["params"]["iterations"] == 10 and r[0]["iteration"] == any_) >= 2
    assert count(lambda g, r: g["params"]["iterations"] == 10 and r[0]["iteration"] == "flow_iteration") >= 2
    for ps in (0.6, 0.7, 0.8):      # a sampled level whose W / w is no integer
        assert count(lambda g, r: g["params"]["pyr_scale"] == ps and any(lv["pyramid"] == "sampled" and lv["ratio"] != round(lv["ratio"]) for lv in r)) >= 1, ps
    assert count(lambda g, r: len(r) - 1 >= 6) >= 3
    assert 2 * count(lambda g, r: len(r) - 1 >= 2) >= len(sp.CASES)
    assert count(lambda g, r: r[-1]["bands"] >= 3) >= 2 and count(lambda g, r: r[-1]["segments"] >= 2) >= 4


def test_every_band_edge_is_met_from_both_sides():
    kernels = {
        "box_solve_any": lambda p: p["winsize"] != 15 and p["winsize"] != 3 and sp.box_band(p["winsize"]),
        "box_solve_fused / flow_iteration": lambda p: p["winsize"] == 15 and sp.FUSED_BAND,
        "poly_expansion<5>": lambda p: p["poly_n"] == 5 and sp.POLY_BAND[5],
        "poly_expansion<7>": lambda p: p["poly_n"] == 7 and sp.POLY_BAND[7],
    }
    for name, band_of in kernels.items():
        offsets = {g["W"] - band_of(g["params"]) for g in sp.GROUPS if band_of(g["params"])}
        assert {-1, 0, 1} <= offsets, (name, sorted(offsets))
    # two bands and one column: the coarser level of a halving pyramid is one band wide to the column
    assert any(g["W"] == 2 * sp.box_band(g["params"]["winsize"]) + 1 and g["params"]["pyr_scale"] == 0.5 and sp.used_levels(g) >= 1
               and sp.group_route(g)[-2]["w"] == sp.box_band(g["params"]["winsize"]) for g in sp.GROUPS)


def test_every_height_class_occurs_under_and_over_the_literal_window():
    seen = set()
    for g in sp.GROUPS:
        win = g["params"]["winsize"]
        for name, h in sp.height_classes(win).items():
            if g["H"] == h and win not in (3, 15):
                seen.add((name, sp.winsize_class(win)))
    assert seen == set(itertools.product(sp.height_classes(9), ("under", "over"))), sorted(seen)
    assert sum(sp.BY_ID[c[0]]["H"] < sp.BY_ID[c[0]]["params"]["winsize"] for c in sp.CASES) >= 2


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_flow_plan_equals_the_oracle_on_every_group():
    for g in sp.GROUPS:
        p = g["params"]
        got, want = sp.plan(g["H"], g["W"], p["pyr_scale"], p["levels"]), pc.oracle_plan(g["H"], g["W"], p["pyr_scale"], p["levels"])
        assert [lv[:3] for lv in got] == [lv[:3] for lv in want], g["id"]
        assert all(math.isclose(a[3], b[3], rel_tol=1e-14, abs_tol=1e-15) for a, b in zip(got, want)), g["id"]
        assert len(got) - 1 == flow_ref.pyramid_levels(g["H"], g["W"], p["pyr_scale"], p["levels"])


# ---- input conditions, from the two oracles alone ----------------------------------------------------------------------------------------
def conditions(case):
    f64, f32 = sp.reference(case)
    d = np.abs(f32.astype(np.float64) - f64)
    return float(d.max()), float(d.mean()), float(np.abs(f64).max()), bool(np.isfinite(f64).all() and np.isfinite(f32).all())


@pytest.mark.parametrize("case", GATED, ids=[sp.case_id(c) for c in GATED])
def test_every_gated_case_is_well_posed_has_a_unit_and_moves(case):
    """Measured over the table: max |fp32 - fp64| 7.6e-7 .. 1.9e-4, mean 1.1e-7 .. 6.6e-6, max |flow| 1.03 .. 12.1 px."""
    d_max, d_mean, flow_max, finite = conditions(case)
    print(f"{sp.case_id(case)}: max |fp32 - fp64| {d_max:.2e}, mean {d_mean:.2e}, max |flow| {flow_max:.2f}")
    assert finite
    assert d_max < pc.WELL_POSED, d_max
    assert d_mean >= UNIT_FLOOR, d_mean
    assert flow_max >= MIN_FLOW, flow_max


def test_the_bits_only_group_is_small_and_each_member_misses_a_condition():
    assert len(sp.BITS_ONLY) <= sp.BITS_ONLY_SHARE * len(sp.CASES)
    assert set(sp.BITS_ONLY) <= set(sp.CASES)
    win3 = [c for c in sp.CASES if sp.BY_ID[c[0]]["params"]["winsize"] == 3]
    assert len(win3) == 1 and win3[0] in sp.BITS_ONLY
    for case, reason in sp.BITS_ONLY.items():
        assert isinstance(reason, str) and len(reason) > 20, case
        d_max, d_mean, flow_max, finite = conditions(case)
        assert finite and (d_max >= pc.WELL_POSED or d_mean < UNIT_FLOOR or flow_max < MIN_FLOW), (case, d_max, d_mean, flow_max)


# ---- every parameter is live where it is counted ----------------------------------------------------------------------------------------
FACTOR_KEYS = ("pyr_scale", "winsize", "poly_n", "iterations")


def _smallest(groups):
    return min(groups, key=lambda g: g["H"] * g["W"])


def live_groups():
    """{group id: the parameters that must be live in it}: for each of the sixteen factor combinations (on a pyramid) the four factors'
    parameters, for each limit value of an axis that parameter - on the smallest group that has the combination or the value."""
    gated_groups = [g for g in sp.GROUPS if any((g["id"], c) not in sp.BITS_ONLY for c in g["contents"])]
    picked = {}
    for combo in itertools.product((True, False), (True, False), sp.POLY_NS, (True, False)):
        g = _smallest([g for g in gated_groups if sp.factors(g["params"]) == combo and sp.used_levels(g) >= 1 and not sp.dead_parameters(g)])
        picked.setdefault(g["id"], set()).update(FACTOR_KEYS)
    for key, values in [("pyr_scale", sp.PYR_SCALES), ("levels", sp.LEVELS), ("winsize", sp.WINSIZES), ("iterations", sp.ITERATIONS),
                        ("poly_n", sp.POLY_NS), ("poly_sigma", sp.POLY_SIGMAS)]:
        for limit in (min(values), max(values)):
            if (key, limit) == ("levels", 0):
                continue      # (no level to take away: levels = 0 is live where levels = 1 differs from it, which the groups with levels = 1 show)
            g = _smallest([g for g in gated_groups if g["params"][key] == limit and key not in sp.dead_parameters(g)
                           and (key != "levels" or sp.used_levels(g) == limit)])
            picked.setdefault(g["id"], set()).add(key)
    return picked


LIVE = live_groups()


@pytest.mark.parametrize("gid", list(LIVE), ids=list(LIVE))
def test_every_parameter_is_live_where_it_is_counted(gid):
    """The float32 oracle with ONE parameter replaced by a neighbour lies more than 16 x PARITY_CAP float32-oracle distances from the
    float64 oracle with the right parameters (test_the_wrong_parameter_references_are_far_from_the_right_ones's rule): a kernel that took
    the neighbour's value would fail the GPU gate by a wide margin.  Measured: 984 (poly_n 5 for 7 at sigma 1.5, winsize 5) and up for the
    parameters that must be live; the others are printed (the one figure under the bound: 16, one level fewer than eight at pyr_scale 0.95
    under a 45-pixel window)."""
    g = sp.BY_ID[gid]
    case = sp.live_case(gid)
    f64, f32 = sp.reference(case)
    a, b = fc.make_pair(sp.pair_of(case))
    ga, gb = flow_ref.bgr2gray(a), flow_ref.bgr2gray(b)
    wrong_params = sp.neighbours(g)
    assert set(wrong_params) | sp.dead_parameters(g) >= set(pc.KEYS) and not LIVE[gid] & sp.dead_parameters(g)
    for key, wrong in wrong_params.items():
        if key in sp.dead_parameters(g):
            continue
        ratio = fc.parity_ratio(flow_ref.farneback(ga, gb, **wrong), f64, f32)
        print(f"{sp.case_id(case)} with {key}={wrong[key]:g}: ratio {ratio:.0f}" + (" (must be live)" if key in LIVE[gid] else ""))
        if key in LIVE[gid]:
            assert ratio > 16 * fc.PARITY_CAP, (gid, key, wrong[key], ratio)
