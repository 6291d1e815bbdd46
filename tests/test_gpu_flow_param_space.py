"""Farneback flow through relax_optical_flow_ex on the table of tests/flow_param_space.py: the six parameters in combination, at their
limits, at widths one column either side of every kernel's band and heights one row either side of a row segment.  One GPU call per
(parameters, H, W) group.  The flow against oracle/flow_ref.farneback with the same parameters in float64, in units of the float32 oracle's
own distance from it, under the gate tests/test_gpu_flow_params.py takes from profiles/flow_params_parity.json (these cases feed no gate);
the flow image against the oracle's and, bit for bit, against flow_to_rgb of the call's own flow; and every group bit-stable over runs,
chunks, forced row segmentations, the two iteration paths, the two pyramids, batches, and flow-only / image-only requests."""
import functools

import numpy as np
import pytest
import torch

from oracle import flow_ref
from tests import flow_cases as fc
from tests import flow_param_cases as pc
from tests import flow_param_space as sp
from tests.gpu_common import engine

pytestmark = pytest.mark.gpu

DEFAULTS = {"flow_fused": 1, "flow_seg_rows": 0, "flow_max_pairs": 0, "flow_pyramid_fused": 1}
CASE_IDS = [sp.case_id(c) for c in sp.CASES]


@functools.lru_cache(maxsize=None)
def frames_of(gid):
    """uint8 [pairs, 2, H, W, 3] on the host, made once per group; do not write into it"""
    return fc.frames_of(sp.batch_of(sp.BY_ID[gid]))


def run(gid, pairs=None, want_flow=True, want_image=True, **options):
    """One call through relax_optical_flow_ex on the group's pairs (or on the rows `pairs` of its batch) under the given options
    (restored afterwards)."""
    eng = engine()
    frames = torch.from_numpy(np.ascontiguousarray(frames_of(gid)[slice(None) if pairs is None else pairs])).cuda()
    try:
        for k, v in options.items():
            assert eng.get_option(k) == DEFAULTS[k], k
            eng.set_option(k, v)
        return eng.optical_flow_ex(frames, want_flow=want_flow, want_image=want_image, **sp.BY_ID[gid]["params"])
    finally:
        for k in options:
            eng.set_option(k, DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def batch_result(gid):
    """-> (flow, image) on the host of the group's batch: one GPU call, computed once"""
    flow, img = run(gid)
    return flow.cpu().numpy(), img.cpu().numpy()


def gpu_result(case):
    flow, img = batch_result(case[0])
    k = sp.BY_ID[case[0]]["contents"].index(case[1])
    return flow[k], img[k]


def measure():
    """{case id: dict(mean_ratio, max_ratio, route, used_levels)} of every case (tools/flow_param_space_parity.py records them)"""
    out = {}
    for case in sp.CASES:
        f64, f32 = sp.reference(case)
        mean_r, max_r = pc.parity_terms(gpu_result(case)[0], f64, f32)
        g = sp.BY_ID[case[0]]
        out[sp.case_id(case)] = {"mean_ratio": mean_r, "max_ratio": max_r, "bits_only": case in sp.BITS_ONLY, "used_levels": sp.used_levels(g),
                                 "route": sp.route_word(g)}
    return out


# ---- a. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sp.CASES, ids=CASE_IDS)
def test_flow_parity_per_case(case):
    f64, f32 = sp.reference(case)
    flow = gpu_result(case)[0]
    assert np.isfinite(flow).all()
    if sp.BY_ID[case[0]]["params"]["winsize"] == 3:
        return      # not well posed by design (flow_param_cases.py's win3): finite
    err = np.abs(flow - f64)
    mean_r, max_r = pc.parity_terms(flow, f64, f32)
    ratio, gate = fc.parity_ratio(flow, f64, f32), pc.parity_gate()
    print(f"{sp.case_id(case)}: mean ratio {mean_r:.3f}, max ratio {max_r:.3f} (gate {gate:g}); max |gpu - fp64| {err.max():.2e}, mean {err.mean():.2e}; "
          f"max |fp32 oracle - fp64| {np.abs(f32 - f64).max():.2e}")
    if case in sp.BITS_ONLY:
        assert err.max() < 2e-3 and err.mean() < 2e-5, (err.max(), err.mean())      # test_flow_on_small_and_odd_frames's bound
    else:
        assert ratio <= gate, (ratio, gate)


@pytest.mark.parametrize("case", sp.CASES, ids=CASE_IDS)
def test_flow_image_per_case(case):
    flow, img = gpu_result(case)
    if case not in sp.BITS_ONLY:
        want = flow_ref.flow_to_rgb(sp.reference(case)[1])
        d = np.abs(img.astype(np.int32) - want.astype(np.int32))
        print(f"{sp.case_id(case)}: equal {(d == 0).mean():.5f}, within 1 {(d <= 1).mean():.5f}")
        assert (d == 0).mean() > 0.995 and (d <= 1).mean() > 0.9995, ((d == 0).mean(), (d <= 1).mean())     # test_flow_image_per_case's thresholds


@pytest.mark.parametrize("gid", sp.GROUP_IDS)
def test_the_image_of_the_call_is_flow_to_rgb_of_its_flow(gid):
    """The magnitude range rides on the last launch of level 0 - another kernel on every route."""
    flow, img = batch_result(gid)
    again = engine().flow_to_rgb(torch.from_numpy(flow).cuda())
    assert np.array_equal(again.cpu().numpy(), img)


# ---- b. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", sp.GROUP_IDS)
def test_every_group_gives_the_same_bits_whatever_the_run_chunk_segmentation_path_pyramid_batch_and_request(gid):
    g = sp.BY_ID[gid]
    winsize, pairs = g["params"]["winsize"], len(g["contents"])
    flow, img = run(gid)
    assert bool(torch.isfinite(flow).all())
    base_f, base_i = batch_result(gid)
    assert np.array_equal(flow.cpu().numpy(), base_f) and np.array_equal(img.cpu().numpy(), base_i), "a second call"
    options = [{"flow_seg_rows": winsize}, {"flow_seg_rows": 4 * winsize}]
    if pairs > 1:
        options.append({"flow_max_pairs": 1})
    if winsize == 15:
        assert {lv["iteration"] for lv in sp.group_route(g)} == {"flow_iteration"}
        options.append({"flow_fused": 0})
    if sp.group_route(g)[0]["pyramid"] == "fused":
        options.append({"flow_pyramid_fused": 0})
    for opt in options:
        f, i = run(gid, **opt)
        assert torch.equal(f, flow), (opt, float((f - flow).abs().max()), float((f != flow).float().mean()))
        assert torch.equal(i, img), opt
    if pairs > 1:
        for k in range(pairs):          # a pair's result does not depend on its batch
            f, i = run(gid, pairs=slice(k, k + 1))
            assert torch.equal(f[0], flow[k]) and torch.equal(i[0], img[k]), g["contents"][k]
    f, none = run(gid, want_image=False)
    assert none is None and torch.equal(f, flow)
    none, i = run(gid, want_flow=False)
    assert none is None and torch.equal(i, img)


# ---- c. the gate sees the parameters on the new routes ------------------------------------------------------------------------------
def _first(pred):
    return next(g["id"] for g in sp.GROUPS if pred(g, sp.group_route(g)) and not sp.dead_parameters(g))


_ANY = "update_matrices_k+box_solve_any"
WRONG = {
    "pyramid_fused+box_solve_any": _first(lambda g, r: r[0]["pyramid"] == "fused" and r[0]["iteration"] == _ANY),
    "poly7+resize2+box_solve_any": _first(lambda g, r: g["params"]["poly_n"] == 7 and r[-1]["up"] == "resize_linear_f32<2>" and r[0]["iteration"] == _ANY),
    "resize2+box_solve_any-one-iteration": _first(lambda g, r: g["params"]["poly_n"] == 5 and g["params"]["iterations"] == 1
                                                  and r[-1]["up"] == "resize_linear_f32<2>" and r[0]["iteration"] == _ANY),
    "poly7+resize2+flow_iteration": _first(lambda g, r: g["params"]["poly_n"] == 7 and r[-1]["up"] == "resize_linear_f32<2>" and r[0]["iteration"] == "flow_iteration"),
}


@pytest.mark.parametrize("gid", list(WRONG.values()), ids=list(WRONG))
def test_a_reference_with_a_neighbouring_parameter_fails_the_gate_by_a_wide_margin(gid):
    """The GPU flow against the oracle with ONE of pyr_scale, winsize, iterations and poly_n replaced by its neighbour
    (flow_param_space.neighbours): the gate of test_flow_parity_per_case would see a kernel that took that value."""
    case = sp.live_case(gid)
    flow = gpu_result(case)[0]
    for key in ("pyr_scale", "winsize", "iterations", "poly_n"):
        f64, f32 = pc.reference(sp.neighbours(sp.BY_ID[gid])[key], sp.pair_of(case))
        ratio = fc.parity_ratio(flow, f64, f32)
        print(f"{sp.case_id(case)} against the oracle with {key}={sp.neighbours(sp.BY_ID[gid])[key][key]:g}: ratio {ratio:.0f}")
        assert ratio > 16 * fc.PARITY_CAP, (key, ratio)
