"""Optical flow on the GPU on large motion, hard edges, noise, saturated regions, a motion boundary and flows in every hue sector
(tests/flow_cases.py; tests/test_flow_cases_cpu.py holds what those inputs reach): the flow against the oracle in float64, in units of
the float32 oracle's own distance from it; the flow image against the oracle's; every kernel path and batching bit-equal on these inputs,
where the gathers of the fused iteration kernel go far from a pixel's own row band; and flow_to_rgb alone, exact, on a field that sits on
every boundary of its arithmetic."""
import functools

import numpy as np
import pytest
import torch

from oracle import flow_ref
from tests import flow_cases as fc
from tests.gpu_common import engine

pytestmark = pytest.mark.gpu

IDS = [fc.case_id(c) for c in fc.CASES]
BATCHES = {size: fc.batches(size) for size in fc.SIZES}
DEFAULTS = {"flow_fused": 1, "flow_pyramid_fused": 1, "flow_seg_rows": 0}


def run(cases, **options):
    """The engine's flow and flow image of the pairs of `cases` in ONE call, under the given options (restored afterwards)."""
    eng = engine()
    frames = torch.from_numpy(fc.frames_of(cases)).cuda()
    try:
        for k, v in options.items():
            assert eng.get_option(k) == DEFAULTS[k], k
            eng.set_option(k, v)
        return eng.optical_flow(frames, want_flow=True, want_image=True)
    finally:
        for k in options:
            eng.set_option(k, DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def batch_result(batch):
    """-> (flow [n,h,w,2] float32, image [n,h,w,3] uint8) on the host, one GPU call per batch, computed once"""
    flow, img = run(batch)
    return flow.cpu().numpy(), img.cpu().numpy()


def gpu_result(case):
    for batch in BATCHES[case[:2]]:
        if case in batch:
            flow, img = batch_result(tuple(batch))
            return flow[batch.index(case)], img[batch.index(case)]
    raise KeyError(case)


# ---- measurements (tools/flow_content_parity.py records them in profiles/flow_content_parity.json) -----------------------------
def measure_ratios():
    out = {}
    for case in fc.CASES:
        f64, f32 = fc.reference(case)
        out[fc.case_id(case)] = fc.parity_ratio(gpu_result(case)[0], f64, f32)
    return out


FIELDS = {
    "128x264x1": lambda: fc.boundary_field(1, 128, 264),         # HW a multiple of 4: flow_visualise_v4
    "35x49x2": lambda: fc.boundary_field(2, 35, 49),             # odd pixel count: flow_visualise, the second pair off every 16-byte line
    "35x49x1-constant-magnitude": lambda: fc.constant_magnitude_field(35, 49),
}


def measure_field(name):
    """-> (explained pixels, unexplained pixels [(pair, y, x)], the GPU's image)"""
    field = FIELDS[name]()
    got = engine().flow_to_rgb(torch.from_numpy(field).cuda()).cpu().numpy()
    explained, unexplained = 0, []
    for p in range(len(field)):
        e, u = fc.unexplained_pixels(got[p], field[p])
        explained += e
        unexplained += [(p,) + yx for yx in u]
    return explained, unexplained, got


# ---- a. the flow -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=IDS)
def test_flow_parity_per_case(case):
    f64, f32 = fc.reference(case)
    flow = gpu_result(case)[0]
    assert np.isfinite(flow).all()
    ratio, gate = fc.parity_ratio(flow, f64, f32), fc.parity_gate()
    print(f"{fc.case_id(case)}: ratio {ratio:.3f} (gate {gate:g}); max |gpu - fp64| {np.abs(flow - f64).max():.2e}, "
          f"max |fp32 oracle - fp64| {np.abs(f32 - f64).max():.2e}")
    assert ratio <= gate, (ratio, gate)


# ---- b. the flow image ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES, ids=IDS)
def test_flow_image_per_case(case):
    want = flow_ref.flow_to_rgb(fc.reference(case)[1])
    d = np.abs(gpu_result(case)[1].astype(np.int32) - want.astype(np.int32))
    print(f"{fc.case_id(case)}: equal {(d == 0).mean():.5f}, within 1 {(d <= 1).mean():.5f}")
    assert (d == 0).mean() > 0.995 and (d <= 1).mean() > 0.9995, ((d == 0).mean(), (d <= 1).mean())     # test_flow_matches_oracle's thresholds


# ---- c. the paths agree on these inputs ----------------------------------------------------------------------------------------
PATHS = [{"flow_fused": 0}, {"flow_pyramid_fused": 0}, {"flow_seg_rows": 30}, {"flow_seg_rows": 135}]


def _assert_same(batch, options):
    flow, img = run(batch)
    assert bool(torch.isfinite(flow).all())
    for opt in options:
        f, i = run(batch, **opt)
        assert torch.equal(f, flow), (opt, float((f - flow).abs().max()), float((f != flow).float().mean()))
        assert torch.equal(i, img), opt
    for k, case in enumerate(batch):          # a pair's result does not depend on its batch
        f, i = run([case])
        assert torch.equal(f[0], flow[k]) and torch.equal(i[0], img[k]), fc.case_id(case)


@pytest.mark.parametrize("k", range(len(BATCHES[(256, 264)])))
def test_every_path_gives_the_same_bits_at_256x264(k):
    """flow_iteration against update_matrices_k + box_solve_fused, pyramid_fused against the per-level kernels, three row segmentations,
    and each pair alone: flow and image identical bit for bit."""
    _assert_same(BATCHES[(256, 264)][k], PATHS)


def test_both_iteration_paths_give_the_same_bits_at_97x131():
    """Odd pixel count: the second and third pair's coefficient blocks start off a 16-byte line."""
    _assert_same(BATCHES[(97, 131)][1], [{"flow_fused": 0}])


# ---- d. flow_to_rgb alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["128x264x1", "35x49x2"])
def test_flow_to_rgb_is_exact_or_explained_on_the_boundary_field(name):
    explained, unexplained, got = measure_field(name)
    print(f"{name}: {explained} of {got[..., 0].size} pixels differ from the oracle's and are explained, {len(unexplained)} are not")
    assert not unexplained, unexplained[:10]


def test_flow_to_rgb_of_a_constant_magnitude_is_black():
    explained, unexplained, got = measure_field("35x49x1-constant-magnitude")
    assert int(got.max()) == 0 and explained == 0 and not unexplained      # empty range: cv2.normalize's scale is 0


# ---- e. no correspondence at all -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", fc.SIZES, ids=["97x131", "256x264"])
def test_entirely_new_content_in_a_batch_of_ordinary_pairs(size):
    """The second frame shares nothing with the first: the flow is wild (60 to 100 px) but finite, equal to the pair's flow alone, and -
    where the float32 oracle agrees with its float64 form on it - as close to the oracle as every other case."""
    case = fc.DEGENERATE[size]
    batch = [BATCHES[size][0][1], case, BATCHES[size][1][0]]
    flow, img = run(batch)
    assert bool(torch.isfinite(flow).all())
    alone, alone_img = run([case])
    assert torch.equal(alone[0], flow[1]) and torch.equal(alone_img[0], img[1])
    for k in (0, 2):
        assert np.array_equal(flow[k].cpu().numpy(), gpu_result(batch[k])[0])
    f64, f32 = fc.reference(case)
    well_posed = float(np.abs(f32 - f64).max()) < 1e-3
    ratio = fc.parity_ratio(flow[1].cpu().numpy(), f64, f32)
    print(f"{fc.case_id(case)}: max |flow| {float(flow[1].abs().max()):.1f}, well-posed {well_posed}, ratio {ratio:.3f}")
    if well_posed:
        assert ratio <= fc.parity_gate(), ratio
