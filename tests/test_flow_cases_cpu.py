"""The inputs of tests/test_gpu_flow_content.py do what they claim (tests/flow_cases.py), checked with the oracle on the CPU: these are
conditions on the listed cases, not measurements - a case that misses one gets another seed or leaves the list."""
import numpy as np
import pytest

from oracle import flow_ref
from tests import flow_cases as fc

IDS = [fc.case_id(c) for c in fc.CASES]


def test_the_list_covers_every_kind_and_motion_at_both_sizes():
    assert 20 <= len(fc.CASES) <= 24 and len(set(fc.CASES)) == len(fc.CASES)
    motions = fc.SHIFTS + fc.ROTZOOMS + [fc.OCCLUSION]
    for size in fc.SIZES:
        cs = [c for c in fc.CASES if c[:2] == size]
        assert {c[2] for c in cs} == set(fc.KINDS), size
        assert {c[3] for c in cs} == set(motions), size
        for batch in fc.batches(size):
            assert 2 <= len(batch) <= 3 and len({c[3] for c in batch}) == len(batch), batch      # different motions in one call


@pytest.mark.parametrize("case", fc.CASES, ids=IDS)
def test_case_meets_its_conditions(case):
    h, w, kind, motion, _ = case
    a, b = fc.make_pair(case)
    assert a.shape == b.shape == (h, w, 3) and a.dtype == b.dtype == np.uint8
    cov = fc.coverage(case)
    print(fc.case_id(case), cov)
    assert cov["levels"] == {(97, 131): 2, (256, 264): 4}[(h, w)]
    if motion[0] == "shift":
        assert cov["max_flow"] >= 8.0, cov                       # displacement
        assert cov["interior_out_of_frame"] >= 0.01, cov         # the out-of-frame branch at full weight, outside the border band
    if motion[0] == "rotzoom":
        assert min(cov["hue_sectors"]) >= 0.05, cov              # every branch of the HSV -> BGR sector table
    if kind == "sat":
        assert (a == 0).mean() > 0.05 and (a == 255).mean() > 0.05, ((a == 0).mean(), (a == 255).mean())     # flat clipped regions
    if kind == "steps":
        assert set(np.unique(a).tolist()) == {0, 255}
    # well-posed: the float32 oracle agrees with its float64 form (no in-frame test that flips between the two precisions)
    f64, f32 = fc.reference(case)
    assert f64.dtype == np.float64 and f32.dtype == np.float32
    d = float(np.abs(f32 - f64).max())
    assert d < 1e-3, d


def test_shift_brings_new_content_in_and_is_no_wrap_around():
    h, w = 97, 131
    a, b = fc.make_pair((h, w, "noise", fc.SHIFTS[0], 6))
    assert np.array_equal(b[:h - 6, 9:], a[6:, :w - 9])          # the content moved by (+9, -6)
    assert not np.array_equal(b[:h - 6, :9], a[6:, w - 9:])      # what np.roll would have brought in


def test_default_dtype_and_hook_leave_the_oracle_as_it_was():
    """farneback's default is float32 through its own update_matrices; the copy the wrong variants are made from is that function, bit
    for bit, in both precisions."""
    a, b = fc.make_pair(fc.CASES[1])
    ga, gb = flow_ref.bgr2gray(a), flow_ref.bgr2gray(b)
    for dtype in (np.float32, np.float64):
        want = flow_ref.farneback(ga, gb, dtype=dtype)
        assert want.dtype == dtype
        assert np.array_equal(want, flow_ref.farneback(ga, gb, dtype=dtype, update_matrices=fc.wrong_update_matrices(None)))
    assert np.array_equal(fc.reference(fc.CASES[1])[1], flow_ref.farneback(ga, gb))


@pytest.mark.parametrize("bug", fc.WRONG)
def test_listed_cases_expose_a_wrong_matrix_update(bug):
    """Each of the six mistakes moves the float32 flow by at least a pixel on some listed case (the 1- to 3-pixel inputs of the other
    flow tests: at most 0.14 px, one of them under the 1e-3 gate)."""
    worst = 0.0
    for case in [c for c in fc.CASES if c[3][0] == "shift"]:
        a, b = fc.make_pair(case)
        got = flow_ref.farneback(flow_ref.bgr2gray(a), flow_ref.bgr2gray(b), update_matrices=fc.wrong_update_matrices(bug))
        worst = max(worst, float(np.abs(got - fc.reference(case)[1]).max()))
        if worst >= 1.0:
            break
    print(bug, worst)
    assert worst >= 1.0, (bug, worst)


def test_existing_inputs_never_leave_the_frame_outside_the_border_band():
    """Why this file exists: tests/test_gpu_flow.py's own pair takes the out-of-frame branch only inside the 5-pixel border band."""
    from tests.test_gpu_flow import _smooth_pair
    a, b = _smooth_pair(200, 264, 1)
    flow = flow_ref.farneback(flow_ref.bgr2gray(a), flow_ref.bgr2gray(b))
    assert fc.interior_out_of_frame_share(flow) == 0.0
    assert float(np.abs(flow).max()) < 8.0


def test_boundary_field_holds_what_it_claims():
    v = fc.boundary_vectors()
    assert len(v) == 4096 * 8 + 13 * 8 + 4
    full = fc.boundary_field(1, 128, 264)
    assert full.shape == (1, 128, 264, 2) and np.array_equal(full.reshape(-1, 2)[:len(v)], v)
    small = fc.boundary_field(2, 35, 49)
    assert small.shape == (2, 35, 49, 2) and not np.array_equal(small[0], small[1])
    for p in range(2):
        mags = np.hypot(small[p, ..., 0].astype(np.float64), small[p, ..., 1]).ravel()
        for m in fc.MAGNITUDES.tolist():
            assert (np.abs(mags - m) < 1e-4 * m).sum() > 100       # every magnitude on the ring survives the subsampling
    hue, _, _ = fc.visualisation_parts(full[0])
    assert hue.max() >= 179.0 and np.signbit(full[..., 0]).any() and (full == 0).all(axis=-1).any()
    sectors = np.floor(np.uint8(hue).astype(np.float32) * np.float32(6.0 / 180.0)).astype(int)
    assert set(np.unique(sectors).tolist()) >= {0, 1, 2, 3, 4, 5}
    c = fc.constant_magnitude_field(35, 49)[0]
    assert len(np.unique(np.sqrt(c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]))) == 1
    assert int(flow_ref.flow_to_rgb(c).max()) == 0               # empty range: scale 0, black


def test_the_explanation_rule_accepts_the_oracle_and_refuses_a_wrong_pixel():
    flow = fc.boundary_field(1, 128, 264)[0]
    hue, val, want = fc.visualisation_parts(flow)
    assert np.array_equal(flow_ref.hsv_to_bgr_u8(np.stack([np.uint8(hue), np.full(hue.shape, 255, np.uint8), np.uint8(val)], -1)), want)
    assert fc.unexplained_pixels(want, flow) == (0, [])
    near = (np.abs(hue - np.rint(hue)) <= fc.NEAR) | (np.abs(val - np.rint(val)) <= fc.NEAR)
    n = len(fc.boundary_vectors())
    assert near.ravel()[n - 4096 * 8:n].mean() < 0.01            # on the ring (the axis vectors and the zero padding are integers by design)
    wrong = want.copy()
    y, x = np.argwhere(~near & (want.max(axis=-1) > 40))[0]
    wrong[y, x] = wrong[y, x][::-1] if wrong[y, x, 0] != wrong[y, x, 2] else wrong[y, x] // 2
    assert fc.unexplained_pixels(wrong, flow) == (0, [(int(y), int(x))])
