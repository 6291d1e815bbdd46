"""The Gaussian window (flags 256) and the initial flow (flags 4) of relax_optical_flow_flags on the GPU (csrc/flow.hip: gauss_solve_any,
resize_area_f32x2; RelaxEngine.optical_flow(..., extended=True)), on the table of tests/flow_flag_cases.py: the flow against
tests/flow_flag_ref.farneback_flags in float64 in units of the float32 reference's own distance (gate from profiles/flow_flags_parity.json);
a reference of the other mode far outside the gate; relax_flow_initial_level against the float64 area resize; flags 0 bit-equal to
relax_optical_flow_ex; every set bit-stable over runs, batches, chunks and forced segmentations; in place against out of place; the edges of
gauss_solve_any's tile; and the flow_params keyword of the clip methods.  Both modes are pinned to the stated formulas, not to an OpenCV build."""
import functools

import numpy as np
import pytest
import torch

from tests import flow_cases as fc
from tests import flow_flag_cases as gc
from tests import flow_flag_ref as fr
from tests import flow_param_cases as pc
from tests.gpu_common import engine, rn50_weights, vit_weights

pytestmark = pytest.mark.gpu

DEFAULTS = {"flow_fused": 1, "flow_seg_rows": 0, "flow_max_pairs": 0}
SET_SIZES = gc.set_sizes()
SET_SIZE_IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in SET_SIZES]
GATED = gc.gated_cases()
EDGES = gc.edge_cases()


def run_params(params, cases, init=None, want_image=True, **options):
    """Flow and flow image of the pairs of `cases` in ONE call through relax_optical_flow_flags, under the given options (restored afterwards)."""
    eng = engine()
    frames = torch.from_numpy(fc.frames_of(cases)).cuda()
    try:
        for k, v in options.items():
            assert eng.get_option(k) == DEFAULTS[k], k
            eng.set_option(k, v)
        return eng.optical_flow_flags(frames, want_flow=True, want_image=want_image, initial_flow=None if init is None else torch.from_numpy(init).cuda(),
                                      **params)
    finally:
        for k in options:
            eng.set_option(k, DEFAULTS[k])


def run(name, cases, **options):
    return run_params(gc.SETS[name][0], cases, gc.initial_fields(name, cases), **options)


@functools.lru_cache(maxsize=None)
def batch_result(name, size):
    """-> (flow, image) on the host of the set's batch of three at a size: one GPU call, computed once"""
    flow, img = run(name, gc.batch_of(name, size))
    return flow.cpu().numpy(), img.cpu().numpy()


def gpu_result(name, case):
    batch = gc.batch_of(name, case[:2])
    flow, img = batch_result(name, case[:2])
    return flow[batch.index(case)], img[batch.index(case)]


@functools.lru_cache(maxsize=None)
def edge_result(ws, h, w):
    flow, _ = run_params(gc.edge_params(ws), [pc.pair_case((h, w), gc.SECOND)], want_image=False)
    return flow[0].cpu().numpy()


def measure_ratios():
    """{case id: the gated figure} of every gated case and every edge case (tools/flow_flags_parity.py records them)"""
    out = {}
    for item in GATED:
        name, case, kind = item
        f64, f32 = gc.reference(name, case)
        out[gc.gated_id(item)] = gc.case_ratio(kind, gpu_result(name, case)[0], f64, f32)
    for ws, h, w in EDGES:
        f64, f32 = gc.edge_reference(ws, h, w)
        out[f"edge-win{ws}-{h}x{w}"] = fc.parity_ratio(edge_result(ws, h, w), f64, f32)
    return out


# ---- a. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", GATED, ids=[gc.gated_id(i) for i in GATED])
def test_flow_parity_per_case(item):
    name, case, kind = item
    f64, f32 = gc.reference(name, case)
    flow = gpu_result(name, case)[0]
    assert np.isfinite(flow).all()
    mean_r, max_r = pc.parity_terms(flow, f64, f32)
    ratio, gate = gc.case_ratio(kind, flow, f64, f32), gc.parity_gate()
    print(f"{gc.gated_id(item)}: mean ratio {mean_r:.3f}, max ratio {max_r:.3f}, gated figure {ratio:.3f} (gate {gate:g}); "
          f"max |gpu - fp64| {np.abs(flow - f64).max():.2e}, max |fp32 reference - fp64| {np.abs(f32 - f64).max():.2e}")
    assert ratio <= gate, (ratio, gate)


@pytest.mark.parametrize("ws,h,w", EDGES, ids=[f"win{ws}-{h}x{w}" for ws, h, w in EDGES])
def test_the_edges_of_the_gaussian_tile(ws, h, w):
    """Widths one column either side of the 64-column tile and 2 x 64 + 1, heights 2 winsize +- 1 and 16 (shorter than the window): bit-stable
    and within the gate, on the noise pair."""
    f64, f32 = gc.edge_reference(ws, h, w)
    flow = edge_result(ws, h, w)
    assert np.isfinite(flow).all()
    ratio, gate = fc.parity_ratio(flow, f64, f32), gc.parity_gate()
    print(f"win{ws} {h}x{w}: ratio {ratio:.3f} (gate {gate:g})")
    assert ratio <= gate, (ratio, gate)
    cases = [pc.pair_case((h, w), gc.SECOND), pc.pair_case((h, w), gc.SMOOTH)]
    both, _ = run_params(gc.edge_params(ws), cases, want_image=False)
    assert np.array_equal(both[0].cpu().numpy(), flow), "alone against in a batch"
    again, _ = run_params(gc.edge_params(ws), cases, want_image=False, flow_max_pairs=1)
    assert torch.equal(again, both)


# ---- b. the gate sees the mode ---------------------------------------------------------------------------------------------------
def test_the_box_reference_fails_the_gate_of_the_gaussian_result_by_a_wide_margin():
    case = pc.pair_case(gc.SMALL, gc.SMOOTH)
    b64, b32 = gc.reference("gauss33", case, flags=0)
    ratio = fc.parity_ratio(gpu_result("gauss33", case)[0], b64, b32)
    print(f"gauss33 against the box reference: ratio {ratio:.1f}")
    assert ratio > 16 * fc.PARITY_CAP, ratio


@pytest.mark.parametrize("name", ["init_lit", "init_l0"])
def test_the_reference_without_the_initial_flow_fails_the_gate_by_a_wide_margin(name):
    case = pc.pair_case(gc.SMALL, gc.SECOND)
    z64, z32 = gc.reference(name, case, flags=0)
    ratio = fc.parity_ratio(gpu_result(name, case)[0], z64, z32)
    print(f"{name} against the reference without the initial flow: ratio {ratio:.1f}")
    assert ratio > 16 * fc.PARITY_CAP, ratio


# ---- c. relax_flow_initial_level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,pyr_scale,levels,want_hw", [(gc.SMALL, 0.5, 3, (48, 66)), (gc.LARGE, 0.5, 3, (32, 33)), (gc.SMALL, 0.8, 4, None),
                                                           (gc.SMALL, 0.5, 0, (97, 131))],
                         ids=["97x131-to-48x66", "256x264-to-32x33", "97x131-at-0.8^4", "levels0-copy"])
def test_initial_level_against_the_float64_area_resize(size, pyr_scale, levels, want_hw):
    """Every element within 4 x 2^-24 x max |init|: double accumulation, one rounding to float, one multiply by (float)scale."""
    cases = gc.batch_of("init_lit", size)
    init = np.stack([gc.initial_field("init_s08", c) for c in cases])           # the strongest field: +- 3 px around (25, -20)
    init[0, 0, 0, 0] = -0.0
    got = engine().flow_initial_level(torch.from_numpy(init).cuda(), pyr_scale, levels).cpu().numpy()
    want = np.stack([fr.initial_level(f, pyr_scale, levels, np.float64) for f in init])
    assert got.shape == want.shape and (want_hw is None or got.shape[1:3] == want_hw), got.shape
    err = np.abs(got - want).max()
    print(f"{size} {pyr_scale}^{levels} -> {got.shape[1:3]}: max err {err:.3e}, bound {4 * 2.0 ** -24 * np.abs(init).max():.3e}")
    assert err <= 4 * 2.0 ** -24 * np.abs(init).max()
    if levels == 0:
        assert np.array_equal(got.view(np.uint32), init.view(np.uint32))


# ---- d. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["literal", "win33", "scale08"])
def test_flags_zero_through_the_new_entry_is_the_ex_entry_bit_for_bit(name):
    eng = engine()
    params, sizes = pc.SETS[name]
    frames = torch.from_numpy(fc.frames_of(pc.batch_of(name, sizes[0]))).cuda()
    old_f, old_i = eng.optical_flow_ex(frames, want_flow=True, want_image=True, **params)
    new_f, new_i = eng.optical_flow_flags(frames, want_flow=True, want_image=True, **params, flags=0)
    assert torch.equal(new_f, old_f) and torch.equal(new_i, old_i)
    kw_f, kw_i = eng.optical_flow(frames, want_flow=True, want_image=True, **params, extended=True)
    assert torch.equal(kw_f, old_f) and torch.equal(kw_i, old_i)


@pytest.mark.parametrize("name,size", SET_SIZES, ids=SET_SIZE_IDS)
def test_every_set_gives_the_same_bits_whatever_the_run_batch_chunk_and_segmentation(name, size):
    """(gauss_solve_any keeps no running sums: flow_seg_rows changes nothing in it by construction; the init_* sets with the box window run the
    kernels that honour it)"""
    batch = gc.batch_of(name, size)
    winsize = gc.SETS[name][0]["winsize"]
    flow, img = run(name, batch)
    assert bool(torch.isfinite(flow).all())
    assert np.array_equal(flow.cpu().numpy(), batch_result(name, size)[0]) and np.array_equal(img.cpu().numpy(), batch_result(name, size)[1]), "a second call"
    for opt in [{"flow_seg_rows": winsize}, {"flow_seg_rows": 4 * winsize}, {"flow_max_pairs": 1}]:
        f, i = run(name, batch, **opt)
        assert torch.equal(f, flow), (opt, float((f - flow).abs().max()), float((f != flow).float().mean()))
        assert torch.equal(i, img), opt
    for k, case in enumerate(batch):          # a pair's result does not depend on its batch
        f, i = run(name, [case])
        assert torch.equal(f[0], flow[k]) and torch.equal(i[0], img[k]), fc.case_id(case)


@pytest.mark.parametrize("name", ["init_lit", "init_gauss"])
def test_in_place_equals_out_of_place_also_across_chunks(name):
    eng = engine()
    batch = gc.batch_of(name, gc.SMALL)
    frames = torch.from_numpy(fc.frames_of(batch)).cuda()
    flow, img = batch_result(name, gc.SMALL)
    for chunk in (0, 1):
        buf = torch.from_numpy(gc.initial_fields(name, batch)).cuda()
        eng.set_option("flow_max_pairs", chunk)
        try:
            got_f, got_i = eng.optical_flow_in_place(frames, buf, want_image=True, **gc.SETS[name][0])
        finally:
            eng.set_option("flow_max_pairs", 0)
        assert got_f.data_ptr() == buf.data_ptr()
        assert np.array_equal(buf.cpu().numpy(), flow) and np.array_equal(got_i.cpu().numpy(), img), chunk


def test_an_overlap_that_is_not_the_same_buffer_is_refused():
    eng = engine()
    batch = gc.batch_of("init_lit", gc.SMALL)
    frames = torch.from_numpy(fc.frames_of(batch)).cuda()
    T, _, H, W, _ = frames.shape
    big = torch.zeros((T + 1, H, W, 2), dtype=torch.float32, device="cuda")
    p = gc.SETS["init_lit"][0]
    fb = H * W * 3
    import ctypes as C
    rc = eng.lib.relax_optical_flow_flags(eng.h, C.c_void_p(frames.data_ptr()), C.c_void_p(frames.data_ptr() + fb), 2 * fb, T, H, W, p["pyr_scale"],
                                          p["levels"], p["winsize"], p["iterations"], p["poly_n"], p["poly_sigma"], p["flags"],
                                          C.c_void_p(big[1:].data_ptr()), C.c_void_p(big.data_ptr()), None, None)
    assert rc == -1 and "overlap" in eng.lib.relax_last_error(eng.h).decode()


@pytest.mark.parametrize("name", ["gauss9", "init_lit"])
def test_flow_only_and_image_only_calls_agree_with_the_call_for_both(name):
    """gauss9: one iteration on the finest level - the magnitude range rides on the only gauss_solve_any launch of level 0."""
    eng = engine()
    batch = gc.batch_of(name, gc.SMALL)
    flow, img = batch_result(name, gc.SMALL)
    frames = torch.from_numpy(fc.frames_of(batch)).cuda()
    init = gc.initial_fields(name, batch)
    init = None if init is None else torch.from_numpy(init).cuda()
    f, none = eng.optical_flow(frames, want_flow=True, want_image=False, **gc.SETS[name][0], initial_flow=init, extended=True)
    assert none is None and np.array_equal(f.cpu().numpy(), flow)
    none, i = eng.optical_flow(frames, want_flow=False, want_image=True, **gc.SETS[name][0], initial_flow=init, extended=True)
    assert none is None and np.array_equal(i.cpu().numpy(), img)
    assert np.array_equal(eng.flow_to_rgb(f).cpu().numpy(), img)


# ---- e. plumbing -----------------------------------------------------------------------------------------------------------------
def test_flow_params_keyword_carries_the_gaussian_window_into_full_clip_vector():
    from relax_vqa_amd import synth
    eng = engine()
    rn50_weights()
    vit_weights("vit_base")
    clip = torch.from_numpy(synth.synthetic_clip(2, 96, 128, clip_id=5)).cuda()
    gauss = {"flags": 256, "extended": True}
    got = eng.full_clip_vector(clip, flow=True, flow_params=gauss)
    _, img_g = eng.optical_flow(clip, flags=256, extended=True)
    _, img_lit = eng.optical_flow(clip)
    assert not torch.equal(img_g, img_lit)
    assert torch.equal(got, eng.full_clip_vector(clip, flow_images=img_g))
    assert not torch.equal(got, eng.full_clip_vector(clip, flow=True))
    with pytest.raises(ValueError, match="initial_flow"):
        eng.full_clip_vector(clip, flow=True, flow_params={"flags": 4, "extended": True, "initial_flow": torch.zeros((2, 96, 128, 2))})
    with pytest.raises(RuntimeError, match="OPTFLOW_FARNEBACK_GAUSSIAN \\(256\\): the Gaussian window has no oracle here"):
        eng.optical_flow(clip, flags=256)
    with pytest.raises(RuntimeError, match="OPTFLOW_USE_INITIAL_FLOW \\(4\\): an initial flow has no oracle here"):
        eng.optical_flow(clip, flags=4)
    with pytest.raises(ValueError, match="extended"):
        eng.optical_flow(clip, flags=4, initial_flow=torch.zeros((2, 96, 128, 2)))
    with pytest.raises(RuntimeError, match="init_flow is NULL"):
        eng.optical_flow(clip, flags=4, extended=True)
    with pytest.raises(RuntimeError, match="init_flow is given"):
        eng.optical_flow(clip, flags=256, extended=True, initial_flow=torch.zeros((2, 96, 128, 2)))
    flow, _ = eng.optical_flow(clip, want_flow=True, flags=256, extended=True)     # the handle works on after a refusal
    assert bool(torch.isfinite(flow).all())
