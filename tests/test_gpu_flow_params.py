"""Farneback flow with OpenCV's parameters as arguments on the GPU (relax_optical_flow_ex; RelaxEngine.optical_flow's keywords), on the
parameter sets of tests/flow_param_cases.py: the flow against oracle/flow_ref.farneback with the same parameters in float64, in units of the
float32 oracle's own distance from it (gate from profiles/flow_params_parity.json); the flow image against the oracle's; the literal set
through the _ex entry bit-equal to relax_optical_flow; every set bit-stable over runs, batches, chunks, forced row segmentations and -
where a set has both - the two iteration paths; one deliberately wrong reference; and the flow_params keyword of the clip methods."""
import functools

import numpy as np
import pytest
import torch

from oracle import flow_ref
from tests import flow_cases as fc
from tests import flow_param_cases as pc
from tests.gpu_common import engine, rn50_weights, vit_weights

pytestmark = pytest.mark.gpu

DEFAULTS = {"flow_fused": 1, "flow_seg_rows": 0, "flow_max_pairs": 0}
SET_SIZES = pc.set_sizes()
SET_SIZE_IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in SET_SIZES]
GATED = pc.gated_cases()


def run(name, cases, **options):
    """Flow and flow image of the pairs of `cases` under the set's parameters in ONE call through relax_optical_flow_ex, under the given
    options (restored afterwards)."""
    eng = engine()
    frames = torch.from_numpy(fc.frames_of(cases)).cuda()
    try:
        for k, v in options.items():
            assert eng.get_option(k) == DEFAULTS[k], k
            eng.set_option(k, v)
        return eng.optical_flow_ex(frames, want_flow=True, want_image=True, **pc.SETS[name][0])
    finally:
        for k in options:
            eng.set_option(k, DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def batch_result(name, size):
    """-> (flow, image) on the host of the set's batch at a size: one GPU call, computed once"""
    flow, img = run(name, pc.batch_of(name, size))
    return flow.cpu().numpy(), img.cpu().numpy()


def gpu_result(name, case):
    batch = pc.batch_of(name, case[:2])
    flow, img = batch_result(name, case[:2])
    return flow[batch.index(case)], img[batch.index(case)]


def measure_ratios():
    """{case id: the gated figure} of every gated case (tools/flow_params_parity.py records them)"""
    out = {}
    for name, case in GATED:
        f64, f32 = pc.reference(pc.SETS[name][0], case)
        out[pc.gated_id((name, case))] = pc.case_ratio(name, gpu_result(name, case)[0], f64, f32)
    return out


# ---- a. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", GATED, ids=[pc.gated_id(i) for i in GATED])
def test_flow_parity_per_case(item):
    name, case = item
    f64, f32 = pc.reference(pc.SETS[name][0], case)
    flow = gpu_result(name, case)[0]
    assert np.isfinite(flow).all()
    mean_r, max_r = pc.parity_terms(flow, f64, f32)
    ratio, gate = pc.case_ratio(name, flow, f64, f32), pc.parity_gate()
    print(f"{pc.gated_id(item)}: mean ratio {mean_r:.3f}, max ratio {max_r:.3f}, gated figure {ratio:.3f} (gate {gate:g}); "
          f"max |gpu - fp64| {np.abs(flow - f64).max():.2e}, max |fp32 oracle - fp64| {np.abs(f32 - f64).max():.2e}")
    assert ratio <= gate, (ratio, gate)


@pytest.mark.parametrize("item", GATED, ids=[pc.gated_id(i) for i in GATED])
def test_flow_image_per_case(item):
    name, case = item
    want = flow_ref.flow_to_rgb(pc.reference(pc.SETS[name][0], case)[1])
    d = np.abs(gpu_result(name, case)[1].astype(np.int32) - want.astype(np.int32))
    print(f"{pc.gated_id(item)}: equal {(d == 0).mean():.5f}, within 1 {(d <= 1).mean():.5f}")
    assert (d == 0).mean() > 0.995 and (d <= 1).mean() > 0.9995, ((d == 0).mean(), (d <= 1).mean())     # test_flow_image_per_case's thresholds


# ---- b. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", pc.SETS["literal"][1], ids=["97x131", "256x264"])
def test_literal_set_through_ex_is_the_old_entry_bit_for_bit(size):
    """relax_optical_flow_ex at (0.5, 3, 15, 3, 5, 1.2, 0) against relax_optical_flow: flow and image, in a batch of three and alone."""
    eng = engine()
    batch = pc.batch_of("literal", size)
    frames = torch.from_numpy(fc.frames_of(batch)).cuda()
    old_f, old_i = eng.optical_flow(frames, want_flow=True, want_image=True)
    new_f, new_i = eng.optical_flow_ex(frames, want_flow=True, want_image=True, **pc.LITERAL, flags=0)
    assert torch.equal(new_f, old_f) and torch.equal(new_i, old_i)
    kw_f, kw_i = eng.optical_flow(frames, want_flow=True, want_image=True, **pc.LITERAL)      # the keywords at their defaults: the old entry
    assert torch.equal(kw_f, old_f) and torch.equal(kw_i, old_i)
    for k in range(len(batch)):
        f, i = eng.optical_flow_ex(frames[k:k + 1], want_flow=True, want_image=True, **pc.LITERAL)
        o_f, o_i = eng.optical_flow(frames[k:k + 1], want_flow=True, want_image=True)
        assert torch.equal(f, o_f) and torch.equal(i, o_i)
        assert torch.equal(f[0], old_f[k]) and torch.equal(i[0], old_i[k])


def both_paths(name):
    """flow_fused 0 / 1 pick different kernels for the 15-pixel window only (flow_iteration | update_matrices_k + box_solve_fused)."""
    return pc.SETS[name][0]["winsize"] == 15


@pytest.mark.parametrize("name,size", SET_SIZES, ids=SET_SIZE_IDS)
def test_every_set_gives_the_same_bits_whatever_the_run_batch_chunk_segmentation_and_path(name, size):
    batch = pc.batch_of(name, size)
    winsize = pc.SETS[name][0]["winsize"]
    flow, img = run(name, batch)
    assert bool(torch.isfinite(flow).all())
    again_f, again_i = run(name, batch)
    assert torch.equal(again_f, flow) and torch.equal(again_i, img), "a second call"
    options = [{"flow_seg_rows": winsize}, {"flow_seg_rows": 4 * winsize}]
    if len(batch) > 1:
        options.append({"flow_max_pairs": 1})
    if both_paths(name):
        options.append({"flow_fused": 0})
    for opt in options:
        f, i = run(name, batch, **opt)
        assert torch.equal(f, flow), (opt, float((f - flow).abs().max()), float((f != flow).float().mean()))
        assert torch.equal(i, img), opt
    if len(batch) > 1:
        for k, case in enumerate(batch):          # a pair's result does not depend on its batch
            f, i = run(name, [case])
            assert torch.equal(f[0], flow[k]) and torch.equal(i[0], img[k]), fc.case_id(case)


def test_flow_only_and_image_only_calls_agree_with_the_call_for_both():
    """win9: one iteration on the finest level - the magnitude range rides on the only box launch of level 0."""
    batch = pc.batch_of("win9", pc.SMALL)
    flow, img = run("win9", batch)
    eng = engine()
    frames = torch.from_numpy(fc.frames_of(batch)).cuda()
    f, none = eng.optical_flow(frames, want_flow=True, want_image=False, **pc.SETS["win9"][0])
    assert none is None and torch.equal(f, flow)
    none, i = eng.optical_flow(frames, want_flow=False, want_image=True, **pc.SETS["win9"][0])
    assert none is None and torch.equal(i, img)
    assert torch.equal(eng.flow_to_rgb(flow), img)


# ---- c. the gate sees the parameters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wrong", [("win33", {"winsize": 35}), ("win9", {"winsize": 11}), ("poly7", {"poly_n": 5})],
                         ids=["win33-vs-35", "win9-vs-11", "poly7-vs-poly5"])
def test_a_reference_with_another_parameter_fails_the_gate_by_a_wide_margin(name, wrong):
    params, sizes = pc.SETS[name]
    case = pc.pair_case(sizes[0], pc.SMOOTH)
    f64, f32 = pc.reference({**params, **wrong}, case)
    ratio = pc.case_ratio(name, gpu_result(name, case)[0], f64, f32)
    print(f"{name} against the oracle with {wrong}: ratio {ratio:.1f} (gate {pc.parity_gate():g})")
    assert ratio > 16 * fc.PARITY_CAP, ratio


# ---- d. the plan and the refusals on a live handle --------------------------------------------------------------------------------
def test_flow_plan_through_the_engine_and_refusals_with_a_handle():
    eng = engine()
    plan = eng.flow_plan(1024, 1056, 0.5, 5)
    assert [(p["h"], p["w"], p["ksize"]) for p in plan] == [(32, 33, 79), (64, 66, 39), (128, 132, 19), (256, 264, 9), (512, 528, 3), (1024, 1056, 3)]
    frames = torch.from_numpy(fc.frames_of(pc.batch_of("win9", pc.SMALL)[:1])).cuda()
    for bad, word in [({"winsize": 14}, "winsize=14"), ({"poly_n": 6}, "poly_n=6"), ({"flags": 4}, "OPTFLOW_USE_INITIAL_FLOW"),
                      ({"flags": 256}, "OPTFLOW_FARNEBACK_GAUSSIAN"), ({"pyr_scale": 0.6, "levels": 8}, "levels=8")]:
        frames_ = frames if "levels" not in bad else torch.zeros((1, 2, 2048, 2048, 3), dtype=torch.uint8, device="cuda")
        with pytest.raises(RuntimeError, match=word):
            eng.optical_flow(frames_, **bad)
    flow, _ = eng.optical_flow(frames, want_flow=True, **pc.SETS["win9"][0])     # the handle works on after a refusal
    assert bool(torch.isfinite(flow).all())


# ---- e. the keyword through the clip methods ---------------------------------------------------------------------------------------
def test_flow_params_keyword_reaches_the_flow_of_full_clip_vector():
    from relax_vqa_amd import synth
    eng = engine()
    rn50_weights()
    vit_weights("vit_base")
    clip = torch.from_numpy(synth.synthetic_clip(2, 96, 128, clip_id=5)).cuda()
    poly7 = pc.SETS["poly7"][0]
    got = eng.full_clip_vector(clip, flow=True, flow_params=poly7)
    _, img7 = eng.optical_flow(clip, **poly7)
    _, img_lit = eng.optical_flow(clip)
    assert not torch.equal(img7, img_lit)
    by_hand = eng.full_clip_vector(clip, flow_images=img7)
    assert torch.equal(got, by_hand)
    today = eng.full_clip_vector(clip, flow=True)
    assert torch.equal(eng.full_clip_vector(clip, flow=True, flow_params=None), today)
    assert torch.equal(today, eng.full_clip_vector(clip, flow_images=img_lit))
    assert not torch.equal(got, today)
    feats = eng.whole_residual_features(clip, "optical_flow", resnet=True, vit=False, flow_params=poly7)
    want = eng.whole_residual_features(clip, "optical_flow", resnet=True, vit=False, flow_images=img7)
    assert torch.equal(feats["resnet"], want["resnet"])
