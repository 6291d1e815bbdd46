"""Backbone parity on the GPU: ResNet-50 layer-stack / pool and ViT tokens / pool against the oracle, plus the
reference-derived ViT golden tokens and the whole-clip path."""
import os

import numpy as np
import pytest
import torch

from oracle import fragment_ref, pooling_ref, resnet50_ref, vit_ref
from tests.gpu_common import WEIGHT_SET_IDS, WEIGHT_SETS, assert_close, engine, golden_tag, rn50_weights, synth, vit_weights

pytestmark = pytest.mark.gpu


def _fragments(n, seed=0):
    frs = []
    for i in range(n):
        o, nx = synth.synthetic_pair(240, 320, 500 + seed * 64 + i)
        f = fragment_ref.fragment_pair(o, nx)
        frs.append(f["ori_frag"] if i % 2 == 0 else f["diff_frag"])
    return np.stack(frs)


@pytest.mark.parametrize("adversarial", WEIGHT_SETS, ids=WEIGHT_SET_IDS)
def test_resnet50_taps_and_features(each_precision, each_split_k, adversarial):
    """Every hooked activation and both feature vectors, on the regular synthetic weights, on the adversarial set (BatchNorm
    variances over 1e-3..10, gammas of mixed sign) and on the outlier set (one channel per stage 50 - 100 x the others, dead channel
    groups: what the per-image scales of the f16x2 layers must survive), on every arithmetic."""
    sd = rn50_weights(adversarial)
    frags = _fragments(3)
    ls, pool, taps = engine().resnet50_features(torch.from_numpy(frags).cuda(), taps=range(15))
    torch.cuda.synchronize()
    tsd = resnet50_ref.to_torch_state_dict(sd)
    ref_taps, ref_avg = resnet50_ref.forward_taps(tsd, resnet50_ref.preprocess_bgr_u8(frags))
    for i, name in enumerate(pooling_ref.RESNET50_TAPS):      # every hooked activation, in tap order
        assert_close(taps[i], ref_taps[name].numpy(), name, channel_axis=1 if adversarial == "outliers" else None)   # (the per-channel floor: its argument holds for the hot channels of that set alone)
    want_ls = resnet50_ref.layer_stack_features(tsd, frags)
    want_pool = resnet50_ref.pool_features(tsd, frags)
    off = 0
    for name, c in zip(pooling_ref.RESNET50_TAPS, pooling_ref.RESNET50_TAP_CHANNELS):
        assert_close(ls[:, off:off + c], want_ls[:, off:off + c], f"layer-stack block {name}")
        off += c
    assert_close(pool[:, :2048], want_pool[:, :2048], "pool vector")
    assert_close(pool[:, 2048:], want_pool[:, 2048:], "pool stats (mean,max,std)")
    rn50_weights()   # the shared engine goes back to the regular set


def test_resnet50_pool_only_and_batch_independence(each_precision):
    rn50_weights()
    frags = _fragments(5, seed=1)
    ls_all, pool_all = engine().resnet50_features(torch.from_numpy(frags).cuda())
    none_ls, pool_only = engine().resnet50_features(torch.from_numpy(frags).cuda(), layer_stack=False, pool=True)
    assert none_ls is None
    assert torch.equal(pool_only, pool_all)
    # a different batch composition changes which tail tiles are K-split: equal to fp32 rounding by default ...
    ls_one, pool_one = engine().resnet50_features(torch.from_numpy(frags[3:4]).cuda())
    assert_close(ls_one[0], ls_all[3].cpu().numpy(), "batch 1 vs batch 5 layer-stack", rtol=1e-5, atol_frac=1e-5)
    # ... and bit-identical with the split switched off (the mode for comparing sharded runs)
    engine().set_option("gemm_split_k", 0)
    try:
        ls_a, pool_a = engine().resnet50_features(torch.from_numpy(frags).cuda())
        ls_b, pool_b = engine().resnet50_features(torch.from_numpy(frags[3:4]).cuda())
        assert torch.equal(ls_b[0], ls_a[3]) and torch.equal(pool_b[0], pool_a[3]), "result depends on batch"
        again, _ = engine().resnet50_features(torch.from_numpy(frags).cuda())
        assert torch.equal(again, ls_a), "not deterministic"
    finally:
        engine().set_option("gemm_split_k", 1)
    again, _ = engine().resnet50_features(torch.from_numpy(frags).cuda())
    assert torch.equal(again, ls_all), "not deterministic with split-K"


@pytest.mark.parametrize("adversarial", WEIGHT_SETS, ids=WEIGHT_SET_IDS)
@pytest.mark.parametrize("name,heads", [("vit_tiny", 3), ("vit_base", 12)])
def test_vit_matches_reference_golden_tokens(golden_dir, name, heads, each_precision, each_split_k, adversarial):
    """Tokens computed by the reference's own VisionTransformer class; the adversarial weights drive the attention kernel's
    max subtraction / exp2 path with logits of +-20 (near one-hot softmax rows); the outlier set has five residual-stream channels
    hundreds of times the median with LayerNorm gains up to 10 on them (every static f16x2 scale is 2^7 - 2^10 loose for the other
    763 channels) and a near-one-hot head."""
    vit_weights(name, adversarial)
    z = np.load(os.path.join(golden_dir, f"{name}{golden_tag(adversarial)}_tokens.npz"))
    tokens, pooled = engine().vit_features(torch.from_numpy(z["frags"]).cuda(), tokens=True, pooled=True)
    assert_close(tokens, z["tokens"], f"{name} tokens vs reference VisionTransformer")
    want = np.stack([pooling_ref.vit_pool_vector(t) for t in z["tokens"]])
    assert_close(pooled, want, f"{name} pooled vs reference process_video_feature")


def test_vit_base_oracle_batch(each_precision, each_split_k):
    sd = vit_weights("vit_base")
    frags = _fragments(3, seed=2)
    tokens, pooled = engine().vit_features(torch.from_numpy(frags).cuda(), tokens=True, pooled=True)
    tsd = vit_ref.to_torch_state_dict(sd)
    assert_close(tokens, vit_ref.tokens(tsd, frags, 12), "vit_base tokens")
    assert_close(pooled, vit_ref.pool_features(tsd, frags, 12), "vit_base pooled")


def test_config1_eight_224_frames_pool_path():
    """BASELINE config 1: 8 sampled frames already 224x224 -> every one of the 14x14 patches is kept, in raster order,
    so the original fragment IS the frame; ResNet-50 `pool` path -> [8, 2051]."""
    sd = rn50_weights()
    clip = synth.synthetic_clip(8, 224, 224, clip_id=11)
    frag = engine().fragment_pairs(torch.from_numpy(clip).cuda())
    assert frag["counts"].tolist() == [196] * 8
    raster = np.stack(np.divmod(np.arange(196), 14), 1).astype(np.int32)
    assert np.array_equal(frag["positions"].cpu().numpy(), np.broadcast_to(raster, (8, 196, 2)))
    assert np.array_equal(frag["ori_frag"].cpu().numpy(), clip[:, 0])
    assert np.array_equal(frag["diff_frag"].cpu().numpy(), fragment_ref.absdiff(clip[:, 0], clip[:, 1]))
    _, pool = engine().resnet50_features(frag["ori_frag"], layer_stack=False, pool=True)
    want = resnet50_ref.pool_features(resnet50_ref.to_torch_state_dict(sd), clip[:, 0])
    assert pool.shape == (8, 2051)
    assert_close(pool, want, "config 1 pool features")


def test_extract_clip_config2_shape_720p():
    """BASELINE config 2 (720p, residual-fragment + RN50 layer-stack) on a short clip, against the oracle."""
    sd = rn50_weights()
    T = 3
    clip = synth.synthetic_clip(T, 720, 1280, clip_id=2)
    out = engine().extract_clip(torch.from_numpy(clip).cuda(), resnet=True, vit=False)
    tsd = resnet50_ref.to_torch_state_dict(sd)
    refs = [fragment_ref.fragment_pair(clip[t, 0], clip[t, 1]) for t in range(T)]
    assert np.array_equal(out["positions"].cpu().numpy(), np.stack([r["positions"] for r in refs]))
    want = np.concatenate([resnet50_ref.layer_stack_features(tsd, np.stack([r["ori_frag"] for r in refs])),
                           resnet50_ref.pool_features(tsd, np.stack([r["diff_frag"] for r in refs]))], axis=1)
    assert out["resnet"].shape == (T, 15171)
    assert_close(out["resnet"][:, :13120], want[:, :13120], "clip layer-stack")
    assert_close(out["resnet"][:, 13120:], want[:, 13120:], "clip residual pool")


def test_extract_clip_config3_1080p_with_vit(each_precision):
    sd_r, sd_v = rn50_weights(), vit_weights("vit_base")
    T = 2
    clip = synth.synthetic_clip(T, 1080, 1920, clip_id=3)
    out = engine().extract_clip(torch.from_numpy(clip).cuda())
    refs = [fragment_ref.fragment_pair(clip[t, 0], clip[t, 1]) for t in range(T)]
    assert np.array_equal(out["positions"].cpu().numpy(), np.stack([r["positions"] for r in refs]))
    ori, res = np.stack([r["ori_frag"] for r in refs]), np.stack([r["diff_frag"] for r in refs])
    tv = vit_ref.to_torch_state_dict(sd_v)
    want_vit = np.concatenate([vit_ref.pool_features(tv, ori, 12), vit_ref.pool_features(tv, res, 12)], axis=1)
    assert out["vit"].shape == (T, 4608) and out["resnet"].shape == (T, 15171)
    assert_close(out["vit"], want_vit, "clip vit pooled")
    tr = resnet50_ref.to_torch_state_dict(sd_r)
    assert_close(out["resnet"][:, :13120], resnet50_ref.layer_stack_features(tr, ori), "clip layer-stack 1080p")
    vec = engine().clip_vector(torch.from_numpy(clip).cuda())
    assert vec.shape == (15171 + 4608,)


def test_clip_vectors_batch_of_mixed_resolutions_config4_shape(each_precision):
    """BASELINE config 4 shape (540p) next to a 720p clip in ONE batched pass; each row must equal the clip processed
    alone (to fp32 rounding with the default tail split-K, bit for bit without it)."""
    rn50_weights(), vit_weights("vit_base")
    eng = engine()
    a = torch.from_numpy(synth.synthetic_clip(3, 540, 960, clip_id=40)).cuda()
    b = torch.from_numpy(synth.synthetic_clip(2, 720, 1280, clip_id=41)).cuda()
    both = eng.clip_vectors([a, b])
    assert both.shape == (2, 15171 + 4608)
    alone = torch.stack([eng.clip_vector(a), eng.clip_vector(b)])
    assert_close(both, alone.cpu().numpy(), "batched vs single clips", rtol=1e-4, atol_frac=1e-5)
    eng.set_option("gemm_split_k", 0)
    try:
        both0 = eng.clip_vectors([a, b])
        alone0 = torch.stack([eng.clip_vector(a), eng.clip_vector(b)])
        assert torch.equal(both0, alone0), "batching changed bits with split-K off"
    finally:
        eng.set_option("gemm_split_k", 1)


def test_bf16x3_mode_meets_the_feature_tolerance():
    """The opt-in bf16x3 precision (hi/lo bf16 split products, fp32 accumulate) against the fp32 oracle: the 1e-3 feature
    bar of the north star holds with ~100x margin in norm-relative terms."""
    sd_r, sd_v = rn50_weights(), vit_weights("vit_base")
    eng = engine()
    frags = _fragments(4, seed=5)
    eng.set_precision("bf16x3")
    try:
        ls, pool = eng.resnet50_features(torch.from_numpy(frags).cuda())
        _, pooled = eng.vit_features(torch.from_numpy(frags).cuda(), tokens=False, pooled=True)
    finally:
        eng.set_precision("bf16x6")
    tr, tv = resnet50_ref.to_torch_state_dict(sd_r), vit_ref.to_torch_state_dict(sd_v)
    want_ls, want_pool = resnet50_ref.layer_stack_features(tr, frags), resnet50_ref.pool_features(tr, frags)
    want_vit = vit_ref.pool_features(tv, frags, 12)
    for name, got, want in (("layer-stack", ls, want_ls), ("pool", pool, want_pool), ("vit pooled", pooled, want_vit)):
        got = got.cpu().numpy()
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel < 5e-5, (name, rel)
        assert_close(got, want, f"bf16x3 {name}")   # and the element-wise bar of the fp32 tests (measured: <= 0.38 of it; fp32: <= 0.03)
        assert_close(got, want, f"bf16x3 {name}", rtol=1e-3, atol_frac=2e-4)


def test_step_is_graph_capturable():
    """The C-ABI only enqueues on the caller's stream (no allocation after warm-up, no host sync): a whole clip pass can be
    captured into a HIP graph and replayed with bit-identical results."""
    rn50_weights(), vit_weights("vit_base")
    eng = engine()
    clip = torch.from_numpy(synth.synthetic_clip(2, 240, 320, clip_id=77)).cuda()
    ref = eng.clip_vectors([clip])
    torch.cuda.synchronize()
    poison = eng.get_option("debug_poison")     # the debugging aid fills workspaces synchronously: not a thing to capture
    eng.set_option("debug_poison", 0)
    try:
        _capture_and_replay(eng, clip, ref)
    finally:
        eng.set_option("debug_poison", poison)


def _capture_and_replay(eng, clip, ref):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.clip_vectors([clip])
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            out = eng.clip_vectors([clip])
    torch.cuda.synchronize()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_headline_batch_equals_clip_by_clip_at_full_size():
    """The bench workload itself (BASELINE config 3: 1080p, 32 pairs, 8 clips per pass = 512 fragments through both
    backbones): with the tail split off, the batched pass gives every clip the bits it gets alone, and two runs agree."""
    rn50_weights(), vit_weights("vit_base")
    eng = engine()
    clips = [torch.from_numpy(synth.synthetic_clip(32, 1080, 1920, clip_id=300 + i, distinct=2)).cuda() for i in range(8)]
    eng.set_option("gemm_split_k", 0)
    try:
        both = eng.clip_vectors(clips)
        again = eng.clip_vectors(clips)
        assert both.shape == (8, 15171 + 4608) and bool(torch.isfinite(both).all())
        assert torch.equal(both, again), "not deterministic"
        for i in (0, 5):
            assert torch.equal(eng.clip_vectors([clips[i]])[0], both[i]), f"clip {i} depends on its batch"
    finally:
        eng.set_option("gemm_split_k", 1)
    split = eng.clip_vectors(clips)     # default (tail split on): same to fp32 rounding
    assert_close(split, both.cpu().numpy(), "tail split-K on vs off", rtol=1e-5, atol_frac=1e-5)


def test_bf16x3_at_the_headline_batch_uses_the_large_tiles_and_holds_the_bar():
    """8 clips x 64 fragments: the ViT GEMMs have >= 256 tiles of 256x256, so the opt-in precision runs its 8-wave kernel;
    clip vectors against the exact-fp32 path of the same engine."""
    rn50_weights(), vit_weights("vit_base")
    eng = engine()
    clips = [torch.from_numpy(synth.synthetic_clip(32, 1080, 1920, clip_id=320 + i, distinct=2)).cuda() for i in range(8)]
    eng.set_precision("fp32")
    exact = eng.clip_vectors(clips).cpu().numpy()
    eng.set_precision("bf16x3")
    fast = eng.clip_vectors(clips).cpu().numpy()
    rel = np.linalg.norm(fast - exact) / np.linalg.norm(exact)
    assert rel < 5e-5, rel
    assert_close(fast, exact, "bf16x3 clip vectors vs fp32")


def test_clip_features_entry_point_equals_the_two_group_calls(each_precision):
    """relax_resnet50_clip_features: layer stack of the first group, pool of the second, one forward - the values the classic entry
    point gives on the respective images (bit for bit without the tail split), also with an empty group."""
    rn50_weights()
    eng = engine()
    frags = torch.from_numpy(_fragments(7, seed=4)).cuda()
    eng.set_option("gemm_split_k", 0)
    try:
        ls_all, pool_all = eng.resnet50_features(frags, layer_stack=True, pool=True)
        for n_ls in (0, 3, 7):
            ls, pool = eng.resnet50_clip_features(frags, n_ls)
            assert ls.shape == (n_ls, 13120) and pool.shape == (7 - n_ls, 2051)
            assert torch.equal(ls, ls_all[:n_ls]), f"layer stack of a {n_ls} + {7 - n_ls} batch"
            assert torch.equal(pool, pool_all[n_ls:]), f"pool of a {n_ls} + {7 - n_ls} batch"
    finally:
        eng.set_option("gemm_split_k", 1)
    with pytest.raises(ValueError, match="n_layer_stack"):
        eng.resnet50_clip_features(frags, 9)
    rc = eng.lib.relax_resnet50_clip_features(eng.h, frags.data_ptr(), 7, 9, None, None, None)      # the C entry refuses it too
    assert rc == -1 and b"bad arguments" in eng.lib.relax_last_error(eng.h)
