"""The code path the bench times, directly under the oracle (round-2 review, "weak" 2 and 3): batches large enough that the ViT
GEMMs run unsplit 256x256 tiles through the in-kernel epilogue with the DEFAULT tail split on (32 fragments: fc1 = 25 x 12 =
300 tiles >= the 256 workgroup slots) and that conv1_x6's persistent workgroups reuse both patch buffers in steady state
(32 x 49 = 1568 tiles over 256 workgroups = 6 per workgroup).  All 15 ResNet taps, the patch tokens and every feature vector
are compared element-wise with the CPU oracle; the oracle results are computed once per module."""
import functools

import numpy as np
import pytest
import torch

from oracle import fragment_ref, pooling_ref, resnet50_ref, vit_ref
from tests.gpu_common import assert_close, engine, rn50_weights, synth, vit_weights

pytestmark = pytest.mark.gpu
N_FRAGS = 32


@functools.lru_cache(maxsize=None)
def _fragments():
    frs = []
    for i in range(N_FRAGS):
        o, nx = synth.synthetic_pair(240, 320, 9000 + i)
        f = fragment_ref.fragment_pair(o, nx)
        frs.append(f["ori_frag"] if i % 2 == 0 else f["diff_frag"])
    return np.stack(frs)


@functools.lru_cache(maxsize=None)
def _resnet_oracle():
    tsd = resnet50_ref.to_torch_state_dict(synth.resnet50_state_dict())
    frags = _fragments()
    taps, _ = resnet50_ref.forward_taps(tsd, resnet50_ref.preprocess_bgr_u8(frags))
    return ({k: v.numpy() for k, v in taps.items()}, resnet50_ref.layer_stack_features(tsd, frags),
            resnet50_ref.pool_features(tsd, frags))


@functools.lru_cache(maxsize=None)
def _vit_oracle():
    tsd = vit_ref.to_torch_state_dict(synth.vit_state_dict("vit_base"))
    frags = _fragments()
    return vit_ref.tokens(tsd, frags, 12), vit_ref.pool_features(tsd, frags, 12)


def test_resnet50_32_fragments_all_taps_against_the_oracle(each_precision, each_split_k):
    rn50_weights()
    want_taps, want_ls, want_pool = _resnet_oracle()
    ls, pool, taps = engine().resnet50_features(torch.from_numpy(_fragments()).cuda(), taps=range(15))
    torch.cuda.synchronize()
    for i, name in enumerate(pooling_ref.RESNET50_TAPS):
        assert_close(taps[i], want_taps[name], f"{name} at 32 fragments")
        del taps[i]
    off = 0
    for name, c in zip(pooling_ref.RESNET50_TAPS, pooling_ref.RESNET50_TAP_CHANNELS):
        assert_close(ls[:, off:off + c], want_ls[:, off:off + c], f"layer-stack block {name} at 32 fragments")
        off += c
    assert_close(pool[:, :2048], want_pool[:, :2048], "pool vector at 32 fragments")
    assert_close(pool[:, 2048:], want_pool[:, 2048:], "pool stats at 32 fragments")


def test_vit_base_32_fragments_tokens_against_the_oracle(each_precision, each_split_k):
    vit_weights("vit_base")
    want_tokens, want_pooled = _vit_oracle()
    tokens, pooled = engine().vit_features(torch.from_numpy(_fragments()).cuda(), tokens=True, pooled=True)
    assert_close(tokens, want_tokens, "vit_base tokens at 32 fragments")
    assert_close(pooled, want_pooled, "vit_base pooled at 32 fragments")


def test_clip_vectors_of_one_bench_sized_clip_against_the_oracle_pipeline():
    """One 540p clip of 16 pairs (config 4's clip shape: 32 fragments per backbone pass) through clip_vectors - the call the
    bench loop makes - against the oracle pipeline's de-duplicated schedule, block by block of the 19779 vector."""
    from oracle import pipeline_ref
    rn, vit = rn50_weights(), vit_weights("vit_base")
    clip = synth.synthetic_clip(16, 540, 960, clip_id=77)
    got = engine().clip_vectors([torch.from_numpy(clip).cuda()])[0]
    want = pipeline_ref.clip_features(clip, rn, vit, schedule="dedup")
    want = np.concatenate([want["resnet"], want["vit"]], axis=1).mean(axis=0)
    edges = [0, 13120, 15171, 15171 + 2304, 19779]
    for a, b, nm in zip(edges[:-1], edges[1:], ["RN50 layer stack", "RN50 residual pool", "ViT original", "ViT residual"]):
        assert_close(got[a:b], want[a:b], f"clip vector block: {nm}")


def test_bench_dump_outputs_hold_what_the_timed_path_returned(tmp_path):
    """bench.py --dump-outputs: DIR/clip_vectors.npy is the output of the LAST timed step - config 4's clip shape, one clip per step,
    two timed steps: step 1 takes resident clip 1 (synthetic_clip(16, 540, 960, clip_id=1, distinct=4)) - and the result line
    carries the step count asked for and ms_per_step.  The same clip through clip_vectors here gives the same vector."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = tmp_path / "outputs"
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", "config4", "--clips-per-step", "1",
                          "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-fast-mode", "--no-h2d", "--no-measure-traffic",
                          "--dump-outputs", str(out_dir)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert os.listdir(out_dir) == ["clip_vectors.npy"]
    dumped = np.load(out_dir / "clip_vectors.npy")
    assert dumped.dtype == np.float32 and dumped.shape == (1, 19779)
    rn50_weights(), vit_weights("vit_base")
    clip = synth.synthetic_clip(16, 540, 960, clip_id=1, distinct=4)
    want = engine().clip_vectors([torch.from_numpy(clip).cuda()]).cpu().numpy()
    assert_close(dumped, want, "dumped clip vector vs clip_vectors", rtol=1e-5, atol_frac=1e-6)
