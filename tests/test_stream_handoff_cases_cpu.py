"""The inputs and the stand-in engine of tests/stream_handoff_cases.py, without a GPU: the fingerprint tells every clip from every
other and from its decoy, the ragged set holds the structure the GPU scenarios rely on, and the stand-in goes through
extract_dataset_clips on the CPU device (where the stager passes everything through) with and without loader threads."""
import itertools

import numpy as np
import torch

from relax_vqa_amd import dataset
from tests import stream_handoff_cases as hc


def _fp(a):
    return hc.fingerprint(torch.from_numpy(np.ascontiguousarray(a)))


def test_fingerprint_is_exact_and_changes_with_any_single_byte():
    clip = hc.clip_bytes((2, 2, 16, 16, 3), 1)
    base = _fp(clip)
    assert base.dtype == torch.float32 and base.shape == (hc.FP_DIM,)
    assert torch.equal(base, base.round()) and float(base.max()) < 4096 and float(base.min()) >= 0
    x = clip.reshape(-1).astype(np.int64)
    k = np.arange(x.size, dtype=np.int64)
    sums = [int(x.sum()), int((x * (1 + k % 251)).sum()), int((x * (1 + (k // 251) % 241)).sum())]
    assert [int(v) for v in base] == [(s >> (12 * j)) & 0xFFF for s in sums for j in range(3)]
    flat = clip.reshape(-1)
    for at in range(flat.size):                              # every position, the smallest change and a large one
        for delta in (1, 128):
            other = flat.copy()
            other[at] = (int(other[at]) + delta) % 256
            assert not torch.equal(_fp(other.reshape(clip.shape)), base), (at, delta)
    swapped = flat.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert flat[0] != flat[1] and not torch.equal(_fp(swapped), base)              # the same bytes in another order
    full = np.full(hc.RAGGED[5], 255, np.uint8)                                     # the largest clip of the set, every byte 255
    assert full.size <= hc.FP_MAX_BYTES and int(full.astype(np.int64).sum()) == sum(int(v) << (12 * j) for j, v in enumerate(_fp(full)[:3]))


def test_every_generated_clip_and_decoy_has_its_own_fingerprint():
    sets = [c for which in (hc.REAL, hc.DECOY) for c in hc.ragged_clips(which) if c is not None]
    sets += [hc.clip_bytes(hc.FEEDER_SHAPES[i % 2], i, hc.REAL) for i in range(2 * hc.FEEDER_STEPS)]
    sets += [hc.clip_bytes(hc.FEEDER_SHAPES[j], 50 + j, hc.DECOY) for j in range(2)]
    prints = [tuple(_fp(c).tolist()) for c in sets]
    for (i, a), (j, b) in itertools.combinations(enumerate(prints), 2):
        assert a != b, (i, j)
    for real, decoy in zip(hc.ragged_clips(hc.REAL), hc.ragged_clips(hc.DECOY)):
        assert (real is None) == (decoy is None) and (real is None or (real.shape == decoy.shape and not np.array_equal(real, decoy)))


def test_ragged_set_holds_the_growth_batch_the_loader_error_and_the_refused_clip():
    shapes = hc.RAGGED
    assert 9 <= len(shapes) <= 10 and shapes[hc.ERROR_CLIP] is None and [i for i, s in enumerate(shapes) if s is None] == [hc.ERROR_CLIP]
    assert [i for i, s in enumerate(shapes) if s is not None and tuple(s[2:4]) == hc.REFUSED_HW] == [hc.REFUSED_CLIP]
    assert hc.REFUSED_CLIP // 2 != hc.ERROR_CLIP // 2 and shapes[hc.REFUSED_CLIP ^ 1] is not None      # refused INSIDE a batch: its neighbour is retried
    # batch 2 outgrows its block after its first clip (6 KiB, then 72 KiB); so does, by 768 bytes, the batch with the refused clip
    assert hc.slot_blocks(shapes, 2) == [(hc.GROWTH_BATCH, 1), (hc.REFUSED_CLIP // 2, 1)]
    assert hc.slot_blocks([s for s in shapes if s is not None][:2] * 5, 2) == []  # (equal clips never do)
    for s in shapes:
        if s is not None:
            assert s[0] <= 3 and s[1] == 2 and s[4] == 3 and 32 <= s[2] <= 64 and 32 <= s[3] <= 64 and s[2] % 2 == 0 and s[3] % 2 == 0
            dataset._check_clip(np.empty(s, np.uint8))
    assert len({s for s in shapes if s is not None}) > 3
    src = hc.host_source()
    try:
        src(hc.ERROR_CLIP)
        raise AssertionError("the error clip loaded")
    except OSError as e:
        assert "cannot decode" in str(e)


def test_stand_in_engine_on_the_cpu_device_with_and_without_loader_threads():
    cpu = torch.device("cpu")
    before = dataset.feature_dim
    inline, e0 = hc.run_pass(hc.host_source(), hc.FingerprintEngine(cpu), prefetch=0)
    eng = hc.FingerprintEngine(cpu)
    threaded, e2 = hc.run_pass(hc.host_source(), eng, prefetch=2, workers=3)
    alloc, e3 = hc.run_pass(hc.host_source(alloc=True), hc.FingerprintEngine(cpu), prefetch=2, workers=3)
    assert dataset.feature_dim is before
    assert e0 == e2 == e3 and [i for i, _ in e0] == [hc.ERROR_CLIP, hc.REFUSED_CLIP]
    assert "cannot decode" in e0[0][1] and "refused" in e0[1][1]
    assert inline.shape == (len(hc.RAGGED), hc.FP_DIM) and inline.dtype == torch.float32
    for got in (threaded, alloc):
        assert torch.equal(got.view(torch.int32), inline.view(torch.int32))
    clips = hc.ragged_clips()
    for i, c in enumerate(clips):
        if i in (hc.ERROR_CLIP, hc.REFUSED_CLIP):
            assert torch.isnan(inline[i]).all()
        else:
            assert torch.equal(inline[i], _fp(c))
    assert eng.calls == 7 and eng.vacuous is None       # five batches; the one with the refused clip is retried clip by clip
