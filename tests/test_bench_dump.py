"""bench.py --dump-outputs, the writer itself (CPU): float32 .npy files, at most DUMP_LIMIT_BYTES in all, a seeded row sample beyond
that.  The flag on the timed path is run on the GPU in tests/test_gpu_bench_path.py."""
import os

import numpy as np
import torch

import bench


def _written(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_outputs_below_the_limit_are_written_whole_as_float32(tmp_path):
    x = torch.randn(32, 19779, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(str(tmp_path), {"clip_vectors": x})
    got = np.load(tmp_path / "clip_vectors.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert os.listdir(tmp_path) == ["clip_vectors.npy"]


def test_outputs_above_the_limit_are_a_seeded_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    x = torch.arange(1000 * 700, dtype=torch.float32).reshape(1000, 700)        # 2.8 MB
    y = torch.ones(300, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "y": y})
        assert _written(tmp_path / d) <= bench.DUMP_LIMIT_BYTES
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert np.array_equal(a, b) and 0 < a.shape[0] < 1000 and a.shape[1] == 700
    rows = a[:, 0].astype(np.int64) // 700
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, x.numpy()[rows])   # whole rows, in order, as computed
    assert 0 < np.load(tmp_path / "a" / "y.npy").shape[0] < 300
