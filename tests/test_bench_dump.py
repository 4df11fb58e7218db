"""bench.py --dump-outputs on the host: one float64 DIR/<name>.npy per array, the whole dump
within its size cap (an array too large for it becomes a fixed every-k-th sample)."""
import os

import numpy as np

import bench


def test_dump_outputs_writes_float64_arrays(tmp_path):
    x = np.arange(10, dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), {"x": x, "niter": 7.0, "hits_boundary": False})
    assert sorted(os.listdir(tmp_path / "out")) == ["hits_boundary.npy", "niter.npy", "x.npy"]
    got = np.load(tmp_path / "out" / "x.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x)
    assert float(np.load(tmp_path / "out" / "niter.npy")) == 7.0
    assert float(np.load(tmp_path / "out" / "hits_boundary.npy")) == 0.0


def test_dump_outputs_samples_what_exceeds_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 1000 + 8)
    x = np.arange(4500, dtype=np.float64)
    for run in range(2):
        bench.dump_outputs(str(tmp_path / str(run)), {"x": x, "niter": 3.0})
    a, b = (np.load(tmp_path / str(run) / "x.npy") for run in range(2))
    assert a.size <= 1000 and np.array_equal(a, b)
    assert np.array_equal(a, x[::5])
    total = sum(os.path.getsize(tmp_path / "0" / f) for f in os.listdir(tmp_path / "0"))
    assert total <= bench.DUMP_BYTES + 2 * 128      # (+ one .npy header per file)
