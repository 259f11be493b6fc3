"""bench.py --dump-outputs: the writer of the last step's results (host side, no GPU)."""

import os

import numpy as np
import torch

import bench


def _dump(tmp_path, name, arrays):
    path = tmp_path / name
    bench.dump_outputs(str(path), arrays)
    return {f: np.load(path / f) for f in sorted(os.listdir(path))}, \
        sum(os.path.getsize(path / f) for f in os.listdir(path))


def test_arrays_within_the_limit_are_written_whole(tmp_path):
    f = torch.arange(1000, dtype=torch.float32) * 0.5
    got, _ = _dump(tmp_path, "a", {"model_f32": f, "model_i64_entries": torch.empty(0)})
    assert sorted(got) == ["model_f32.npy", "model_i64_entries.npy"]
    assert got["model_f32.npy"].dtype == np.float32 and got["model_f32.npy"].tobytes() == f.numpy().tobytes()
    assert got["model_i64_entries.npy"].shape == (0,)


def test_larger_arrays_are_cut_to_a_fixed_sample_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100_000)
    f = torch.arange(70_001, dtype=torch.float32)  # 280 KB: over the limit, an odd length
    i = torch.arange(33, dtype=torch.float32)
    a, size_a = _dump(tmp_path, "a", {"model_f32": f, "model_i64_entries": i})
    b, _ = _dump(tmp_path, "b", {"model_f32": f.clone(), "model_i64_entries": i.clone()})
    assert size_a <= 100_000
    for name in a:  # the same positions in every run
        assert a[name].dtype == np.float32 and a[name].tobytes() == b[name].tobytes()
    s = a["model_f32.npy"]
    assert 20_000 < s.size < 70_001 and (np.diff(s) >= 0).all() and s.max() <= 70_000  # values are positions here
    # the sample follows the data: another result at the same positions
    c, _ = _dump(tmp_path, "c", {"model_f32": f + 1, "model_i64_entries": i})
    assert np.array_equal(c["model_f32.npy"], s + 1)
