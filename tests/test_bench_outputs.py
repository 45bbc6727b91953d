"""bench.dump_outputs, the writer behind ``bench.py --dump-outputs`` (CPU): small arrays are
written whole in float32, a large one as the same seeded sample in every run, and the files
stay within the byte budget."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4 * (1000 + 64))  # two files of 1000 float32 each
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4).to(torch.bfloat16)
    large = torch.arange(5000, dtype=torch.float32) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", small), ("large", large)])
    s, l = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "large.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, np.arange(12).reshape(3, 4))
    assert l.dtype == np.float32 and l.ndim == 1 and 500 < l.size <= 1000
    assert np.all(np.diff(l) > 0) and np.all(np.isin(l, large.numpy()))  # distinct elements, in order
    assert np.array_equal(l, np.load(tmp_path / "b" / "large.npy"))  # the same sample every run
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES
