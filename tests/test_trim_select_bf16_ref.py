"""The bfloat16 selection route of the trimmed mean and median without a GPU: what every surface
still refuses before the library is touched, and the host-side refusals of the two C entries."""
import numpy as np
import pytest
import torch


def test_surface_refuses_before_the_library(monkeypatch):
    from fedjax_amd import _lib, tree_util
    from fedjax_amd.slab import ClientDeltaSlab

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    for name in ("load", "call", "host", "upload", "check"):
        monkeypatch.setattr(_lib, name, boom)

    def slab(K):
        s = object.__new__(ClientDeltaSlab)
        s.num_clients, s.dtype, s.num_params = K, torch.bfloat16, 8
        return s

    leaf = lambda dt: torch.zeros(3, dtype=dt)
    trees = lambda K, dts=(torch.bfloat16,): [{f"l{i}": leaf(dt) for i, dt in enumerate(dts)}] * K
    calls = [lambda K, **kw: slab(K).trimmed_mean(0, **kw), lambda K, **kw: slab(K).median(**kw),
             lambda K, **kw: tree_util.tree_trimmed_mean(trees(K), 0, **kw),
             lambda K, **kw: tree_util.tree_median(trees(K), **kw)]
    for call in calls:
        for kw in ({}, {"method": "sort"}, {"bucket_size": 2}):
            with pytest.raises(TypeError, match="float32"):
                call(8, **kw)
        with pytest.raises(ValueError, match="1024"):
            call(1025, method="select")
    for dts in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.int32), (torch.float16,)):
        with pytest.raises(TypeError):
            tree_util.tree_trimmed_mean(trees(8, dts), 0, method="select")
        with pytest.raises(TypeError):
            tree_util.tree_median(trees(8, dts), method="select")


def test_c_entries_refuse_on_the_host():
    from fedjax_amd import _lib

    lib = _lib.load()
    err = lib.fjagg_last_error
    img = np.zeros(64, np.int64).ctypes.data
    dense = lambda K, t, fl=0, dt=_lib.BF16: lib.fjagg_trim_select16_dense(dt, 16, 8, K, 8, t, 1.0, 16, fl, None)
    ptrs = lambda K, t, fl=0, dt=_lib.BF16, nblk=1: lib.fjagg_trim_select16_ptrs(dt, img, 1, K, nblk, t, 1.0, fl, None)
    for entry in (dense, ptrs):
        assert entry(200, 0, dt=_lib.F32) == -3 and b"bfloat16" in err()
        assert entry(1025, 0) == -3 and b"K <= 1024" in err()
        assert entry(200, 0, _lib.ACCUMULATE) == -3 and entry(200, 0, 1 << 8) == -3
        assert entry(1024, 512) == -1 and b"2t < K" in err()
        assert entry(0, 0) == -1
    assert ptrs(200, 0, nblk=0) == -1 and b"bad plan" in err()
    assert lib.fjagg_trim_select16_dense(_lib.BF16, 16, 4, 200, 8, 0, 1.0, 16, 0, None) == -1  # ld < P
