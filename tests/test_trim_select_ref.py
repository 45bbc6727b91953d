"""The selection route of the trimmed mean and median without a GPU: the column rule of
fjtrimsel_dev.h built for the host against tests/robust_mean_ref.py, and the refusals of every surface."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import robust_mean_ref as ref
from tests.trim_select_cases import families, trims

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = next((shutil.which(n) for n in ("c++", "g++", "clang++") if shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("trim_select") / "trim_select_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
           os.path.join(ROOT, "tests", "trim_select_host.cpp"), "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        subprocess.run([c for c in cmd if "sanitize" not in c], check=True, capture_output=True)
    return exe


def test_host_build_of_the_column_rule_is_the_restatement(host_program, tmp_path):
    rng = np.random.RandomState(77)
    P, cases = 12, []
    for K in [1, 2, 3, 64, 65, 129, 257, 1000, 1024] + rng.randint(1, 1025, 4).tolist():
        cases += [(K, t, ref.mixed_data(rng, K, P)) for t in trims(K) + [int(rng.randint(0, (K - 1) // 2 + 1))]]
    for K in (257, 1024):
        cases += [(K, t, x) for x in families(K, P).values() for t in trims(K)]
    blob = [struct.pack("<i", len(cases))]
    for K, t, x in cases:
        blob += [struct.pack("<3iI", K, t, P, int(ref.inverse(K - 2 * t).view(np.uint32))), x.astype(F32).tobytes()]
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([host_program, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got, at = np.frombuffer(dst.read_bytes(), dtype=np.uint32), 0
    for K, t, x in cases:
        y, mask = got[at:at + P], got[at + P:at + P + K * P].reshape(K, P)
        at += P + K * P
        assert np.array_equal(mask != 0, ref.kept_mask_by_counts(x, t)), (K, t)
        assert ref.canon(y.view(F32)).tolist() == ref.canon(ref.trimmed_mean(x, t)).tolist(), (K, t)


def test_surface_refuses_before_the_library(monkeypatch):
    from fedjax_amd import _lib, aggregators, kernels, tree_util
    from fedjax_amd.slab import ClientDeltaSlab

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    for name in ("load", "call", "host", "upload", "check"):
        monkeypatch.setattr(_lib, name, boom)

    def slab(K):
        s = object.__new__(ClientDeltaSlab)
        s.num_clients, s.dtype, s.num_params = K, torch.float32, 8
        return s

    assert kernels.TRIM_SELECT_MAX_CLIENTS == 1024 and kernels.TRIM_MAX_CLIENTS == 128
    trees = lambda K: [{"w": np.zeros(3, F32)}] * K
    calls = [lambda K, **kw: slab(K).trimmed_mean(0, **kw), lambda K, **kw: slab(K).median(**kw),
             lambda K, **kw: tree_util.tree_trimmed_mean(trees(K), 0, **kw),
             lambda K, **kw: tree_util.tree_median(trees(K), **kw),
             lambda K, **kw: aggregators.trimmed_mean_aggregator(0.1, **kw),
             lambda K, **kw: aggregators.median_aggregator(**kw)]
    for call in calls:
        with pytest.raises(ValueError, match="method must be"):
            call(8, method="radix")
        with pytest.raises(ValueError, match="bucket_size"):
            call(8, method="select", bucket_size=2)
    for call in calls[:4]:
        with pytest.raises(ValueError, match="1024"):
            call(1025, method="select")


def test_c_entries_refuse_on_the_host():
    from fedjax_amd import _lib

    lib = _lib.load()
    err = lib.fjagg_last_error
    img = np.zeros(64, np.int64).ctypes.data
    dense = lambda K, t, fl=0, dt=_lib.F32: lib.fjagg_trim_select_dense(dt, 16, 8, K, 8, t, 1.0, 16, fl, None)
    ptrs = lambda K, t, fl=0, dt=_lib.F32: lib.fjagg_trim_select_ptrs(dt, img, 1, K, 1, t, 1.0, fl, None)
    for entry in (dense, ptrs):
        assert entry(1025, 0) == -3 and b"K <= 1024" in err()
        assert entry(1024, 512) == -1 and b"2t < K" in err()
        assert entry(129, -1) == -1 and entry(0, 0) == -1 and entry(200, 0, dt=_lib.BF16) == -3
        assert entry(200, 0, _lib.ACCUMULATE) == -3 and entry(200, 0, 1 << 8) == -3
