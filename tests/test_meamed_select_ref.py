"""The selection route of the mean around the median and of Bulyan's second stage without a GPU: the
column rule of fjmeamedsel_dev.h built for the host against tests/around_median_ref.py, and the refusals."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import around_median_ref as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 3, 5, 64, 65, 129, 300, 1024]
P = 64


def cases_of(K):
    """[(beta, kind, x)]: every keep count of the list at every data kind, 64 columns each."""
    rng = np.random.RandomState(3000 + K)
    betas = sorted({b for b in (1, 2, (K + 1) // 2, K - 1, K) if 1 <= b <= K})
    return [(beta, kind, ref.DATA[kind](rng, K, P)) for beta in betas for kind in sorted(ref.DATA)]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = next((shutil.which(n) for n in ("c++", "g++", "clang++") if shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("meamed_select") / "meamed_select_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
           os.path.join(ROOT, "tests", "meamed_select_host.cpp"), "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        subprocess.run([c for c in cmd if "sanitize" not in c], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("K", KS)
def test_host_build_of_the_column_rule_is_the_restatement(host_program, tmp_path, K):
    cases = cases_of(K)
    blob = [struct.pack("<i", len(cases))]
    for beta, _, x in cases:
        blob += [struct.pack("<3iI", K, beta, P, int(ref.inverse(beta).view(np.uint32))), x.tobytes()]
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([host_program, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint32).reshape(len(cases), 2 + K, P)
    for (beta, kind, x), res in zip(cases, got):
        assert res[0].tolist() == ref.window_start_by_counts(x, beta).tolist(), (K, beta, kind, "count rule")
        assert res[0].tolist() == ref.window_start_greedy(x, beta).tolist(), (K, beta, kind, "greedy")
        assert np.array_equal(res[2:] != 0, ref.kept_mask_by_counts(x, beta)), (K, beta, kind)
        assert ref.canon(res[1].view(F32)).tolist() == ref.canon(ref.mean_around_median(x, beta)).tolist(), (K, beta, kind)


def test_the_cases_reach_the_edges():
    edge = {kind: 0 for kind in ref.DATA}
    nonfinite = dict(edge)
    for K in KS:
        for beta, kind, x in cases_of(K):
            edge[kind] += ref.edge_ties(x, beta)
            nonfinite[kind] += ref.nonfinite_medians(x)
    assert edge["ties"] > 0 and nonfinite["poisoned"] > 0, (edge, nonfinite)


@pytest.fixture()
def no_library(monkeypatch):
    """Any touch of libfjagg.so or the host helper fails the test."""
    from fedjax_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    for name in ("load", "call", "host", "upload", "check"):
        monkeypatch.setattr(_lib, name, boom)


def test_surface_refuses_before_the_library(no_library):
    from fedjax_amd import aggregators, kernels, tree_util
    from fedjax_amd.slab import ClientDeltaSlab

    def slab(K, dtype=torch.float32):
        s = object.__new__(ClientDeltaSlab)
        s.num_clients, s.dtype, s.num_params = K, dtype, 8
        return s

    assert kernels.MEAMED_SELECT_MAX_CLIENTS == 1024
    assert kernels.meamed_method("select") and not kernels.meamed_method("sort")
    trees = lambda K: [{"w": np.zeros(3, F32)}] * K
    for call in (lambda **kw: slab(8).mean_around_median(1, **kw), lambda **kw: slab(8).bulyan(1, **kw),
                 lambda **kw: tree_util.tree_mean_around_median(trees(8), 1, **kw),
                 lambda **kw: tree_util.tree_bulyan(trees(8), 1, **kw),
                 lambda **kw: aggregators.mean_around_median_aggregator(1, **kw),
                 lambda **kw: aggregators.bulyan_aggregator(1, **kw), lambda **kw: kernels.meamed_method(**kw)):
        with pytest.raises(ValueError, match="method must be"):
            call(method="radix")
    for call in (lambda: slab(1025).mean_around_median(1, method="select"),
                 lambda: tree_util.tree_mean_around_median(trees(1025), 1, method="select"),
                 lambda: kernels.meamed_select_dense(torch.zeros(1025, 2), 1),
                 lambda: kernels.meamed_select_dense(torch.zeros(1025, 2), 1, [0, 1]),
                 lambda: kernels.meamed_select_ptrs(torch.zeros(64, dtype=torch.int64), 1, 1025, 1, 1, None),
                 lambda: slab(1025).bulyan(1, method="select"),
                 lambda: tree_util.tree_bulyan(trees(1025), 1, method="select")):
        with pytest.raises(ValueError, match="1024"):
            call()
    for call in (lambda: slab(200).bulyan(10, select="device", method="select"),
                 lambda: tree_util.tree_bulyan(trees(200), 10, select="device", method="select"),
                 lambda: aggregators.bulyan_aggregator(10, select="device", method="select")):
        with pytest.raises(ValueError, match='select="host"'):
            call()
    with pytest.raises(ValueError, match="K - 2f <= 128"):  # the default method keeps its limit
        slab(200).bulyan(10)
    with pytest.raises(ValueError, match="4f"):
        slab(200).bulyan(50, method="select")
    with pytest.raises(ValueError, match="128"):
        slab(129).mean_around_median(1)
    x = torch.zeros(300, 8)
    with pytest.raises(ValueError, match=r"\[1, 300\]"):
        kernels.meamed_select_dense(x, 301)
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        slab(300).mean_around_median(3, rows=[0, 299], method="select")
    with pytest.raises(TypeError, match="int"):
        slab(300).mean_around_median(True, method="select")
    with pytest.raises(TypeError, match="float32"):
        slab(300, torch.bfloat16).mean_around_median(1, method="select")
    with pytest.raises(TypeError, match="float32"):
        kernels.meamed_select_dense(x.to(torch.bfloat16), 1)
    for rows in ([1, 1], [2, 1], [0, 300], [-1, 2]):
        with pytest.raises(ValueError, match="strictly ascending"):
            kernels.meamed_select_dense(x, 1, rows)
    with pytest.raises(ValueError, match="out must be"):
        kernels.meamed_select_dense(x, 1, out=torch.zeros(7))
    with pytest.raises(ValueError, match="device tensors"):
        kernels.meamed_select_dense(x, 150, list(range(0, 300, 2)))  # valid arguments, host tensor: no library call
    with pytest.raises(ValueError, match="bad plan"):
        kernels.meamed_select_ptrs(torch.zeros(64, dtype=torch.int64), 8, 300, 20, 1, None)


def test_c_entries_refuse_on_the_host():
    from fedjax_amd import _lib

    lib = _lib.load()
    err = lib.fjagg_last_error
    img = np.zeros(64, np.int64).ctypes.data

    def dense(M, keep, fl=0, dt=_lib.F32, K_rows=None, rows=16, ld=8, P=8, x=16):
        return lib.fjagg_meamed_select_dense(dt, x, ld, M if K_rows is None else K_rows, P, rows, M, keep, 1.0, 16, fl, None)

    def ptrs(M, keep, fl=0, dt=_lib.F32, nblk=1):
        return lib.fjagg_meamed_select_ptrs(dt, img, 1, M, nblk, keep, 1.0, fl, None)

    for entry in (dense, ptrs):
        assert entry(1025, 1) == -3 and b"1024" in err()
        assert entry(300, 0) == -1 and b"keep <= M" in err()
        assert entry(300, 301) == -1 and entry(0, 1) == -1 and entry(300, 1, dt=_lib.BF16) == -3
        assert entry(300, 1, _lib.ACCUMULATE) == -3 and entry(300, 1, 1 << 8) == -3
    assert dense(300, 1, _lib.UNALIGNED) == -3
    assert dense(10, 1, K_rows=1025) == -3 and dense(10, 1, K_rows=0) == -1 and dense(10, 1, K_rows=9) == -1
    assert dense(10, 1, K_rows=20, rows=None) == -1 and b"without a row table" in err()
    assert dense(10, 1, ld=7) == -1 and dense(10, 1, x=None) == -1
    assert dense(10, 1, ld=(1 << 28) + 1, P=(1 << 28) + 1) == -3 and b"1 GiB" in err()
    assert ptrs(300, 1, nblk=0) == -1 and b"bad plan" in err()
