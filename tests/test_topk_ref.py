"""The top-k sparsified mean without a GPU: the digit and scan rules of
fedjax_amd/csrc/fjsparse_dev.h built for the host and compared bit for bit with the numpy
restatement of tests/topk_ref.py (itself checked against a direct definition), the keep-count
table, every refusal of the Python surfaces and of the C entries, the new names, and the
unchanged ABI versions."""
import os
import re

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, aggregators, kernels, tree_util
from fedjax_amd.aggregators import compression
from fedjax_amd.slab import ClientDeltaSlab
from tests import topk_host
from tests import topk_ref as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------- the reference against the definition
def test_reference_threshold_mask_and_sent_by_hand():
    row = np.array([0.5, -2.0, 0.0, -0.0, 2.0, 1.0, -0.5], F32)
    assert ref.threshold(row, 1) == np.array(2.0, F32).view(np.uint32)
    assert ref.threshold(row, 2) == np.array(2.0, F32).view(np.uint32)  # the tie at the top
    assert ref.threshold(row, 3) == np.array(1.0, F32).view(np.uint32)
    assert ref.threshold(row, 6) == 0 and ref.threshold(row, 7) == 0
    T, sent = ref.select([row], 4)
    assert T[0] == np.array(0.5, F32).view(np.uint32) and sent[0] == 5  # both +-0.5 are kept
    kept = ref.mask_row(row, T[0])
    assert kept.view(np.uint32).tolist() == np.array([0.5, -2.0, 0.0, 0.0, 2.0, 1.0, -0.5], F32).view(np.uint32).tolist()
    T, sent = ref.select([row], 6)
    assert T[0] == 0 and sent[0] == 5  # zeros are never sent
    assert ref.mask_row(row, 0).view(np.uint32).tolist() == row.view(np.uint32).tolist()  # a kept -0 passes
    nan_row = np.array([1.0, np.nan, np.inf, -3.0], F32)
    assert ref.threshold(nan_row, 1) == (nan_row.view(np.uint32)[1] & 0x7FFFFFFF)  # a NaN is kept first
    assert ref.threshold(nan_row, 2) == 0x7F800000


def test_reference_mean_is_tree_mean_of_the_masked_rows():
    rng = np.random.RandomState(3)
    rows = list(ref.family("gauss", 4, 37, rng))
    w = [3, 0.5, 0, -2.0]
    mean, T, sent = ref.topk_mean_rows(rows, w, 5)
    s = None
    for r, t, wk in zip(rows, T, w):
        term = ref.mask_row(r, t) * F32(wk)
        s = term if s is None else (s + term).astype(F32)
    want = (s * F32(1.0 / 1.5)).astype(F32)
    assert mean.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert (sent >= 5).all()


# ----------------------------------------------------------- the device rules, built for the host
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = topk_host.compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    return topk_host.build_host_program(cxx, tmp_path_factory.mktemp("topk_select"))


_run_host = topk_host.run_host  # (moved to tests/topk_host.py, shared with tests/test_topk_cases.py)


def _check(exe, cases, tmp_path):
    got = _run_host(exe, cases, tmp_path)
    for i, ((row, c), (T, sent, trace)) in enumerate(zip(cases, got)):
        wT, wsent = ref.select([np.ascontiguousarray(row).view(F32).ravel()], c)
        assert (T, sent) == (int(wT[0]), int(wsent[0])), (i, c, hex(T), hex(int(wT[0])), sent, int(wsent[0]))
        assert trace[0] == T >> 20 and trace[2] == (T >> 10) & 1023 and trace[4] == T & 1023, (i, trace)
    return got


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_host_select_families(host_program, tmp_path, name):
    rng = np.random.RandomState(ref.FAMILIES.index(name))
    cases = []
    for P in (1, 2, 257, 1000):
        row = ref.family(name, 1, P, rng)[0]
        cases += [(row, c) for c in ref.keep_counts(P)]
    _check(host_program, cases, tmp_path)


def test_host_select_rank_on_a_bin_boundary(host_program, tmp_path):
    """The rank lands on the last element of a bin, and on the first of the next, at every level."""
    def row(shift):
        hi = (np.uint32(0x3F8) << 20) if shift != 20 else np.uint32(0)
        top = hi | (np.uint32(700) << shift)
        low = hi | (np.uint32(300) << shift)
        return np.concatenate([np.full(5, top, np.uint32), np.full(5, low, np.uint32), np.zeros(3, np.uint32)])
    cases = [(row(s), c) for s in (20, 10, 0) for c in (1, 4, 5, 6, 10, 11, 13)]
    got = _check(host_program, cases, tmp_path)
    by = {(s, c): g for (s, c), g in zip([(s, c) for s in (20, 10, 0) for c in (1, 4, 5, 6, 10, 11, 13)], got)}
    for s in (20, 10, 0):
        assert by[(s, 5)][0] == by[(s, 1)][0] != by[(s, 6)][0]
        assert by[(s, 5)][1] == 5 and by[(s, 6)][1] == 10 and by[(s, 11)][:2] == (0, 10)


def test_host_select_fewer_nonzeros_than_the_keep_count(host_program, tmp_path):
    row = np.zeros(50, F32)
    row[[3, 17, 40]] = [1.5, -2.5, 1e-40]
    got = _check(host_program, [(row, 10), (row, 3), (row, 4), (row, 50)], tmp_path)
    assert [g[:2] for g in got] == [(0, 3), (int(np.array(1e-40, F32).view(np.uint32)), 3), (0, 3), (0, 3)]


def test_host_select_every_key_equal_and_all_zero(host_program, tmp_path):
    eq = np.full(300, F32(-7.25))
    z = np.zeros(300, F32)
    z[::2] = -0.0
    got = _check(host_program, [(eq, 1), (eq, 150), (eq, 300), (z, 1), (z, 300)], tmp_path)
    assert [g[1] for g in got] == [300, 300, 300, 0, 0] and got[3][0] == 0


def test_header_constants_match_the_python_side():
    src = open(os.path.join(ROOT, "fedjax_amd", "csrc", "fjsparse_dev.h")).read()
    consts = dict(re.findall(r"constexpr int (k\w+) = (\d+);", src))
    assert int(consts["kChunk"]) == kernels.TOPK_CHUNK == _lib.TOPK_CHUNK
    assert int(consts["kMaxClients"]) == kernels.TOPK_MAX_CLIENTS == 4096
    assert int(consts["kMaxBins"]) == 2048 and int(consts["kLevels"]) == 3
    hdr = open(os.path.join(ROOT, "include", "fjcomp.h")).read()
    assert f"#define FJCOMP_TOPK_CHUNK {kernels.TOPK_CHUNK}" in hdr
    assert f"#define FJCOMP_TOPK_MAX_CLIENTS {kernels.TOPK_MAX_CLIENTS}" in hdr


# ----------------------------------------------------------- surfaces
def test_topk_count_table():
    tc = kernels.topk_count
    assert [tc(1, 1), tc(1, 10), tc(10, 10), tc(np.int64(3), 10)] == [1, 1, 10, 3]
    assert [tc(1.0, 10), tc(0.1, 10), tc(0.01, 10), tc(0.29, 100), tc(0.5, 7), tc(np.float32(0.5), 8)] == \
        [10, 1, 1, 28, 3, 4]
    assert tc(0.1, (1 << 31) - 1) == int(np.floor(0.1 * ((1 << 31) - 1)))
    assert tc((1 << 31) - 1, (1 << 31) - 1) == (1 << 31) - 1
    for bad in (True, False, np.bool_(True), "3", None, [1]):
        with pytest.raises(TypeError):
            tc(bad, 10)
    for bad, P, word in ((0, 10, "1 <= k <= P = 10"), (11, 10, "1 <= k <= P = 10"), (-1, 10, "1 <= k <= P"),
                         (0.0, 10, "(0, 1]"), (1.5, 10, "(0, 1]"), (-0.1, 10, "(0, 1]"), (float("nan"), 10, "(0, 1]"),
                         (1, 0, "at least 1"), (1, 1 << 31, "2^31")):
        with pytest.raises(ValueError) as e:
            tc(bad, P)
        assert word in str(e.value), (bad, P, str(e.value))


def test_kernel_wrappers_refuse_before_any_launch():
    x = torch.zeros(3, 8)
    w = torch.ones(3)
    for bad in (x.to(torch.bfloat16), x.to(torch.int32)):
        with pytest.raises(TypeError, match="float32"):
            kernels.topk_select_dense(bad, 1)
        with pytest.raises(TypeError, match="float32"):
            kernels.topk_mean_dense(bad, w, 1, scale=1.0)
    big = torch.zeros(4097, 2)
    with pytest.raises(ValueError, match="K <= 4096"):
        kernels.topk_select_dense(big, 1)
    with pytest.raises(ValueError, match="K <= 4096"):
        kernels.topk_mean_dense(big, torch.ones(4097), 1, scale=1.0)
    for c in (0, 9, -1):
        with pytest.raises(ValueError, match="1 <= k <= P = 8"):
            kernels.topk_select_dense(x, c)
        with pytest.raises(ValueError, match="1 <= k <= P = 8"):
            kernels.topk_mean_dense(x, w, c, scale=1.0)
    for c in (True, 0.5, "1"):
        with pytest.raises(TypeError):
            kernels.topk_select_dense(x, c)
    with pytest.raises(TypeError, match=r"shape \(3,\)"):
        kernels.topk_mean_dense(x, torch.ones(4), 1, scale=1.0)
    with pytest.raises(ValueError, match="unit column stride"):
        kernels.topk_select_dense(torch.zeros(8, 3).t(), 1)
    with pytest.raises(ValueError, match="device tensors"):  # everything else was in order: host deltas
        kernels.topk_select_dense(x, 1)
    with pytest.raises(ValueError, match="K <= 4096"):
        kernels.TopKTables(np.zeros((4097, 1), np.int64), [4])
    with pytest.raises(ValueError, match="need 2 weights"):
        kernels.TopKTables(np.zeros((2, 1), np.int64), [4], [0], np.ones(3, F32))


def test_topk_tables_layout():
    ptrs = np.array([[1024, 4096 + 4], [8192, 16384 + 4]], np.int64)
    t = kernels.TopKTables(ptrs, [kernels.TOPK_CHUNK + 1, 0], [256, 512], np.array([1.5, -2.0], F32))
    assert (t.K, t.L, t.P, t.nchunks) == (2, 2, kernels.TOPK_CHUNK + 1, 2)
    assert not t.unaligned  # the misaligned pointers belong to an empty leaf, which is never read
    assert t.host[:4].tolist() == ptrs.ravel().tolist() and t.host[4:6].tolist() == [256, 512]
    assert t.host[6:8].tolist() == [kernels.TOPK_CHUNK + 1, 0] and t.host[8:11].tolist() == [0, 2, 2]
    assert t.host[11:].view(F32)[:2].tolist() == [1.5, -2.0]
    assert kernels.TopKTables(ptrs, [3, 5]).unaligned


def test_slab_and_tree_surfaces_refuse_before_any_launch():
    cpu = torch.device("cpu")
    slab = ClientDeltaSlab({"a": np.zeros(5, F32), "b": np.zeros((2, 2), F32)}, 3, device=cpu)
    with pytest.raises(ValueError, match="need 3 weights"):
        slab.topk_mean([1, 2], 2)
    for bad, err in ((0, ValueError), (10, ValueError), (1.5, ValueError), (True, TypeError), ("2", TypeError)):
        with pytest.raises(err):
            slab.topk_mean([1, 1, 1], bad)
        with pytest.raises(err):
            slab.topk_thresholds(bad)
    with pytest.raises(TypeError, match="float32 slab"):
        ClientDeltaSlab({"a": np.zeros(5, F32)}, 3, dtype=torch.bfloat16, device=cpu).topk_mean([1, 1, 1], 2)
    with pytest.raises(TypeError, match="float32 slab"):
        ClientDeltaSlab({"a": np.zeros(5, F32)}, 3, dtype=torch.bfloat16, device=cpu).topk_thresholds(2)
    with pytest.raises(ValueError, match="K <= 4096"):
        ClientDeltaSlab({"a": np.zeros(1, F32)}, 4097, device=cpu).topk_thresholds(1)
    assert tree_util.tree_topk_mean([], 3) == tree_util.TopKMean(None, None, None)
    with pytest.raises(TypeError):
        aggregators.top_k_sparsifier(True)
    with pytest.raises(TypeError):
        aggregators.top_k_sparsifier("0.1")
    agg = aggregators.top_k_sparsifier(0.1)
    state = agg.init()
    assert isinstance(state, compression.SparsifierState) and state.num_bits == 0.0
    mean, state2 = agg.apply([], state)
    assert mean is None and state2.num_bits == 0.0  # an empty round


def test_c_entries_refuse_with_the_limit_in_the_message():
    lib = _lib.load()
    err = lambda: lib.fjagg_last_error().decode()
    ws = lib.fjcomp_topk_workspace_bytes(3)
    assert ws == 3 * (2048 + 2) * 4 and lib.fjcomp_topk_workspace_bytes(0) == 0
    sel = lambda dt, K, P, c, ws_bytes=1 << 30, x=16, ld=None: lib.fjcomp_topk_select_dense(
        dt, x, P if ld is None else ld, K, P, c, 16, 16, 16, ws_bytes, None)
    for dt in (_lib.BF16, _lib.I32):
        assert sel(dt, 3, 8, 1) == -3 and "float32" in err()
    assert sel(_lib.F32, 4097, 8, 1) == -3 and "4096" in err()
    assert sel(_lib.F32, 0, 8, 1) == -1 and "K must be" in err()
    assert sel(_lib.F32, 3, 1 << 31, 1) == -3 and "2^31" in err()
    assert sel(_lib.F32, 3, 8, 0) == -1 and "[1, P = 8]" in err()
    assert sel(_lib.F32, 3, 8, 9) == -1 and "[1, P = 8]" in err()
    assert sel(_lib.F32, 3, 8, 1, ws_bytes=ws - 1) == -1 and str(ws) in err()
    assert sel(_lib.F32, 3, 8, 1, ld=7) == -1 and "ld" in err()
    assert sel(_lib.F32, 3, 8, 1, x=None) == -1 and "null" in err()
    assert sel(_lib.F32, 3, 0, 1) == 0  # P = 0 launches nothing
    mean = lambda dt, K, P, c, w=16: lib.fjcomp_topk_mean_dense(dt, 16, P, K, P, c, w, 1.0, 16, 16, 16, 16, 1 << 30, None)
    assert mean(_lib.BF16, 3, 8, 1) == -3 and "float32" in err()
    assert mean(_lib.F32, 5000, 8, 1) == -3 and "4096" in err()
    assert mean(_lib.F32, 3, 8, 9) == -1 and "[1, P = 8]" in err()
    assert mean(_lib.F32, 3, 8, 1, w=None) == -1 and "null" in err()
    assert mean(_lib.F32, 3, 0, 1) == 0
    psel = lambda dt, K, L, nchunks, P, c, flags=0, tab=16: lib.fjcomp_topk_select_ptrs(
        dt, tab, K, L, tab, tab, nchunks, P, c, 16, 16, 16, 1 << 30, flags, None)
    assert psel(_lib.I32, 3, 2, 1, 8, 1) == -3 and "float32" in err()
    assert psel(_lib.F32, 4097, 2, 1, 8, 1) == -3 and "4096" in err()
    assert psel(_lib.F32, 3, 2, 1, 8, 9) == -1 and "[1, P = 8]" in err()
    assert psel(_lib.F32, 3, 0, 1, 8, 1) == -1 and "L must be" in err()
    assert psel(_lib.F32, 3, 2, 0, 8, 1) == -1 and "nchunks" in err()
    assert psel(_lib.F32, 3, 2, 4, 8, 1) == -1 and "nchunks" in err()
    assert psel(_lib.F32, 3, 2, 1, 8, 1, flags=_lib.NARROW) == -3 and "flags" in err()
    assert psel(_lib.F32, 3, 2, 1, 8, 1, tab=None) == -1 and "null" in err()
    pmean = lambda dt, K, c, outp=16: lib.fjcomp_topk_mean_ptrs(dt, 16, K, 2, 16, 16, 1, 8, c, 16, 1.0, outp, 16, 16, 16,
                                                                 1 << 30, 0, None)
    assert pmean(_lib.BF16, 3, 1) == -3 and "float32" in err()
    assert pmean(_lib.F32, 4097, 1) == -3 and "4096" in err()
    assert pmean(_lib.F32, 3, 0) == -1 and "[1, P = 8]" in err()
    assert pmean(_lib.F32, 3, 1, outp=None) == -1 and "null" in err()


def test_new_names_and_unchanged_abi_versions():
    for name in ("tree_topk_mean", "TopKMean"):
        assert name in tree_util.__all__ and hasattr(tree_util, name)
    for name in ("top_k_sparsifier", "SparsifierState"):
        assert name in compression.__all__ and hasattr(aggregators, name)
    for name in ("topk_count", "topk_select_dense", "topk_select_ptrs", "topk_mean_dense", "topk_mean_ptrs"):
        assert callable(getattr(kernels, name))
    assert callable(ClientDeltaSlab.topk_mean) and callable(ClientDeltaSlab.topk_thresholds)
    assert tree_util.TopKMean._fields == ("mean", "thresholds", "sent")
    lib = _lib.load()
    assert (lib.fjagg_abi_version(), lib.fjcomp_abi_version()) == (4, 1) == (_lib.ABI_VERSION, _lib.COMP_ABI_VERSION)
    assert "#define FJCOMP_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "fjcomp.h")).read()
    assert re.search(r"#define FJAGG_ABI_VERSION 4\b", open(os.path.join(ROOT, "include", "fjagg.h")).read())
    for sym in ("fjcomp_topk_workspace_bytes", "fjcomp_topk_select_dense", "fjcomp_topk_select_ptrs",
                "fjcomp_topk_mean_dense", "fjcomp_topk_mean_ptrs"):
        assert sym in _lib.SYMBOLS
