"""The numpy restatement of the mean around the median (tests/around_median_ref.py) pinned
against itself (greedy == count rule, the window property, the keep = K / keep = 1
consequences, a hand-worked tie); the device routine of fjrobust_dev.h built for the host and
compared with it bitwise; and the product's host surface: every refusal before the library is
touched and at the C entries, the aggregators, the symbols. No GPU needed."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import around_median_ref as ref
from tests import robust_mean_ref as trim_ref

F32 = np.float32
KS = [1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 64, 65, 100, 127, 128]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def betas(K, rng):
    return sorted({1, min(2, K), max(K // 2, 1), max(K - 1, 1), K, int(rng.randint(1, K + 1))})


# ------------------------------------------------------------------ the restatement pins itself
@pytest.mark.parametrize("K", KS)
def test_count_rule_is_the_greedy(K):
    rng = np.random.RandomState(300 + K)
    for kind in ("normal", "ties", "specials"):
        x = ref.DATA[kind](rng, K, 60)
        for beta in betas(K, rng):
            assert ref.window_start_by_counts(x, beta).tolist() == ref.window_start_greedy(x, beta).tolist(), (kind, beta)
            assert np.array_equal(ref.kept_mask(x, beta), ref.kept_mask_by_counts(x, beta)), (kind, beta)
            assert ref.kept_mask(x, beta).sum(0).tolist() == [beta] * 60
            assert ref.bits(ref.mean_around_median(x, beta)) == ref.bits(ref.mean_around_median(x, beta, ref.kept_mask))


@pytest.mark.parametrize("K", KS)
def test_window_holds_the_closest(K):
    """max d inside the window <= min d outside it."""
    rng = np.random.RandomState(400 + K)
    for kind in ("normal", "ties", "specials"):
        x = ref.DATA[kind](rng, K, 60)
        d = ref.distances(np.sort(ref.keys(x), axis=0))
        mid = (K - 1) // 2
        assert (d[1:mid + 1] <= d[:mid]).all() and (d[mid + 1:] >= d[mid:-1]).all()  # falls to mid, rises after
        for beta in betas(K, rng):
            a = ref.window_start_by_counts(x, beta)
            pos = np.arange(K)[:, None]
            inside = (pos >= a[None, :]) & (pos < a[None, :] + beta)
            assert inside[(K - 1) // 2].all()
            worst_in = np.where(inside, d, F32(0)).max(0)
            best_out = np.where(inside, F32(np.inf), d).min(0)
            assert (worst_in <= best_out).all(), (kind, beta)


@pytest.mark.parametrize("K", KS)
def test_keep_all_keep_one_and_the_median(K):
    rng = np.random.RandomState(500 + K)
    x = ref.specials(rng, K, 80)
    assert ref.bits(ref.mean_around_median(x, K)) == ref.bits(trim_ref.trimmed_mean(x, 0))
    srt = np.sort(ref.keys(x), axis=0)
    # verbatim up to the quieting of a signalling NaN by the multiplication with f32(1)
    assert ref.canon(ref.mean_around_median(x, 1)).tolist() == ref.canon(ref.values_of(srt[(K - 1) // 2])).tolist()
    finite = np.isfinite(ref.values_of(srt[(K - 1) // 2]))
    assert np.array_equal(ref.mean_around_median(x, 1).view(np.uint32)[finite],
                          ref.values_of(srt[(K - 1) // 2]).view(np.uint32)[finite])
    if K % 2:
        assert ref.bits(ref.mean_around_median(x, 1)) == ref.bits(trim_ref.median(x))


def test_hand_worked_tie():
    """K = 5, values [3, 1, 2, 1, 0]. Sorted by (key, client): 0(c4) 1(c1) 1(c3) 2(c2) 3(c0); mid = 2,
    med = 1 (client 3's). d = [1, 0, 0, 1, 2]."""
    x = np.array([[3], [1], [2], [1], [0]], F32)
    col = lambda *kept: [[k in kept] for k in range(5)]
    # beta = 2: from {2}, the sides are d[1] = 0 and d[3] = 1: the lower. Positions 1..2: clients 1, 3.
    assert ref.kept_mask(x, 2).tolist() == col(1, 3) == ref.kept_mask_by_counts(x, 2).tolist()
    # beta = 3: then d[0] = 1 against d[3] = 1, a tie: the lower side. Positions 0..2: clients 4, 1, 3.
    assert ref.kept_mask(x, 3).tolist() == col(4, 1, 3) == ref.kept_mask_by_counts(x, 3).tolist()
    assert ref.mean_around_median(x, 3).tolist() == [F32(F32(2) * F32(1.0 / 3.0))]
    # beta = 4: positions 0..3, client 0 (d = 2) stays out
    assert ref.kept_mask(x, 4).tolist() == col(1, 2, 3, 4)
    """The window's edge inside a run of equal keys: [1, 1, 1, 1, 5, 0], sorted 0(c5) 1(c0) 1(c1) 1(c2)
    1(c3) 5(c4), mid = 2 (client 1's 1). beta = 2: d = [1, 0, 0, 0, 0, 4]; d[1] = d[3] = 0, a tie: lower.
    Positions 1..2 hold the first two 1s in client order: clients 0 and 1, not 2 and 3."""
    y = np.array([[1], [1], [1], [1], [5], [0]], F32)
    want = [[True], [True], [False], [False], [False], [False]]
    assert ref.kept_mask(y, 2).tolist() == want == ref.kept_mask_by_counts(y, 2).tolist()
    # signed zeros are different keys at distance 0: [-0, +0, +0], mid = 1 is client 1's +0; beta = 2
    # compares d[0] = |-0 - +0| = 0 with d[2] = 0 (the same key): a tie, the lower side, clients 0 and 1
    z = np.array([[-0.0], [0.0], [0.0]], F32)
    assert ref.kept_mask(z, 2).ravel().tolist() == [True, True, False]
    assert ref.bits(ref.mean_around_median(z, 1)) == [0]


def test_nonfinite_medians_and_distances():
    nan, inf = F32(np.nan), F32(np.inf)
    # the median is +inf; +inf (same key) is at distance 0, the finite value and the NaN at +inf
    x = np.array([[1.0], [inf], [inf], [nan], [inf]], F32)  # sorted: 1 inf inf inf nan, mid = 2
    d = ref.distances(np.sort(ref.keys(x), axis=0)).ravel().tolist()
    assert d == [np.inf, 0, 0, 0, np.inf]
    assert ref.kept_mask(x, 3).ravel().tolist() == [False, True, True, False, True]
    assert ref.kept_mask(x, 4).ravel().tolist() == [True, True, True, False, True]  # the tie keeps the lower side
    # 1e30 against -1e30 is finite in float32; 3e38 against -3e38 overflows to +inf, which is a distance
    y = np.array([[-3e38], [0.0], [3e38]], F32)
    assert ref.distances(np.sort(ref.keys(y), axis=0)).ravel().tolist() == [F32(3e38), 0, F32(3e38)]
    assert ref.nonfinite_medians(x) == 1 and ref.nonfinite_medians(y) == 0


def test_fuzz_cases_cover_the_ground():
    cases = ref.fuzz_cases()
    assert len(cases) == 60 and ref.fuzz_cases() == cases  # seeded
    widths, edge, nonfinite = set(), 0, 0
    for agg, K, arg, leaves, kind, seed in cases:
        assert sum(leaves) >= 1
        if agg == "bulyan":
            assert K >= 4 * arg + 3 and K - 2 * arg <= 128
            widths.add(ref.width_of(K - 2 * arg))
            continue
        assert 1 <= arg <= K <= 128
        widths.add(ref.width_of(K))
        x = ref.DATA[kind](np.random.RandomState(seed), K, sum(leaves))
        edge += ref.edge_ties(x, arg) > 0
        nonfinite += ref.nonfinite_medians(x) > 0
    assert widths == {16, 32, 64, 128}
    assert edge >= 10 and nonfinite >= 5
    assert sum(c[0] == "bulyan" for c in cases) >= 15


# ----------------------------------------------------------- the device routine, built for the host
def _compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return shutil.which("clang++", path="/opt/rocm/llvm/bin")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("around_median") / "around_median_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
           os.path.join(ROOT, "tests", "around_median_host.cpp"), "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        cmd = [c for c in cmd if "sanitize" not in c]
        subprocess.run(cmd, check=True, capture_output=True)
    return exe


def _run_host(exe, cases, tmp_path):
    """cases: (mode, K, arg, x [K, P]). Returns per case {N: uint32 [P]}."""
    blob = [struct.pack("<i", len(cases))]
    for mode, K, arg, x in cases:
        scale = trim_ref.inverse(arg if mode == 0 else K - 2 * arg)
        blob.append(struct.pack("<4iI", mode, K, arg, x.shape[1], int(np.array([scale], F32).view(np.uint32)[0])))
        blob.append(np.ascontiguousarray(x, dtype=F32).tobytes())
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint32)
    out, at = [], 0
    for mode, K, arg, x in cases:
        P = x.shape[1]
        per = {}
        for N in (16, 32, 64, 128):
            if K <= N:
                per[N] = got[at:at + P]
                at += P
        out.append(per)
    assert at == got.size
    return out


def test_host_build_of_the_device_routine_is_the_restatement(host_program, tmp_path):
    rng = np.random.RandomState(77)
    cases = []
    for K in KS:
        for kind in ("normal", "ties", "specials"):
            x = ref.DATA[kind](rng, K, 48)
            for beta in betas(K, rng):
                cases.append((0, K, beta, x))
        x = ref.specials(rng, K, 48)
        for t in sorted({0, (K - 1) // 4, (K - 1) // 2}):  # the trimmed mean shares the sort and the sum
            cases.append((1, K, t, x))
    got = _run_host(host_program, cases, tmp_path)
    widths = set()
    for (mode, K, arg, x), per in zip(cases, got):
        want = ref.mean_around_median(x, arg) if mode == 0 else trim_ref.trimmed_mean(x, arg)
        for N, y in per.items():
            widths.add(N)
            assert ref.canon(y.view(F32)).tolist() == ref.canon(want).tolist(), (mode, K, arg, N)
    assert widths == {16, 32, 64, 128}


# ------------------------------------------------------------------------- the product's surface
@pytest.fixture()
def no_library(monkeypatch):
    """Any touch of libfjagg.so or the host helper fails the test."""
    from fedjax_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched")

    for name in ("load", "call", "host", "upload", "check"):
        monkeypatch.setattr(_lib, name, boom)


def _fake_slab(K, dtype=torch.float32):
    from fedjax_amd.slab import ClientDeltaSlab

    s = object.__new__(ClientDeltaSlab)
    s.num_clients, s.dtype, s.num_params = K, dtype, 8
    return s


def test_keep_count(no_library):
    from fedjax_amd import kernels

    assert kernels.keep_count(1, 1) == 1 and kernels.keep_count(np.int64(5), 128) == 5
    assert kernels.keep_count(128, 128) == 128
    for bad in (True, False, np.bool_(True), 0.5, 2.0, "3", None):
        with pytest.raises(TypeError):
            kernels.keep_count(bad, 10)
    for bad in (0, -1, 11):
        with pytest.raises(ValueError, match=r"\[1, 10\]"):
            kernels.keep_count(bad, 10)
    with pytest.raises(ValueError, match="128"):
        kernels.keep_count(1, 129)
    with pytest.raises(ValueError, match="at least 1"):
        kernels.keep_count(1, 0)


def test_kernel_wrappers_refuse_before_the_library(no_library):
    from fedjax_amd import kernels

    x = torch.zeros(4, 8)
    with pytest.raises(TypeError, match="float32"):
        kernels.meamed_dense(x.to(torch.bfloat16), 1)
    with pytest.raises(TypeError, match="float32"):
        kernels.meamed_dense(x.to(torch.int32), 1)
    with pytest.raises(ValueError, match="128"):
        kernels.meamed_dense(torch.zeros(129, 2), 1)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        kernels.meamed_dense(x, 5)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        kernels.meamed_dense(x, 0)
    with pytest.raises(TypeError):
        kernels.meamed_dense(x, True)
    with pytest.raises(TypeError):
        kernels.meamed_dense(x, 2.0)
    with pytest.raises(ValueError, match="unit column stride"):
        kernels.meamed_dense(torch.zeros(4, 16)[:, ::2], 1)
    with pytest.raises(ValueError, match="column"):
        kernels.meamed_dense(torch.zeros(4, 0), 1)
    with pytest.raises(ValueError, match="out must be"):
        kernels.meamed_dense(x, 1, out=torch.zeros(7))
    with pytest.raises(ValueError, match="device tensors"):
        kernels.meamed_dense(x, 1)  # valid arguments, host tensor: still no library call
    # row tables
    for rows in ([1, 1], [2, 1], [0, 4], [-1, 2]):
        with pytest.raises(ValueError, match="strictly ascending"):
            kernels.meamed_dense(x, 1, rows)
    with pytest.raises(ValueError, match="128"):
        kernels.meamed_dense(torch.zeros(200, 2), 1, list(range(129)))
    with pytest.raises(ValueError, match="128"):
        kernels.meamed_dense(x, 1, [])
    with pytest.raises(ValueError, match="1024"):
        kernels.meamed_dense(torch.zeros(1025, 2), 1, [0, 1])
    with pytest.raises(TypeError, match="int"):
        kernels.meamed_dense(x, 1, [0.0, 1.0])
    with pytest.raises(TypeError, match="int"):
        kernels.meamed_dense(x, 1, [True, False])
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        kernels.meamed_dense(x, 3, [0, 2])  # keep is counted against the table, not the slab
    with pytest.raises(ValueError, match="device tensors"):
        kernels.meamed_dense(torch.zeros(200, 8), 3, [0, 150, 199])
    img = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError, match="128"):
        kernels.meamed_ptrs(img, 1, 129, 1, 1, None)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        kernels.meamed_ptrs(img, 1, 4, 1, 5, None)
    with pytest.raises(TypeError):
        kernels.meamed_ptrs(img, 1, 4, 1, False, None)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.meamed_ptrs(img, 0, 4, 1, 1, None)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.meamed_ptrs(img, 8, 4, 20, 1, None)  # the image is shorter than the plan says
    with pytest.raises(TypeError):
        kernels.meamed_ptrs(img.to(torch.int32), 1, 4, 1, 1, None)


def test_slab_and_tree_refuse_before_the_library(no_library):
    from fedjax_amd import tree_util

    with pytest.raises(TypeError, match="float32"):
        _fake_slab(4, torch.bfloat16).mean_around_median(1)
    with pytest.raises(TypeError, match="float32"):
        _fake_slab(4, torch.int32).mean_around_median(1)
    with pytest.raises(ValueError, match="128"):
        _fake_slab(129).mean_around_median(1)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        _fake_slab(4).mean_around_median(5)
    with pytest.raises(TypeError, match="int"):
        _fake_slab(4).mean_around_median(True)
    with pytest.raises(ValueError, match="strictly ascending"):
        _fake_slab(4).mean_around_median(1, rows=[0, 4])
    with pytest.raises(ValueError, match="1024"):
        _fake_slab(1025).mean_around_median(1, rows=[0, 1])
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        _fake_slab(200).mean_around_median(3, rows=[0, 199])

    trees = [{"w": np.zeros(3, F32)} for _ in range(4)]
    assert tree_util.tree_mean_around_median([], 1) is None and tree_util.tree_mean_around_median(iter([]), 0) is None
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        tree_util.tree_mean_around_median(trees, 5)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        tree_util.tree_mean_around_median(iter(trees), 0)
    with pytest.raises(TypeError, match="int"):
        tree_util.tree_mean_around_median(trees, True)
    with pytest.raises(ValueError, match="128"):
        tree_util.tree_mean_around_median([{"w": np.zeros(1, F32)}] * 129, 1)
    for bad in (torch.zeros(3, dtype=torch.bfloat16), np.zeros(3, np.int32)):
        with pytest.raises(TypeError, match="float32"):
            tree_util.tree_mean_around_median([{"w": bad}] * 4, 1)


def test_c_entries_refuse_on_the_host():
    """The same refusals in the C entry points, with nothing launched (no GPU here)."""
    from fedjax_amd import _lib

    lib = _lib.load()
    ident = np.arange(128, dtype=np.int32)

    def dense(dt, ld, K_rows, P, M, keep, fl, rows=None, x=16, y=16):
        return lib.fjagg_meamed_dense(dt, x, ld, K_rows, P, None if rows is None else rows.ctypes.data, M, keep, 1.0, y,
                                      fl, None)

    assert dense(_lib.F32, 8, 200, 8, 129, 1, 0, np.arange(129, dtype=np.int32)) == -3 and b"128" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 4, 8, 0, 1, 0) == -1
    assert dense(_lib.F32, 8, 4, 8, 4, 5, 0) == -1 and b"keep <= M" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 4, 8, 4, 0, 0) == -1
    assert dense(_lib.F32, 8, 4, 8, 4, -1, 0) == -1
    assert dense(_lib.BF16, 8, 4, 8, 4, 1, 0) == -3 and b"float32" in lib.fjagg_last_error()
    assert dense(_lib.I32, 8, 4, 8, 4, 1, 0) == -3
    assert dense(_lib.F32, 8, 4, 8, 4, 1, 0, x=None) == -1 and b"null" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 4, 8, 4, 1, 0, y=None) == -1
    assert dense(_lib.F32, 8, 4, 0, 4, 1, 0) == -1
    assert dense(_lib.F32, 7, 4, 8, 4, 1, 0) == -1 and b"ld" in lib.fjagg_last_error()
    assert dense(_lib.F32, 1 << 29, 4, (1 << 28) + 1, 4, 1, 0) == -3 and b"1 GiB" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 1025, 8, 4, 1, 0, ident) == -3 and b"1024" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 0, 8, 4, 1, 0, ident) == -1
    assert dense(_lib.F32, 8, 3, 8, 4, 1, 0) == -1 and b"K_rows" in lib.fjagg_last_error()  # identity needs M rows
    for rows in ([0, 1, 1, 2], [0, 2, 1, 3], [0, 1, 2, 9], [-1, 0, 1, 2]):
        assert dense(_lib.F32, 8, 9, 8, 4, 1, 0, np.array(rows, np.int32)) == -1, rows
        assert b"strictly ascending" in lib.fjagg_last_error()
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, _lib.UNALIGNED,
               1 << 8, 1 << 16):
        assert dense(_lib.F32, 8, 4, 8, 4, 1, fl) == -3, fl
    img = np.zeros(64, np.int64)
    ptrs = lambda dt, L, K, nblk, keep, fl, im=img.ctypes.data: lib.fjagg_meamed_ptrs(dt, im, L, K, nblk, keep, 1.0, fl,
                                                                                       None)
    assert ptrs(_lib.F32, 1, 129, 1, 1, 0) == -3 and b"128" in lib.fjagg_last_error()
    assert ptrs(_lib.F32, 1, 0, 1, 1, 0) == -1
    assert ptrs(_lib.F32, 1, 4, 1, 5, 0) == -1 and b"keep <= M" in lib.fjagg_last_error()
    assert ptrs(_lib.F32, 1, 4, 1, 0, 0) == -1
    assert ptrs(_lib.BF16, 1, 4, 1, 1, 0) == -3
    assert ptrs(_lib.F32, 0, 4, 1, 1, 0) == -1 and b"bad plan" in lib.fjagg_last_error()
    assert ptrs(_lib.F32, 1, 4, 0, 1, 0) == -1
    assert ptrs(_lib.F32, 1, 4, 1, 1, 0, im=None) == -1
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, 1 << 8):
        assert ptrs(_lib.F32, 1, 4, 1, 1, fl) == -3, fl


def test_aggregator_state_and_exports():
    import fedjax_amd
    from fedjax_amd import aggregators, slab, tree_util

    assert hasattr(aggregators, "mean_around_median_aggregator")
    agg = aggregators.mean_around_median_aggregator(3)
    assert isinstance(agg, aggregators.Aggregator)
    state = agg.init()
    assert isinstance(state, aggregators.RobustAggregatorState) and fedjax_amd.pytree.leaves_of(state) == []
    got, state2 = agg.apply(iter([]), state)  # no clients: None, the state unchanged
    assert got is None and state2 is state
    for bad in (True, 0.5, "x", None):
        with pytest.raises(TypeError):
            aggregators.mean_around_median_aggregator(bad)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            aggregators.mean_around_median_aggregator(bad)
    assert "tree_mean_around_median" in tree_util.__all__ and callable(tree_util.tree_mean_around_median)
    assert callable(slab.ClientDeltaSlab.mean_around_median)
    assert "no weights" in slab.ClientDeltaSlab.mean_around_median.__doc__.lower()
    assert "ignores the weights" in aggregators.mean_around_median_aggregator.__doc__.lower()


def test_symbols_and_abi():
    from fedjax_amd import _lib, kernels

    assert _lib.ABI_VERSION == 4
    for sym in ("fjagg_meamed_dense", "fjagg_meamed_ptrs"):
        assert sym in _lib.SYMBOLS
    assert callable(kernels.meamed_dense) and callable(kernels.meamed_ptrs) and callable(kernels.keep_count)
    assert kernels.TRIM_MAX_CLIENTS == ref.K_MAX == 128
