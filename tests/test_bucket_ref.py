"""Bucketing without a GPU: the numpy restatement (tests/bucket_ref.py) pinned
against its stated consequences; the bucket adaptor of fjrobust_dev.h built for the host and
compared with it bitwise at all four widths; ``robust.bucket_gram``; and the product's host
surface: every refusal before the library is touched and at the C entries."""
import ctypes
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import bucket_ref as ref
from tests import robust_mean_ref as trim_ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
canon = lambda a: trim_ref.canon(a).tolist()


# ------------------------------------------------------------------ the restatement's consequences
def test_consequences_of_the_rule():
    rng = np.random.RandomState(5)
    x = trim_ref.mixed_data(rng, 37, 50)
    shuffle = rng.permutation(37)
    for t in (0, 3, 18):  # s = 1, identity: the trimmed mean itself; with a table: of the permuted rows
        assert canon(ref.trimmed_mean(x, 1, t)) == canon(trim_ref.trimmed_mean(x, t))
        assert canon(ref.trimmed_mean(x, 1, t, shuffle)) == canon(trim_ref.trimmed_mean(x[shuffle], t))
    # s >= K: one bucket, the mean in table order (first verbatim, sequential, one multiply)
    with np.errstate(all="ignore"):
        a = x[shuffle[0]].copy()
        for k in shuffle[1:]:
            a = (a + x[k]).astype(F32)
        want = (a * F32(1.0 / 37)).astype(F32)
    assert canon(ref.trimmed_mean(x, 37, 0, shuffle)) == canon(want)
    # a short bucket is divided by its own size: K = 7, s = 3 leaves a bucket of one, verbatim
    y = ref.bucket_means(x[:7], 3)
    assert y.shape == (3, 50) and y[2].view(np.uint32).tolist() == x[6].view(np.uint32).tolist()
    # a NaN client poisons only its own bucket, which is then trimmed
    z = rng.standard_normal((12, 9)).astype(F32)
    z[4] = np.nan
    m = ref.bucket_means(z, 3)
    assert np.isnan(m[1]).all() and np.isfinite(np.delete(m, 1, 0)).all()
    assert np.isfinite(ref.trimmed_mean(z, 3, 1)).all()


def test_clamp_restated():
    assert [ref.clamp(i, 5) for i in (-1, 0, 4, 5, -2**31, 2**31 - 1)] == [0, 0, 4, 4, 0, 4]


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
    exe = str(tmp_path_factory.mktemp("bucket_column") / "bucket_column_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
           os.path.join(ROOT, "tests", "bucket_column_host.cpp"), "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        cmd = [c for c in cmd if "sanitize" not in c]
        subprocess.run(cmd, check=True, capture_output=True)
    return exe


def _bits(v):
    return int(np.array([v], F32).view(np.uint32)[0])


def _run_host(exe, cases, tmp_path):
    """cases: (K, s, t, perm or None, x [K, P]). Returns per case {N: uint32 [P]}."""
    blob = [struct.pack("<i", len(cases))]
    for K, s, t, perm, x in cases:
        B = ref.bucket_count(K, s)
        n_last = K - (B - 1) * s
        blob.append(struct.pack("<5i3I", K, s, t, x.shape[1], perm is not None, _bits(trim_ref.inverse(B - 2 * t)),
                                _bits(trim_ref.inverse(s)), _bits(trim_ref.inverse(n_last))))
        if perm is not None:
            blob.append(np.ascontiguousarray(perm, dtype=np.int32).tobytes())
        blob.append(np.ascontiguousarray(x, dtype=F32).tobytes())
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint32)
    out, at = [], 0
    for K, s, t, perm, x in cases:
        P, B, per = x.shape[1], ref.bucket_count(K, s), {}
        for N in (16, 32, 64, 128):
            if B <= N:
                per[N] = got[at:at + P]
                at += P
        out.append(per)
    assert at == got.size
    return out


def _special_columns(K, P, rng):
    """Ties, +-0, +-inf and +-NaN with payloads in every column, among normal values."""
    x = trim_ref.mixed_data(rng, K, P, special=0.25, ties=0.25)
    sp = trim_ref.special_bits().view(F32)
    for p in range(P):
        rows = rng.choice(K, size=min(K, len(sp)), replace=False)
        x[rows, p] = sp[:len(rows)]
    return x


# (K, s): short last buckets of size 1 and s - 1, s = 1, s >= K, every width
HOST_SHAPES = [(5, 2), (7, 3), (11, 4), (16, 1), (17, 1), (9, 9), (33, 2), (40, 3), (64, 2), (100, 3), (130, 2),
               (257, 3), (255, 2), (512, 4), (1021, 8), (1024, 8), (128, 1), (300, 300)]


def test_host_build_of_the_adaptor_is_the_restatement(host_program, tmp_path):
    rng = np.random.RandomState(91)
    cases = []
    for K, s in HOST_SHAPES:
        B = ref.bucket_count(K, s)
        x = _special_columns(K, 24, rng)
        for name, perm in ref.tables(K, 7 * K + s).items():
            for t in ref.trims(B):
                cases.append((K, s, t, perm, x))
    # a stale table: entries outside [0, K) are clamped, never followed (the harness aborts on one)
    stale = np.array([-1, 9, 2**31 - 1, -2**31, 3, 0, 8, 100, 4], np.int32)
    cases.append((9, 2, 1, stale, _special_columns(9, 24, rng)))
    got = _run_host(host_program, cases, tmp_path)
    widths, lasts = set(), set()
    for (K, s, t, perm, x), per in zip(cases, got):
        table = None if perm is None else np.array([ref.clamp(int(i), K) for i in perm])
        want = ref.trimmed_mean(x, s, t, table)
        lasts.add((K - (ref.bucket_count(K, s) - 1) * s, s))
        for N, y in per.items():
            widths.add(N)
            assert canon(y.view(F32)) == canon(want), (K, s, t, N)
    assert widths == {16, 32, 64, 128}
    assert any(n == 1 and s > 1 for n, s in lasts) and any(n == s - 1 and s > 2 for n, s in lasts)


def test_clamp_function(host_program):
    for i, K, want in [(-1, 7, 0), (7, 7, 6), (-2**31, 7, 0), (2**31 - 1, 7, 6), (0, 7, 0), (6, 7, 6), (3, 1, 0),
                       (2**31 - 1, 4096, 4095)]:
        done = subprocess.run([host_program, "clamp", str(i), str(K)], capture_output=True, text=True)
        assert done.returncode == 0 and int(done.stdout) == want == ref.clamp(i, K), (i, K, done.stdout)


# ------------------------------------------------------------------------------ robust.bucket_gram
def _int_gram(K, rng):
    x = rng.randint(-8, 9, size=(K, 12)).astype(np.float64)
    return x, x @ x.T


def test_bucket_gram_exact_on_integers():
    from fedjax_amd import robust

    rng = np.random.RandomState(3)
    for K, s in [(8, 2), (16, 4), (64, 8), (32, 32)]:
        x, G = _int_gram(K, rng)
        for perm in ref.tables(K, K).values():
            table = np.arange(K) if perm is None else perm
            means = np.stack([x[table[j * s:(j + 1) * s]].sum(0) / s for j in range(K // s)])  # exact: s is 2^k
            got = robust.bucket_gram(G, s, perm)
            assert got.dtype == np.float64 and got.tobytes() == (means @ means.T).tobytes(), (K, s)
    _, G = _int_gram(9, rng)
    assert robust.bucket_gram(G, 1).tobytes() == G.tobytes()
    G[0, 1] = -0.0
    assert robust.bucket_gram(G, 1).tobytes() == G.tobytes()


def test_bucket_gram_short_bucket_against_fractions():
    from fedjax_amd import robust

    rng = np.random.RandomState(4)
    x = rng.standard_normal((7, 10))
    G = x @ x.T
    for perm in ref.tables(7, 11).values():
        got = robust.bucket_gram(G, 3, perm)
        groups = robust.bucket_members(7, 3, perm)
        assert [len(g) for g in groups] == [3, 3, 1]
        for a, ga in enumerate(groups):
            for b, gb in enumerate(groups):
                exact = sum(Fraction(G[i, j]) for i in ga for j in gb) / (len(ga) * len(gb))
                bound = (len(ga) * len(gb) + 2) * 2.0 ** -53 * np.abs(G).max()
                assert abs(Fraction(got[a, b]) - exact) <= bound, (a, b)


def test_bucket_gram_confines_a_nan_client():
    from fedjax_amd import robust

    rng = np.random.RandomState(6)
    x = rng.standard_normal((10, 6))
    G = x @ x.T
    G[4, :] = np.nan
    G[:, 4] = np.nan
    Gb = robust.bucket_gram(G, 3)  # client 4 is in bucket 1
    bad = ~np.isfinite(Gb)
    want = np.zeros((4, 4), bool)
    want[1, :] = want[:, 1] = True
    assert np.array_equal(bad, want)
    assert robust.usable(Gb).tolist() == [True, False, True, True]
    for wrong in ([0, 1], list(range(9)) + [8], [0.5] * 10):
        with pytest.raises((ValueError, TypeError)):
            robust.bucket_gram(G, 3, wrong)
    with pytest.raises(TypeError):
        robust.bucket_gram(G, True)
    with pytest.raises(ValueError):
        robust.bucket_gram(G, 0)


def test_bucket_krum_weights_make_the_mean_of_bucket_means():
    from fedjax_amd import tree_util

    rng = np.random.RandomState(8)
    x = rng.standard_normal((11, 5))  # s = 3: buckets of 3, 3, 3, 2
    G = x @ x.T
    selected, scores, w, ids, members = tree_util._bucket_krum_plan(G, 3, None, 0, 4)
    assert sorted(selected.tolist()) == [0, 1, 2, 3] and len(scores) == 4
    assert [w[k] for k in range(11)] == [2] * 9 + [3] * 2 and (ids == 0).all()
    selected, _, w, ids, members = tree_util._bucket_krum_plan(G, 3, None, 0, 1)
    assert set(w) == {1} and sorted(np.flatnonzero(ids == 0).tolist()) == sorted(members[0].tolist())


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


OLD_MESSAGE = "the trimmed mean and median support K <= 128 clients, got K = 129"


def test_kernels_refuse_before_the_library(no_library):
    from fedjax_amd import kernels

    assert kernels.BUCKET_MAX_CLIENTS == ref.K_MAX == 4096 and kernels.TRIM_MAX_CLIENTS == ref.B_MAX
    assert kernels.bucket_count(1024, 8) == 128 and kernels.bucket_count(4033, 32) == 127
    assert kernels.bucket_count(40, 64) == 1 and kernels.bucket_count(5, np.int64(2)) == 3
    for bad in (True, np.bool_(False), 2.0, "2", None):
        with pytest.raises(TypeError):
            kernels.bucket_count(10, bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match=">= 1"):
            kernels.bucket_count(10, bad)
    with pytest.raises(ValueError, match="128 buckets"):
        kernels.bucket_count(1025, 8)
    with pytest.raises(ValueError, match="4096"):
        kernels.bucket_count(4097, 64)
    with pytest.raises(ValueError, match="at least 1"):
        kernels.bucket_count(0, 2)
    with pytest.raises(ValueError, match="128"):  # unchanged: the unbucketed count still stops at 128
        kernels.trim_count(0, 129)
    x = torch.zeros(10, 8)
    with pytest.raises(TypeError):
        kernels.trim_bucket_dense(x, True, 0)
    with pytest.raises(TypeError):
        kernels.trim_bucket_dense(x, 2, True)
    with pytest.raises(ValueError, match="2t < B"):
        kernels.trim_bucket_dense(x, 2, 3)  # B = 5
    with pytest.raises(ValueError, match="128 buckets"):
        kernels.trim_bucket_dense(torch.zeros(129, 2), 1, 0)
    with pytest.raises(TypeError, match="float32"):
        kernels.trim_bucket_dense(x.to(torch.bfloat16), 2, 0)
    with pytest.raises(ValueError, match="perm must be"):
        kernels.trim_bucket_dense(x, 2, 0, perm=torch.arange(10, dtype=torch.int32))  # a host tensor
    with pytest.raises(ValueError, match="device tensors"):
        kernels.trim_bucket_dense(x, 2, 0)  # valid arguments, host tensor: still no library call
    img = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError, match="128 buckets"):
        kernels.trim_bucket_ptrs(img, 1, 300, 1, 2, 0, None)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.trim_bucket_ptrs(img, 0, 10, 1, 2, 0, None)
    with pytest.raises(TypeError):
        kernels.trim_bucket_ptrs(img, 1, 10, 1, False, 0, None)
    for wrong in ([0, 1, 2], [0, 0, 1, 2], [0, 1, 2, 4], [-1, 0, 1, 2]):
        with pytest.raises(ValueError, match="permutation"):
            kernels.check_bucket_perm(wrong, 4)
    for wrong in ([0.0, 1.0, 2.0, 3.0], [True, False, True, False]):
        with pytest.raises(TypeError):
            kernels.check_bucket_perm(wrong, 4)
    assert kernels.check_bucket_perm([3, 1, 0, 2], 4).dtype == np.int32 and kernels.check_bucket_perm(None, 4) is None


def test_slab_and_tree_refuse_before_the_library(no_library):
    from fedjax_amd import tree_util

    for call in (lambda s, **kw: s.trimmed_mean(0, **kw), lambda s, **kw: s.median(**kw)):
        with pytest.raises(ValueError) as e:
            call(_fake_slab(129))
        assert str(e.value) == OLD_MESSAGE
        with pytest.raises(ValueError, match="bucket_size"):
            call(_fake_slab(8), perm=[0] * 8)
        with pytest.raises(TypeError):
            call(_fake_slab(8), bucket_size=True)
        with pytest.raises(ValueError, match=">= 1"):
            call(_fake_slab(8), bucket_size=0)
        with pytest.raises(ValueError, match="128 buckets"):
            call(_fake_slab(1025), bucket_size=8)
        with pytest.raises(ValueError, match="4096"):
            call(_fake_slab(4097), bucket_size=64)
        with pytest.raises(ValueError, match="permutation"):
            call(_fake_slab(8), bucket_size=2, perm=[0, 1, 2, 3, 4, 5, 6, 6])
        with pytest.raises(TypeError, match="float32"):
            call(_fake_slab(8, torch.bfloat16), bucket_size=2)
    with pytest.raises(ValueError, match="2t < B"):
        _fake_slab(8).trimmed_mean(2, bucket_size=2)
    with pytest.raises(TypeError):
        _fake_slab(8).trimmed_mean(True, bucket_size=2)

    trees = lambda K: [{"w": np.zeros(3, F32)}] * K
    for call in (lambda t, **kw: tree_util.tree_trimmed_mean(t, 0, **kw), lambda t, **kw: tree_util.tree_median(t, **kw)):
        with pytest.raises(ValueError) as e:
            call(trees(129))
        assert str(e.value) == OLD_MESSAGE
        with pytest.raises(ValueError, match="bucket_size"):
            call(trees(4), perm=[0, 1, 2, 3])
        with pytest.raises(TypeError):
            call(trees(4), bucket_size=np.bool_(True))
        with pytest.raises(ValueError, match=">= 1"):
            call(trees(4), bucket_size=-1)
        with pytest.raises(ValueError, match="128 buckets"):
            call(trees(300), bucket_size=2)
        with pytest.raises(ValueError, match="4096"):
            call(trees(4097), bucket_size=64)
        with pytest.raises(ValueError, match="permutation"):
            call(trees(4), bucket_size=2, perm=[0, 1, 2, 2])
        assert call([], bucket_size=2) is None
    with pytest.raises(ValueError, match="2t < B"):
        tree_util.tree_trimmed_mean(trees(4), 1, bucket_size=2)


def test_gram_rules_refuse_before_the_library(no_library):
    from fedjax_amd import tree_util

    trees = [{"w": np.zeros(3, F32)}] * 12
    for krum, median in ((lambda **kw: _fake_slab(12).krum(1, **kw), lambda *a, **kw: _fake_slab(12).geometric_median(*a, **kw)),
                         (lambda **kw: tree_util.tree_krum(trees, 1, **kw),
                          lambda *a, **kw: tree_util.tree_geometric_median(trees, *a, **kw))):
        for call in (krum, median):
            with pytest.raises(ValueError, match="host-only"):
                call(bucket_size=2, select="device")
            with pytest.raises(ValueError, match="bucket_size"):
                call(perm=list(range(12)))
            with pytest.raises(TypeError):
                call(bucket_size=True)
            with pytest.raises(ValueError, match=">= 1"):
                call(bucket_size=0)
            with pytest.raises(ValueError, match="permutation"):
                call(bucket_size=2, perm=[0] * 12)
        with pytest.raises(ValueError, match="client weights"):
            median([1.0] * 12, bucket_size=2)
        with pytest.raises(ValueError, match="2f \\+ 3"):  # the checks run on B = 3: f = 1 needs 5 buckets
            krum(bucket_size=4)


def test_aggregators_check_their_arguments(no_library):
    from fedjax_amd import aggregators

    for build in (lambda **kw: aggregators.trimmed_mean_aggregator(0.1, **kw), aggregators.median_aggregator):
        assert isinstance(build(), aggregators.Aggregator)
        agg = build(bucket_size=2)  # rng=None: consecutive clients
        got, state = agg.apply(iter([]), agg.init())
        assert got is None
        for bad in (True, 2.0, "2"):
            with pytest.raises(TypeError):
                build(bucket_size=bad)
        with pytest.raises(ValueError, match=">= 1"):
            build(bucket_size=0)
        with pytest.raises(ValueError, match="bucket_size"):
            build(rng=np.array([0, 1], np.uint32))
        with pytest.raises((TypeError, ValueError)):
            build(bucket_size=2, rng=np.array([0.5, 1.0]))
        with pytest.raises(ValueError, match="128 buckets"):
            build(bucket_size=2).apply([(i, {"w": np.zeros(1, F32)}, 1.0) for i in range(300)], None)
        doc = build.__doc__ if build.__doc__ else aggregators.trimmed_mean_aggregator.__doc__
        assert "BUCKETS" in doc and "UNSHUFFLED" in doc


def test_c_entries_refuse_on_the_host():
    """The same refusals in the C entry points, with nothing launched (no GPU here)."""
    from fedjax_amd import _lib

    lib = _lib.load()
    for sym in ("fjagg_trim_bucket_dense", "fjagg_trim_bucket_ptrs"):
        assert sym in _lib.SYMBOLS

    def dense(dt, ld, K, P, s, t, fl, x=16, y=16, perm=None):
        return lib.fjagg_trim_bucket_dense(dt, x, ld, K, P, perm, s, t, 1.0, y, fl, None)

    err = lambda: lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 1025, 8, 8, 0, 0) == -3 and b"128 buckets" in err()
    assert dense(_lib.F32, 8, 129, 8, 1, 0, 0) == -3 and b"128 buckets" in err()
    assert dense(_lib.F32, 8, 4097, 8, 64, 0, 0) == -3 and b"4096" in err()
    assert dense(_lib.F32, 8, 10, 8, 0, 0, 0) == -1 and b"s >= 1" in err()
    assert dense(_lib.F32, 8, 10, 8, -2, 0, 0) == -1
    assert dense(_lib.F32, 8, 0, 8, 2, 0, 0) == -1
    assert dense(_lib.F32, 8, 10, 8, 2, -1, 0) == -1
    assert dense(_lib.F32, 8, 10, 8, 2, 3, 0) == -1 and b"2t < B" in err()  # B = 5
    assert dense(_lib.F32, 8, 10, 8, 64, 1, 0) == -1  # one bucket
    assert dense(_lib.BF16, 8, 10, 8, 2, 0, 0) == -3 and b"float32" in err()
    assert dense(_lib.I32, 8, 10, 8, 2, 0, 0) == -3
    assert dense(_lib.F32, 8, 10, 8, 2, 0, 0, x=None) == -1 and b"null" in err()
    assert dense(_lib.F32, 8, 10, 8, 2, 0, 0, y=None) == -1
    assert dense(_lib.F32, 8, 10, 0, 2, 0, 0) == -1
    assert dense(_lib.F32, 7, 10, 8, 2, 0, 0) == -1 and b"ld" in err()
    assert dense(_lib.F32, 1 << 29, 10, (1 << 28) + 1, 2, 0, 0) == -3 and b"1 GiB" in err()
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, _lib.UNALIGNED,
               1 << 8, 1 << 16):
        assert dense(_lib.F32, 8, 10, 8, 2, 0, fl) == -3, fl
    img = np.zeros(64, np.int64)

    def ptrs(dt, L, K, nblk, s, t, fl, im=img.ctypes.data):
        return lib.fjagg_trim_bucket_ptrs(dt, im, L, K, nblk, None, s, t, 1.0, fl, None)

    assert ptrs(_lib.F32, 1, 1025, 1, 8, 0, 0) == -3 and b"128 buckets" in err()
    assert ptrs(_lib.F32, 1, 4097, 1, 64, 0, 0) == -3 and b"4096" in err()
    assert ptrs(_lib.F32, 1, 10, 1, 0, 0, 0) == -1
    assert ptrs(_lib.F32, 1, 0, 1, 2, 0, 0) == -1
    assert ptrs(_lib.F32, 1, 10, 1, 2, 3, 0) == -1 and b"2t < B" in err()
    assert ptrs(_lib.BF16, 1, 10, 1, 2, 0, 0) == -3
    assert ptrs(_lib.F32, 0, 10, 1, 2, 0, 0) == -1 and b"bad plan" in err()
    assert ptrs(_lib.F32, 1, 10, 0, 2, 0, 0) == -1
    assert ptrs(_lib.F32, 1, 10, 1, 2, 0, 0, im=None) == -1
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, 1 << 8):
        assert ptrs(_lib.F32, 1, 10, 1, 2, 0, fl) == -3, fl
    # unchanged: the unbucketed entry still stops at 128 clients
    assert lib.fjagg_trim_dense(_lib.F32, 16, 8, 129, 8, 0, 1.0, 16, 0, None) == -3 and b"K <= 128" in err()


def test_exports():
    from fedjax_amd import kernels, random, robust, tree_util

    for name in ("trim_bucket_dense", "trim_bucket_ptrs", "bucket_count"):
        assert callable(getattr(kernels, name))
    assert "permutation" in random.__all__ and "bucket_gram" in robust.__all__
    assert "BucketedKrumResult" in tree_util.__all__
    assert "not ``jax.random.permutation``" in random.permutation.__doc__.replace("NOT", "not")
