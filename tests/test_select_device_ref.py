"""The device selection of Krum and the smoothed Weiszfeld algorithm without a GPU: the rules of
fedjax_amd/csrc/fjselect_dev.h built for the host and compared bit for bit with
fedjax_amd.robust (Krum) and with the numpy restatement of tests/select_device_ref.py
(Weiszfeld, whose sum order robust.py leaves to BLAS); the restatement against robust.py within
the bound DESIGN §3q states; every refusal of the C entries and of the Python surfaces."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from fedjax_amd import robust
from tests import select_device_ref as ref

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).tolist()


# ----------------------------------------------------------- the device rules, built for the host
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
    exe = str(tmp_path_factory.mktemp("select_device") / "select_device_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
           os.path.join(ROOT, "tests", "select_device_host.cpp"), "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        cmd = [c for c in cmd if "sanitize" not in c]
        subprocess.run(cmd, check=True, capture_output=True)
    return exe


def _take(buf, at, dtype, n):
    size = np.dtype(dtype).itemsize * n
    return np.frombuffer(buf[at:at + size], dtype=dtype), at + size


def _run_host(exe, cases, tmp_path):
    """cases: ("krum", G, f, m) or ("weiszfeld", G, alpha or None, nu, iterations). Returns per
    case the tuple the restatements return."""
    blob = [struct.pack("<i", len(cases))]
    last = None
    for case in cases:
        G = np.ascontiguousarray(case[1], dtype=F64)
        K = G.shape[0]
        if case[0] == "krum":
            again = last is not None and last[0] is case[1] and last[1] == case[2]  # the same G and f: scores kept
            blob.append(struct.pack("<4id", 0, -K if again else K, case[2], case[3], 0.0))
            if not again:
                blob.append(G.tobytes())
            last = (case[1], case[2])
        else:
            alpha = case[2]
            blob.append(struct.pack("<4id", 1, K, int(alpha is not None), case[4], float(case[3])))
            blob.append(G.tobytes())
            if alpha is not None:
                blob.append(np.ascontiguousarray(alpha, dtype=F64).tobytes())
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    buf, at, out = dst.read_bytes(), 0, []
    for case in cases:
        K = case[1].shape[0]
        if case[0] == "krum":
            m = case[3]
            scores, at = _take(buf, at, F64, K)
            selected, at = _take(buf, at, np.int64, m)
            count, at = _take(buf, at, np.int32, 1)
            order, at = _take(buf, at, np.int32, m)
            seg, at = _take(buf, at, np.int32, 2)
            wperm, at = _take(buf, at, F32, m)
            gscale, at = _take(buf, at, F32, 1)
            out.append((scores, selected, int(count[0]), order, seg, wperm, gscale))
        else:
            a, at = _take(buf, at, F64, K)
            d, at = _take(buf, at, F64, K)
            a32, at = _take(buf, at, F32, K)
            count, at = _take(buf, at, np.int32, 1)
            order, at = _take(buf, at, np.int32, K)
            seg, at = _take(buf, at, np.int32, 2)
            wperm, at = _take(buf, at, F32, K)
            gscale, at = _take(buf, at, F32, 1)
            out.append((a, d, a32, int(count[0]), order, seg, wperm, gscale))
    assert at == len(buf)
    return out


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, int):
            assert g == w, (what, i, g, w)
        else:
            assert g.dtype == w.dtype and bits(g) == bits(w), (what, i)


@pytest.mark.parametrize("K", ref.KS)
def test_krum_host_build_is_robust_py_bit_for_bit(K, host_program, tmp_path):
    inputs = ref.krum_inputs(np.random.RandomState(1000 + K), K)
    cases = [("krum", G, f, m) for G in inputs.values() for f, m in ref.krum_params(K)]
    names = [(name, f, m) for name in inputs for f, m in ref.krum_params(K)]
    got = _run_host(host_program, cases, tmp_path)
    seen_short = seen_clamp = False
    for (name, f, m), (_, G, _, _), res in zip(names, cases, got):
        want = ref.krum_tables(G, f, m)
        _same(res, want, (K, name, f, m))
        scores, selected, count = want[:3]
        # what the inputs are there to show
        if name == "twins":
            assert scores[0] == scores[K - 1]
            picked = selected[:count].tolist()
            assert K - 1 not in picked or 0 in picked
            if K - 1 in picked:
                assert picked.index(0) < picked.index(K - 1)
        if name in ("nan_diagonal", "inf_diagonal"):
            assert np.isinf(scores[K // 2]) and K // 2 not in selected
        if name == "few_usable":
            assert count <= 2 and not set(selected[:count].tolist()) - {0, 1}
            if K - f - 2 > 1:
                assert count == 0 and np.isinf(scores).all()
                seen_short = True
        if name == "all_unusable":
            assert count == 0 and (selected == -1).all() and bits(want[6]) == [0] and want[4].tolist() == [0, 0]
        if name == "negative_d2":
            assert robust.sq_distances(G)[0, 1] == 0.0
            seen_clamp = True
        assert (np.diff(want[3][:count]) > 0).all()
    assert seen_clamp and (seen_short or K <= 4)


def _weiszfeld_cases(K):
    inputs = ref.weiszfeld_inputs(np.random.RandomState(2000 + K), K)
    return [(name, G, alpha, T) for name, (G, alpha) in inputs.items() for T in (0, 1, 4)]


@pytest.mark.parametrize("K", ref.KS)
def test_weiszfeld_host_build_is_the_restatement_bit_for_bit(K, host_program, tmp_path):
    named = _weiszfeld_cases(K)
    got = _run_host(host_program, [("weiszfeld", G, alpha, 1e-6, T) for _, G, alpha, T in named], tmp_path)
    for (name, G, alpha, T), res in zip(named, got):
        want = ref.weiszfeld(G, alpha, 1e-6, T)
        _same(res, want, (K, name, T))
        a, d, a32, count = want[:4]
        if T == 0:
            assert not d[np.isfinite(d)].any()
        if name == "one_unusable":
            assert a[K // 2] == 0 and np.isinf(d[K // 2]) and K // 2 not in want[4][:count] and count == K - 1
        if name == "twin":
            assert a[0] == a[K - 1] or T > 0  # (the twins share every distance: equal beta)
            assert bits(np.array([d[0]])) == bits(np.array([d[K - 1]]))


# The bound: both sides are references (the restatement and robust.py), which differ in the order
# of three sums per iteration: BLAS for G @ a and a @ Ga, numpy's pairwise sum for the totals.
# Measured here over these 14 (K, input) pairs at iterations = 4: worst relative difference of a
# 6.8e-16 and 0 float32 ulps (an earlier measurement over 18 cases: 1.6e-15); 1e-12
# and 1 ulp leave room for another BLAS.
@pytest.mark.parametrize("K", ref.KS)
def test_restatement_agrees_with_robust_py(K):
    inputs = ref.weiszfeld_inputs(np.random.RandomState(2000 + K), K)
    worst = 0.0
    for name in ("unit", "outlier"):
        G, alpha = inputs[name]
        a, d, a32 = ref.weiszfeld(G, alpha, 1e-6, 4)[:3]
        a_ref, d_ref = robust.weiszfeld_weights(G, alpha, 1e-6, 4)
        rel = np.abs(a - a_ref) / a_ref
        worst = max(worst, float(rel.max()))
        ulps = int(ref.ulp_distance32(a32, a_ref.astype(F32)).max())
        print(f"K={K} {name}: worst relative difference {rel.max():.3g}, {ulps} float32 ulps")
        assert rel.max() <= 1e-12, (name, rel.max())
        assert ulps <= 1, (name, ulps)
        assert np.allclose(d, d_ref, rtol=1e-9, atol=0)


def test_restatement_small_case_by_hand():
    """Three clients on a line at 0, 1, 3 (one coordinate): one iteration from the mean 4/3."""
    x = np.array([[0.0], [1.0], [3.0]], F32)
    a, d, a32, count, order, seg, wperm, gscale = ref.weiszfeld(ref.gram_of(x), None, 1e-6, 1)
    assert np.allclose(d, [4 / 3, 1 / 3, 5 / 3], rtol=1e-14)
    beta = 1 / np.array([4 / 3, 1 / 3, 5 / 3])
    assert np.allclose(a, beta / beta.sum(), rtol=1e-14)
    assert count == 3 and order.tolist() == [0, 1, 2] and seg.tolist() == [0, 3] and bits(wperm) == bits(a32)
    W = F64(a32[0]) + F64(a32[1]) + F64(a32[2])
    assert bits(gscale) == bits(np.array([F32(1.0 / W)]))


# ---------------------------------------------------------------------------------- refusals
def test_c_entries_refuse_on_the_host():
    """Every refusal of the new entries is made before any HIP call (no GPU here)."""
    from fedjax_amd import _lib

    lib = _lib.load()
    err = lib.fjagg_last_error
    p = 64  # any non-null address: nothing is dereferenced before the checks pass

    def krum(K, f, m, gram=p, scores=p, selected=p, count=p, order=p, seg=p, wperm=p, gscale=p):
        return lib.fjagg_krum_select(gram, K, f, m, scores, selected, count, order, seg, wperm, gscale, None)

    assert krum(0, 0, 1) == -1 and b"K must be >= 1" in err()
    assert krum(1025, 0, 1) == -3 and b"1024" in err()
    assert krum(5, -1, 1) == -1 and b"f must be >= 0" in err()
    assert krum(4, 1, 1) == -1 and b"2f + 3" in err()
    assert krum(2, 0, 1) == -1 and b"2f + 3" in err()
    assert krum(5, 1 << 40, 1) == -1 and b"2f + 3" in err()
    assert krum(5, 1, 0) == -1 and b"[1, 4]" in err()
    assert krum(5, 1, 5) == -1 and b"[1, K - f]" in err()
    for name in ("gram", "scores", "selected", "count", "order", "seg", "wperm", "gscale"):
        assert krum(5, 1, 1, **{name: None}) == -1 and b"null" in err(), name

    def weisz(K, nu, T, gram=p, alpha=None, a=p, d=p, a32=p, count=p, order=p, seg=p, wperm=p, gscale=p):
        return lib.fjagg_weiszfeld_select(gram, K, alpha, nu, T, a, d, a32, count, order, seg, wperm, gscale, None)

    assert weisz(0, 1e-6, 4) == -1 and b"K must be >= 1" in err()
    assert weisz(1025, 1e-6, 4) == -3 and b"1024" in err()
    assert weisz(4, 1e-6, -1) == -1 and b"iterations must be >= 0" in err()
    for nu in (0.0, -1.0, float("inf"), float("nan")):
        assert weisz(4, nu, 4) == -1 and b"nu must be finite and > 0" in err(), nu
    for name in ("gram", "a", "d", "a32", "count", "order", "seg", "wperm", "gscale"):
        assert weisz(4, 1e-6, 4, **{name: None}) == -1 and b"null" in err(), name

    def dense(K, P, M, ld=None, dt=_lib.F32, fl=_lib.SCALE, x=p, order=p, seg=p, wperm=p, gscale=p, out=p):
        return lib.fjagg_wsum_group_dense_dev(dt, x, P if ld is None else ld, K, P, M, order, seg, wperm, gscale, out,
                                              fl, None)

    assert dense(0, 8, 1) == -1 and b"K must be >= 1" in err()
    assert dense(4, 8, 0) == -1 and b"M_max must be in [1, K]" in err()
    assert dense(4, 8, 5) == -1 and b"[1, 4]" in err()
    assert dense(4, 0, 1) == -1 and dense(4, 8, 1, ld=7) == -1 and b"ld" in err()
    assert dense(4, (1 << 28) + 1, 1) == -3 and b"1 GiB" in err()
    assert dense(4, 8, 1, dt=_lib.BF16) == -3 and b"float32" in err()
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, _lib.UNALIGNED, 1 << 8):
        assert dense(4, 8, 1, fl=fl) == -3, fl
    for name in ("x", "order", "seg", "wperm", "gscale", "out"):
        assert dense(4, 8, 1, **{name: None}) == -1 and b"null" in err(), name

    def ptrs(K, M, L=1, nblk=1, dt=_lib.F32, fl=_lib.SCALE, image=p, seg=p, wperm=p, gscale=p):
        return lib.fjagg_wsum_group_ptrs_dev(dt, image, L, K, M, nblk, seg, wperm, gscale, fl, None)

    assert ptrs(0, 1) == -1 and b"K must be >= 1" in err()
    assert ptrs(4, 0) == -1 and ptrs(4, 5) == -1 and b"M_max must be in [1, K]" in err()
    assert ptrs(4, 1, L=0) == -1 and b"bad plan" in err()
    assert ptrs(4, 1, nblk=0) == -1 and b"bad plan" in err()
    assert ptrs(4, 1, dt=_lib.BF16) == -3
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, 1 << 8):
        assert ptrs(4, 1, fl=fl) == -3, fl
    for name in ("image", "seg", "wperm", "gscale"):
        assert ptrs(4, 1, **{name: None}) == -1 and b"null" in err(), name

    def gather(K, M, L=1, all_=p, order=p, seg=p, group=p):
        return lib.fjagg_gather_member_ptrs(all_, L, K, order, seg, M, group, None)

    assert gather(0, 1) == -1 and b"K must be >= 1" in err()
    assert gather(1025, 1) == -3 and b"1024" in err()
    assert gather(4, 0) == -1 and gather(4, 5) == -1 and b"M_max must be in [1, K]" in err()
    assert gather(4, 1, L=0) == -1 and b"L must be >= 1" in err()
    for name in ("all_", "order", "seg", "group"):
        assert gather(4, 1, **{name: None}) == -1 and b"null" in err(), name


def _bare_slab(K):
    """A slab's host-side attributes without its storage: the checks under test come first."""
    from fedjax_amd.slab import ClientDeltaSlab

    s = object.__new__(ClientDeltaSlab)
    s.dtype, s.num_clients, s.num_params = torch.float32, K, 8
    return s


def test_select_keyword_on_every_surface():
    from fedjax_amd import aggregators, kernels, tree_util

    trees = [{"w": torch.zeros(3)} for _ in range(5)]
    slab = _bare_slab(5)
    for bogus in ("bogus", "Device", None, 1, True):
        with pytest.raises(ValueError, match="select must be"):
            tree_util.tree_krum(trees, 1, select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            tree_util.tree_geometric_median(trees, select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            slab.krum(1, select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            slab.geometric_median(select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            aggregators.krum_aggregator(1, select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            aggregators.geometric_median_aggregator(select=bogus)
    assert kernels.check_select("host") is False and kernels.check_select("device") is True


def test_device_route_checks_its_arguments_as_the_host_route_does():
    """The same exceptions, raised before any launch (these are host tensors: a launch would be
    refused for that reason instead)."""
    from fedjax_amd import aggregators, tree_util

    trees = [{"w": torch.zeros(3)} for _ in range(5)]
    slab = _bare_slab(5)
    for call in (lambda **kw: tree_util.tree_krum(trees, **kw), lambda **kw: slab.krum(**kw)):
        for select in ("host", "device"):
            with pytest.raises(TypeError, match="num_byzantine must be an int"):
                call(num_byzantine=True, select=select)
            with pytest.raises(TypeError, match="num_selected must be an int"):
                call(num_byzantine=1, num_selected=True, select=select)
            with pytest.raises(ValueError, match="2f \\+ 3"):
                call(num_byzantine=2, select=select)
            with pytest.raises(ValueError, match="num_selected"):
                call(num_byzantine=1, num_selected=5, select=select)
    for call in (lambda *a, **kw: tree_util.tree_geometric_median(trees, *a, **kw),
                 lambda *a, **kw: slab.geometric_median(*a, **kw)):
        for select in ("host", "device"):
            with pytest.raises(ValueError, match="weights"):
                call([1.0, 2.0], select=select)
            with pytest.raises(ValueError, match="finite and > 0"):
                call([1.0, 2.0, 0.0, 1.0, 1.0], select=select)
            if select == "device":  # (the host route checks these after its Gram pass)
                with pytest.raises(TypeError, match="iterations"):
                    call(iterations=True, select=select)
                with pytest.raises(ValueError, match="iterations"):
                    call(iterations=-1, select=select)
            with pytest.raises(ValueError, match="nu"):
                call(nu=0.0, select=select)
            with pytest.raises(TypeError, match="nu"):
                call(nu="x", select=select)
    with pytest.raises(TypeError):
        aggregators.krum_aggregator(True, select="device")
    assert tree_util.tree_krum([], 0, select="device") is None
    assert tree_util.tree_geometric_median(iter([]), select="device") is None
    agg = aggregators.krum_aggregator(1, 2, select="device")
    mean, state = agg.apply(iter([]), agg.init())
    assert mean is None and isinstance(state, aggregators.DeviceKrumAggregatorState) and state.client_ids == ()
    agg = aggregators.geometric_median_aggregator(select="device")
    mean, state = agg.apply([], agg.init())
    assert mean is None and isinstance(state, aggregators.DeviceGeometricMedianAggregatorState)


def test_select_wrappers_check_before_the_library_is_touched():
    from fedjax_amd import kernels

    G = torch.zeros(5, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.krum_select_device(G, 1, 1)
    with pytest.raises(ValueError, match="float64"):
        kernels.krum_select_device(G.float(), 1, 1)
    with pytest.raises(ValueError, match="float64"):
        kernels.weiszfeld_select_device(torch.zeros(5, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="1024"):
        kernels.krum_select_device(torch.zeros(1025, 1025, dtype=torch.float64), 1, 1)


def test_surface_and_symbols():
    from fedjax_amd import _lib, kernels, tree_util

    assert _lib.ABI_VERSION == 4  # additions only
    for sym in ("fjagg_krum_select", "fjagg_weiszfeld_select", "fjagg_wsum_group_dense_dev",
                "fjagg_wsum_group_ptrs_dev", "fjagg_gather_member_ptrs"):
        assert sym in _lib.SYMBOLS
        assert isinstance(getattr(_lib.load(), sym), ctypes._CFuncPtr)
    assert tree_util.DeviceKrumResult._fields == ("mean", "selected", "count", "scores", "gram")
    assert tree_util.DeviceGeometricMedianResult._fields == ("median", "weights", "distances", "count", "gram")
    for name in ("DeviceKrumResult", "DeviceGeometricMedianResult"):
        assert name in tree_util.__all__
    assert callable(kernels.krum_select_device) and callable(kernels.weiszfeld_select_device)
