"""Bulyan's device selection without a GPU: the rule of fedjax_amd/csrc/fjselect_dev.h built for
the host and compared exactly with fedjax_amd.robust.bulyan_select + tree_util._bulyan_plan
(selected, count, keep, scale, rows) and bit for bit with the numpy restatement of
tests/bulyan_select_ref.py (step_scores); the column routine's independence of its width; every
refusal of the three C entries and of the Python surfaces."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from fedjax_amd import robust, tree_util
from tests import bulyan_select_ref as ref

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


def _build(tmp_path_factory, name):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp(name) / name)
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
           os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        cmd = [c for c in cmd if "sanitize" not in c]
        subprocess.run(cmd, check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return _build(tmp_path_factory, "bulyan_select_host")


@pytest.fixture(scope="module")
def column_program(tmp_path_factory):
    return _build(tmp_path_factory, "around_median_host")


def _take(buf, at, dtype, n):
    size = np.dtype(dtype).itemsize * n
    return np.frombuffer(buf[at:at + size], dtype=dtype), at + size


def _run_host(exe, cases, tmp_path):
    """cases: (G, f). Returns per case (selected, count, step_scores, keep, scale, rows)."""
    blob = [struct.pack("<i", len(cases))]
    for G, f in cases:
        G = np.ascontiguousarray(G, dtype=F64)
        blob.append(struct.pack("<2i", G.shape[0], f))
        blob.append(G.tobytes())
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    buf, at, out = dst.read_bytes(), 0, []
    for G, f in cases:
        theta = G.shape[0] - 2 * f
        selected, at = _take(buf, at, np.int64, theta)
        count, at = _take(buf, at, np.int32, 1)
        step_scores, at = _take(buf, at, F64, theta)
        keep, at = _take(buf, at, np.int32, 1)
        scale, at = _take(buf, at, F32, 1)
        rows, at = _take(buf, at, np.int32, theta)
        out.append((selected, int(count[0]), step_scores, int(keep[0]), scale, rows))
    assert at == len(buf)
    return out


def _host_route_tables(G, f):
    """What the host route computes and passes: robust.bulyan_select, tree_util._bulyan_plan and
    np.float32(1 / keep), laid out as the device tables are."""
    K = G.shape[0]
    theta = K - 2 * f
    picked, members, keep = tree_util._bulyan_plan(G, f)
    assert picked.tolist() == robust.bulyan_select(G, f).tolist()
    count = len(picked)
    selected = np.full(theta, -1, np.int64)
    selected[:count] = picked
    rows = np.zeros(theta, np.int32)
    rows[:count] = members
    rows[count:] = members[-1] if count else 0
    scale = np.array([np.float32(tree_util._inverse(keep))], F32)
    return selected, count, keep, scale, rows


@pytest.mark.parametrize("kind", ["integer", "random"])
@pytest.mark.parametrize("K,f", ref.KFS)
def test_bulyan_host_build_is_robust_py_and_the_restatement(K, f, kind, host_program, tmp_path):
    rng = np.random.RandomState(3000 + 7 * K + (kind == "random"))
    named = ref.inputs(rng, K, f, kind)
    perm = rng.permutation(K)
    cases, names = [], []
    for name, (G, expect) in named.items():
        cases += [(G, f), (ref.permuted(G, perm), f)]
        names += [(name, expect, False), (name, expect, True)]
    got = _run_host(host_program, cases, tmp_path)
    theta = K - 2 * f
    for (name, expect, is_perm), (G, _), res in zip(names, cases, got):
        what = (K, f, kind, name, is_perm)
        selected, count, step_scores, keep, scale, rows = res
        h_selected, h_count, h_keep, h_scale, h_rows = _host_route_tables(G, f)
        assert selected.tolist() == h_selected.tolist(), what
        assert (count, keep) == (h_count, h_keep), what
        assert bits(scale) == bits(h_scale), what
        assert rows.tolist() == h_rows.tolist(), what
        r_selected, r_count, r_scores, r_keep, r_scale, r_rows = ref.select(G, f)
        assert selected.tolist() == r_selected.tolist() and count == r_count, what
        assert bits(step_scores) == bits(r_scores), what
        assert keep == r_keep and bits(scale) == bits(r_scale) and rows.tolist() == r_rows.tolist(), what
        # what the inputs are there to show
        assert count == expect, what
        assert keep == (count - 2 * f if count >= 2 * f + 1 else 0)
        assert ((rows >= 0) & (rows < K)).all() and (np.diff(rows[:count]) > 0).all()
        assert (selected[count:] == -1).all() and np.isinf(step_scores[count:]).all()
        if name in ("base", "duplicated", "unusable_2f"):
            assert count == theta and keep == theta - 2 * f
        if name == "short":
            assert count == theta - 1
        if name == "too_short":
            assert keep == 0 and bits(scale) == [0]
        if name == "all_unusable":
            assert count == 0 and (rows == 0).all()
        if name == "duplicated" and not is_perm and K >= 4:
            first = int(selected[0])  # twins share every score: the lower index of a pair wins first
            assert first % 2 == 0 or first == K - 1
    # (a permutation need not permute the selection: two mutual nearest neighbours tie whenever c = 1)


def test_restatement_small_case_by_hand():
    """Five clients on a line at 0, 1, 2, 4, 100 (one coordinate), f = 0: theta = 5, c = n - 2."""
    x = np.array([[0.0], [1.0], [2.0], [4.0], [100.0]], F32)
    selected, count, step_scores, keep, scale, rows = ref.select(ref.gram_of(x), 0)
    # n = 5, c = 3: scores 1+4+16, 1+1+9, 1+4+4, 4+9+16, ...: client 2 (9); n = 4, c = 2: client 0 has
    # 1+16, client 1 has 1+9, client 3 has 9+16: client 1 (10); n = 3, c = 1: 0 -> 16, 3 -> 16, 4 -> 96^2:
    # the tie goes to client 0; n = 2, c = 1: both 96^2: client 3; n = 1: score 0.0
    assert selected.tolist() == [2, 1, 0, 3, 4] and count == 5
    assert step_scores.tolist() == [9.0, 10.0, 16.0, 9216.0, 0.0]
    assert keep == 5 and bits(scale) == bits(np.array([F32(0.2)])) and rows.tolist() == [0, 1, 2, 3, 4]


def test_column_routine_does_not_depend_on_its_width(column_program, tmp_path):
    """The same M <= 16 inputs through N = 16, 32, 64 and 128 of around_median_column: the same
    bits, which is why a short selection run at theta's width equals the host route's."""
    rng = np.random.RandomState(77)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.0, -1.0, 1e30, -1e30, 1e-40, 2.5, 2.5,
                        3.0, -7.0], F32)
    cases = []
    for M in (1, 2, 3, 7, 10, 15, 16):
        P = 64
        x = rng.standard_normal((M, P)).astype(F32)
        x[:, : P // 2] = special[rng.randint(0, len(special), (M, P // 2))]  # NaN, +-inf, +-0 and ties
        x[:, P // 2: P // 2 + 8] = rng.randint(-1, 2, (M, 8)).astype(F32)  # almost all ties
        for keep in sorted({1, (M + 1) // 2, max(M - 2, 1), M}):
            cases.append((M, keep, x))
    blob = [struct.pack("<i", len(cases))]
    for M, keep, x in cases:
        scale = np.array([np.float32(1.0 / keep)], F32).view(np.uint32)[0]
        blob.append(struct.pack("<4iI", 0, M, keep, x.shape[1], int(scale)))
        blob.append(np.ascontiguousarray(x).view(np.uint32).tobytes())
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([column_program, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    buf, at = dst.read_bytes(), 0
    for M, keep, x in cases:
        P = x.shape[1]
        widths = []
        for N in (16, 32, 64, 128):
            y, at = _take(buf, at, np.uint32, P)
            widths.append(y.tolist())
        assert widths[0] == widths[1] == widths[2] == widths[3], (M, keep)
        if keep == M:  # and the routine is not trivially constant: keep = M is the plain sum in client order
            s = x[0].copy()
            with np.errstate(all="ignore"):
                for k in range(1, M):
                    s = s + x[k]
                want = s * np.float32(1.0 / keep)
            fin = np.isfinite(want)
            assert np.array(widths[0], np.uint32)[fin].tolist() == want.view(np.uint32)[fin].tolist()
    assert at == len(buf)


# ---------------------------------------------------------------------------------- refusals
def test_c_entries_refuse_on_the_host():
    """Every refusal of the new entries is made before any HIP call (no GPU here)."""
    from fedjax_amd import _lib

    lib = _lib.load()
    err = lib.fjagg_last_error
    p = 64  # any non-null, 8-byte aligned address: nothing is dereferenced before the checks pass
    big = 1 << 30

    assert lib.fjagg_bulyan_select_workspace_bytes(252) == 252 * 251 * 9
    assert lib.fjagg_bulyan_select_workspace_bytes(3) == 54
    assert lib.fjagg_bulyan_select_workspace_bytes(2) == 0 and lib.fjagg_bulyan_select_workspace_bytes(253) == 0

    def select(K, f, gram=p, ws=p, ws_bytes=big, selected=p, count=p, step_scores=p, keep=p, scale=p, rows=p):
        return lib.fjagg_bulyan_select(gram, K, f, ws, ws_bytes, selected, count, step_scores, keep, scale, rows, None)

    assert select(0, 0) == -1 and b"K must be >= 1" in err()
    assert select(1025, 0) == -3 and b"1024" in err()
    assert select(7, -1) == -1 and b"f must be >= 0" in err()
    assert select(6, 1) == -1 and b"4f + 3" in err()
    assert select(2, 0) == -1 and b"4f + 3" in err()
    assert select(7, 1 << 40) == -1 and b"4f + 3" in err()
    assert select(129, 0) == -3 and b"K - 2f <= 128" in err()
    assert select(253, 62) == -3 and b"K - 2f <= 128" in err()
    assert select(1000, 10) == -3 and b"K - 2f <= 128" in err()
    assert select(252, 62, ws_bytes=252 * 251 * 9 - 1) == -1 and b"workspace" in err()
    assert select(7, 1, ws_bytes=0) == -1 and b"workspace" in err()
    assert select(7, 1, ws=68) == -1 and b"8-byte aligned" in err()
    for name in ("gram", "ws", "selected", "count", "step_scores", "keep", "scale", "rows"):
        assert select(7, 1, **{name: None}) == -1 and b"null" in err(), name

    def dense(K_rows, P, M, ld=None, dt=_lib.F32, fl=_lib.SCALE, x=p, rows=p, count=p, keep=p, scale=p, out=p):
        return lib.fjagg_meamed_dense_dev(dt, x, P if ld is None else ld, K_rows, P, M, rows, count, keep, scale, out,
                                          fl, None)

    assert dense(4, 8, 0) == -1 and b"K must be >= 1" in err()
    assert dense(200, 8, 129) == -3 and b"128" in err()
    assert dense(0, 8, 1) == -1 and dense(1025, 8, 1) == -3 and b"K_rows" in err()
    assert dense(4, 8, 5) == -1 and b"M_max <= K_rows" in err()
    assert dense(4, 0, 1) == -1 and dense(4, 8, 1, ld=7) == -1 and b"ld" in err()
    assert dense(4, (1 << 28) + 1, 1) == -3 and b"1 GiB" in err()
    assert dense(4, 8, 1, dt=_lib.BF16) == -3 and b"float32" in err()
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, _lib.UNALIGNED, 1 << 8):
        assert dense(4, 8, 1, fl=fl) == -3, fl
    for name in ("x", "rows", "count", "keep", "scale", "out"):
        assert dense(4, 8, 1, **{name: None}) == -1 and b"null" in err(), name

    def ptrs(K_rows, M, L=1, nblk=1, dt=_lib.F32, fl=_lib.SCALE, image_all=p, image_group=p, rows=p, count=p, keep=p,
             scale=p):
        return lib.fjagg_meamed_ptrs_dev(dt, image_all, image_group, L, K_rows, M, nblk, rows, count, keep, scale, fl,
                                         None)

    assert ptrs(4, 0) == -1 and b"K must be >= 1" in err()
    assert ptrs(200, 129) == -3 and b"128" in err()
    assert ptrs(0, 1) == -1 and ptrs(1025, 1) == -3 and b"K_rows" in err()
    assert ptrs(4, 5) == -1 and b"M_max <= K_rows" in err()
    assert ptrs(4, 1, L=0) == -1 and b"bad plan" in err()
    assert ptrs(4, 1, nblk=0) == -1 and b"bad plan" in err()
    assert ptrs(4, 1, dt=_lib.BF16) == -3
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, 1 << 8):
        assert ptrs(4, 1, fl=fl) == -3, fl
    for name in ("image_all", "image_group", "rows", "count", "keep", "scale"):
        assert ptrs(4, 1, **{name: None}) == -1 and b"null" in err(), name


def test_k_limit_arithmetic():
    """K >= 4f + 3 and K - 2f <= 128 together bound K at 252 (fjagg.h)."""
    ok = [(K, f) for K in range(1, 1025) for f in range(0, 300) if K >= 4 * f + 3 and K - 2 * f <= 128]
    assert max(K for K, _ in ok) == 252 and (252, 62) in ok


def _bare_slab(K):
    """A slab's host-side attributes without its storage: the checks under test come first."""
    from fedjax_amd.slab import ClientDeltaSlab

    s = object.__new__(ClientDeltaSlab)
    s.dtype, s.num_clients, s.num_params = torch.float32, K, 8
    return s


def test_select_keyword_on_every_surface():
    from fedjax_amd import aggregators

    trees = [{"w": torch.zeros(3)} for _ in range(7)]
    slab = _bare_slab(7)
    for bogus in ("bogus", "Device", None, 1, True):
        with pytest.raises(ValueError, match="select must be"):
            tree_util.tree_bulyan(trees, 1, select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            slab.bulyan(1, select=bogus)
        with pytest.raises(ValueError, match="select must be"):
            aggregators.bulyan_aggregator(1, select=bogus)


def test_device_route_checks_its_arguments_as_the_host_route_does():
    """The same exceptions, raised before any launch."""
    from fedjax_amd import aggregators

    def both(call, exc, match):
        raised = []
        for select in ("host", "device"):
            with pytest.raises(exc, match=match) as info:
                call(select=select)
            raised.append((type(info.value), str(info.value)))
        assert raised[0] == raised[1]

    trees = [{"w": torch.zeros(3)} for _ in range(7)]
    slab = _bare_slab(7)
    for call in (lambda f, **kw: tree_util.tree_bulyan(trees, f, **kw), lambda f, **kw: slab.bulyan(f, **kw)):
        both(lambda **kw: call(True, **kw), TypeError, "num_byzantine must be an int")
        both(lambda **kw: call(1.0, **kw), TypeError, "num_byzantine must be an int")
        both(lambda **kw: call(-1, **kw), ValueError, "num_byzantine must be >= 0")
        both(lambda **kw: call(2, **kw), ValueError, "4f \\+ 3")
    many = [{"w": torch.zeros(1)} for _ in range(200)]
    both(lambda **kw: tree_util.tree_bulyan(many, 1, **kw), ValueError, "K - 2f <= 128")
    both(lambda **kw: _bare_slab(200).bulyan(1, **kw), ValueError, "K - 2f <= 128")
    both(lambda **kw: _bare_slab(1025).bulyan(1, **kw), ValueError, "1024")
    half = _bare_slab(7)
    half.dtype = torch.bfloat16
    both(lambda **kw: half.bulyan(1, **kw), TypeError, "float32 slab")
    with pytest.raises(TypeError):
        aggregators.bulyan_aggregator(True, select="device")
    with pytest.raises(ValueError):
        aggregators.bulyan_aggregator(-1, select="device")
    assert tree_util.tree_bulyan([], 0, select="device") is None
    agg = aggregators.bulyan_aggregator(1, select="device")
    mean, state = agg.apply(iter([]), agg.init())
    assert mean is None and isinstance(state, aggregators.DeviceBulyanAggregatorState) and state.client_ids == ()


def test_select_wrappers_check_before_the_library_is_touched():
    from fedjax_amd import kernels

    G = torch.zeros(7, 7, dtype=torch.float64)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.bulyan_select_device(G, 1)
    with pytest.raises(ValueError, match="float64"):
        kernels.bulyan_select_device(G.float(), 1)
    with pytest.raises(ValueError, match="1024"):
        kernels.bulyan_select_device(torch.zeros(1025, 1025, dtype=torch.float64), 1)
    with pytest.raises(ValueError, match="4f \\+ 3"):
        kernels.check_bulyan_args(7, 2)
    with pytest.raises(ValueError, match="K - 2f <= 128"):
        kernels.check_bulyan_args(200, 1)
    with pytest.raises(TypeError, match="num_byzantine must be an int"):
        kernels.check_bulyan_args(7, True)
    assert kernels.check_bulyan_args(252, 62) == 62
    ints = torch.zeros(5, dtype=torch.int32)
    tables = kernels.DeviceRowTables(ints[:3], ints[3], ints[4], torch.zeros((), dtype=torch.float32), 3)
    x = torch.zeros(7, 8)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.meamed_dense_device(x, tables)
    with pytest.raises(TypeError, match="float32"):
        kernels.meamed_dense_device(x.double(), tables)
    with pytest.raises(ValueError, match="M_max"):
        kernels.meamed_dense_device(x, tables._replace(M_max=0))
    with pytest.raises(ValueError, match="M_max"):
        kernels.meamed_dense_device(x, tables._replace(M_max=129))
    with pytest.raises(ValueError, match="M_max must be <= K"):
        kernels.meamed_dense_device(x[:2], tables)
    with pytest.raises(ValueError, match="tables.rows"):
        kernels.meamed_dense_device(x, tables._replace(rows=ints[:2]))
    with pytest.raises(ValueError, match="tables.count"):
        kernels.meamed_dense_device(x, tables._replace(count=torch.zeros((), dtype=torch.int64)))
    image = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(TypeError, match="image_all"):
        kernels.meamed_ptrs_device(image.int(), image, 1, 7, 1, tables)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.meamed_ptrs_device(image[:3], image, 1, 7, 1, tables)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.meamed_ptrs_device(image, image[:4], 1, 7, 1, tables)


def test_surface_and_symbols():
    from fedjax_amd import _lib, aggregators, kernels

    assert _lib.ABI_VERSION == 4  # additions only
    for sym in ("fjagg_bulyan_select", "fjagg_bulyan_select_workspace_bytes", "fjagg_meamed_dense_dev",
                "fjagg_meamed_ptrs_dev"):
        assert sym in _lib.SYMBOLS
        assert isinstance(getattr(_lib.load(), sym), ctypes._CFuncPtr)
    assert tree_util.DeviceBulyanResult._fields == ("mean", "selected", "count", "keep", "step_scores", "gram")
    assert "DeviceBulyanResult" in tree_util.__all__
    assert kernels.DeviceRowTables._fields == ("rows", "count", "keep", "scale", "M_max")
    assert callable(kernels.bulyan_select_device) and callable(kernels.meamed_dense_device)
    assert callable(kernels.meamed_ptrs_device)
    assert aggregators.DeviceBulyanAggregatorState().client_ids == ()
