"""The numpy restatement of the coordinate-wise trimmed mean and median
(tests/robust_mean_ref.py) pinned against np.median, the sequential mean, Byzantine rows and a
hand-worked tie; and the product's host surface: the trim arithmetic, every refusal before the
library is touched, the aggregators, the symbols. No GPU needed."""
import numpy as np
import pytest
import torch

from tests import robust_mean_ref as ref

F32 = np.float32
KS = [1, 2, 3, 4, 5, 8, 9, 17, 64, 127, 128]


def distinct_finite(K, P, seed):
    """float32 [K, P], finite, all values of a column distinct."""
    rng = np.random.RandomState(seed)
    x = np.stack([rng.permutation(4 * K)[:K] for _ in range(P)], axis=1).astype(F32)
    return (x * F32(0.37) - F32(K)).astype(F32)


# ------------------------------------------------------------------ the restatement pins itself
@pytest.mark.parametrize("K", KS)
def test_median_is_np_median_bitwise(K):
    x = distinct_finite(K, 41, K)
    want = np.median(x, axis=0).astype(F32)
    assert ref.canon(ref.median(x)).tolist() == ref.canon(want).tolist()


@pytest.mark.parametrize("K", KS)
def test_no_trim_is_the_sequential_mean_bitwise(K):
    rng = np.random.RandomState(K)
    x = rng.standard_normal((K, 33)).astype(F32)
    s = x[0].copy()
    for k in range(1, K):
        s = (s + x[k]).astype(F32)
    want = (s * F32(1.0 / float(K))).astype(F32)
    assert ref.trimmed_mean(x, 0).view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_no_trim_is_the_oracle_tree_mean():
    from oracle import tree_util_ref as oracle

    rng = np.random.RandomState(3)
    x = rng.standard_normal((9, 17)).astype(F32)
    want = oracle.tree_mean([(x[k], 1) for k in range(9)])
    assert ref.trimmed_mean(x, 0).view(np.uint32).tolist() == np.asarray(want).view(np.uint32).tolist()


def test_byzantine_rows_are_trimmed():
    rng = np.random.RandomState(7)
    x = rng.standard_normal((10, 29)).astype(F32)
    x[1] = np.nan
    x[4] = np.array([0xFFC00000], np.uint32).view(F32)[0]  # -NaN
    x[6] = -np.inf
    x[8] = F32(3e38)
    got = ref.trimmed_mean(x, 2)
    assert np.isfinite(got).all()
    good = np.delete(x, [1, 4, 6, 8], axis=0)
    assert (got >= good.min(0)).all() and (got <= good.max(0)).all()
    # the order of item 1: -NaN and -inf at the bottom, 3e38 and +NaN at the top
    keep = ref.kept_mask(x, 2)
    assert not keep[[1, 4, 6, 8]].any() and keep.sum(0).tolist() == [6] * 29
    # a third bad row on one side is one more than t = 2 removes: the trim count is the guarantee
    x[2] = -np.inf
    assert np.isneginf(ref.trimmed_mean(x, 2)).all()


def test_key_order():
    bits = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
                     0x3F800000, 0x7F800000, 0x7F800001, 0x7FC00000], np.uint32)  # -NaN .. -0 +0 .. +NaN, ascending
    k = ref.keys(bits.view(F32))
    assert (np.diff(k.astype(np.int64)) > 0).all()


def test_hand_worked_tie():
    """K = 5, values [1, 1, 1, 2, 0], t = 1. Sorted by (key, client): 0(c4) 1(c0) 1(c1) 1(c2) 2(c3).
    Rank 0 (client 4) and rank 4 (client 3) go; clients 0, 1, 2 stay. L = U = 1: nL = 0 copies of L
    below the cut, nU = 0 above, so all three 1s are kept."""
    x = np.array([[1], [1], [1], [2], [0]], F32)
    want = np.array([[True], [True], [True], [False], [False]])
    assert ref.kept_mask(x, 1).tolist() == want.tolist()
    assert ref.kept_mask_by_counts(x, 1).tolist() == want.tolist()
    assert ref.trimmed_mean(x, 1).tolist() == [1.0]
    """The same values at t = 2: ranks 2..2, one value. Sorted: 0(c4) 1(c0) | 1(c1) | 1(c2) 2(c3): of the
    three equal 1s the index rule drops client 0 (below) and client 2 (above) and keeps client 1."""
    want2 = np.array([[False], [True], [False], [False], [False]])
    assert ref.kept_mask(x, 2).tolist() == want2.tolist()
    assert ref.kept_mask_by_counts(x, 2).tolist() == want2.tolist()
    # which equal value is dropped shows in the bits once the values differ in sign of zero
    z = np.array([[0.0], [-0.0], [-0.0], [1.0], [-1.0]], F32)  # sorted: -1(c4) -0(c1) -0(c2) +0(c0) 1(c3)
    assert ref.kept_mask(z, 1).ravel().tolist() == [True, True, True, False, False]
    assert ref.kept_mask(z, 2).ravel().tolist() == [False, False, True, False, False]
    assert np.signbit(ref.trimmed_mean(z, 2)).tolist() == [True]  # a single kept -0 stays -0


@pytest.mark.parametrize("K", [2, 3, 5, 8, 16, 33])
def test_count_rule_is_the_stable_argsort_rule(K):
    rng = np.random.RandomState(100 + K)
    for t in range((K - 1) // 2 + 1):
        x = ref.mixed_data(rng, K, 40, special=0.15, ties=0.5)
        assert np.array_equal(ref.kept_mask(x, t), ref.kept_mask_by_counts(x, t)), (K, t)


def test_sweep_cases_are_all_valid_and_run():
    cases = ref.sweep_cases()
    assert len(cases) == 60 and ref.sweep_cases() == cases  # seeded
    for K, t, leaves, seed in cases:
        assert 1 <= K <= ref.K_MAX and 0 <= 2 * t < K and 1 <= len(leaves) <= 4
        x = ref.mixed_data(np.random.RandomState(seed), K, max(sum(leaves), 1))
        got = ref.trimmed_mean(x, t)
        assert got.shape == (max(sum(leaves), 1),) and got.dtype == F32
    assert {K for K, *_ in cases} >= {1, 2, 16, 17, 64, 65, 128}
    assert any(0 in lv for _, _, lv, _ in cases)


# ------------------------------------------------------------------------- the product's surface
def test_fraction_to_count_arithmetic():
    from fedjax_amd import kernels

    tc = kernels.trim_count
    assert [tc(0.25, K) for K in (4, 8, 10, 128)] == [1, 2, 2, 32]
    assert [tc(0.125, K) for K in (8, 10, 16, 128)] == [1, 1, 2, 16]
    assert [tc(0.1, K) for K in (10, 20, 128)] == [1, 2, 12]
    assert tc(0.29, 100) == 28  # 0.29 * 100 = 28.999999999999996 in double: floor, as documented
    assert tc(0.0, 1) == 0 and tc(0, 1) == 0 and tc(0.49, 2) == 0
    assert tc(3, 7) == 3 and tc(np.int64(2), 5) == 2 and tc(np.float32(0.25), 8) == 2
    for K in (1, 2, 10, 128):
        for trim in (0, 0.1, 0.25, 0.49, (K - 1) // 2):
            assert tc(trim, K) == ref.trim_count(trim, K)


def test_trim_refusals_name_the_limit():
    from fedjax_amd import kernels

    with pytest.raises(ValueError, match="128"):
        kernels.trim_count(0, 129)
    with pytest.raises(ValueError, match="2t < K"):
        kernels.trim_count(2, 4)
    with pytest.raises(ValueError, match="2t < K"):
        kernels.trim_count(-1, 4)
    for beta in (0.5, 0.7, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 0.5\)"):
            kernels.trim_count(beta, 10)
    for bad in (True, False, np.bool_(True), "0.1", None):
        with pytest.raises(TypeError):
            kernels.trim_count(bad, 10)


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


def test_kernel_wrappers_refuse_before_the_library(no_library):
    from fedjax_amd import kernels

    x = torch.zeros(4, 8)
    with pytest.raises(TypeError, match="float32"):
        kernels.trim_dense(x.to(torch.bfloat16), 1)
    with pytest.raises(TypeError, match="float32"):
        kernels.trim_dense(x.to(torch.int32), 1)
    with pytest.raises(ValueError, match="128"):
        kernels.trim_dense(torch.zeros(129, 2), 1)
    with pytest.raises(ValueError, match="2t < K"):
        kernels.trim_dense(x, 2)
    with pytest.raises(ValueError, match="2t < K"):
        kernels.trim_dense(x, -1)
    with pytest.raises(TypeError):
        kernels.trim_dense(x, True)
    with pytest.raises(TypeError):
        kernels.trim_dense(x, 0.25)  # the wrapper takes a count; fractions are the callers'
    with pytest.raises(ValueError, match="unit column stride"):
        kernels.trim_dense(torch.zeros(4, 16)[:, ::2], 1)
    with pytest.raises(ValueError, match="column"):
        kernels.trim_dense(torch.zeros(4, 0), 1)
    with pytest.raises(ValueError, match="out must be"):
        kernels.trim_dense(x, 1, out=torch.zeros(7))
    with pytest.raises(ValueError, match="device tensors"):
        kernels.trim_dense(x, 1)  # valid arguments, host tensor: still no library call
    img = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError, match="128"):
        kernels.trim_ptrs(img, 1, 129, 1, 0, None)
    with pytest.raises(ValueError, match="2t < K"):
        kernels.trim_ptrs(img, 1, 4, 1, 2, None)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.trim_ptrs(img, 0, 4, 1, 1, None)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.trim_ptrs(img, 8, 4, 20, 1, None)  # the image is shorter than the plan says
    with pytest.raises(TypeError):
        kernels.trim_ptrs(img.to(torch.int32), 1, 4, 1, 1, None)


def test_slab_and_tree_refuse_before_the_library(no_library):
    from fedjax_amd import tree_util

    with pytest.raises(TypeError, match="float32"):
        _fake_slab(4, torch.bfloat16).trimmed_mean(1)
    with pytest.raises(TypeError, match="float32"):
        _fake_slab(4, torch.bfloat16).median()
    with pytest.raises(ValueError, match="128"):
        _fake_slab(129).trimmed_mean(1)
    with pytest.raises(ValueError, match="128"):
        _fake_slab(129).median()
    with pytest.raises(ValueError, match="2t < K"):
        _fake_slab(4).trimmed_mean(2)
    with pytest.raises(ValueError, match=r"\[0, 0.5\)"):
        _fake_slab(4).trimmed_mean(0.5)
    with pytest.raises(TypeError, match="bool"):
        _fake_slab(4).trimmed_mean(True)

    trees = [{"w": np.zeros(3, F32)} for _ in range(4)]
    assert tree_util.tree_trimmed_mean([], 1) is None and tree_util.tree_median(iter([])) is None
    with pytest.raises(ValueError, match="2t < K"):
        tree_util.tree_trimmed_mean(trees, 2)
    with pytest.raises(ValueError, match=r"\[0, 0.5\)"):
        tree_util.tree_trimmed_mean(iter(trees), 0.5)
    with pytest.raises(TypeError, match="bool"):
        tree_util.tree_trimmed_mean(trees, False)
    with pytest.raises(ValueError, match="128"):
        tree_util.tree_trimmed_mean([{"w": np.zeros(1, F32)}] * 129, 1)
    with pytest.raises(ValueError, match="128"):
        tree_util.tree_median([{"w": np.zeros(1, F32)}] * 129)
    for bad in (torch.zeros(3, dtype=torch.bfloat16), np.zeros(3, np.int32)):
        with pytest.raises(TypeError, match="float32"):
            tree_util.tree_trimmed_mean([{"w": bad}] * 4, 1)
        with pytest.raises(TypeError, match="float32"):
            tree_util.tree_median([{"w": bad}] * 3)


def test_c_entries_refuse_on_the_host():
    """The same refusals in the C entry points, with nothing launched (no GPU here)."""
    from fedjax_amd import _lib

    lib = _lib.load()
    dense = lambda dt, ld, K, P, t, fl, x=16, y=16: lib.fjagg_trim_dense(dt, x, ld, K, P, t, 1.0, y, fl, None)
    assert dense(_lib.F32, 8, 129, 8, 1, 0) == -3 and b"128" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 0, 8, 0, 0) == -1
    assert dense(_lib.F32, 8, 4, 8, 2, 0) == -1 and b"2t < K" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 4, 8, -1, 0) == -1
    assert dense(_lib.BF16, 8, 4, 8, 1, 0) == -3 and b"float32" in lib.fjagg_last_error()
    assert dense(_lib.I32, 8, 4, 8, 1, 0) == -3
    assert dense(_lib.F32, 8, 4, 8, 1, 0, x=None) == -1 and b"null" in lib.fjagg_last_error()
    assert dense(_lib.F32, 8, 4, 8, 1, 0, y=None) == -1
    assert dense(_lib.F32, 8, 4, 0, 1, 0) == -1
    assert dense(_lib.F32, 7, 4, 8, 1, 0) == -1 and b"ld" in lib.fjagg_last_error()
    assert dense(_lib.F32, 1 << 29, 4, (1 << 28) + 1, 1, 0) == -3 and b"1 GiB" in lib.fjagg_last_error()
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, _lib.UNALIGNED,
               1 << 8, 1 << 16):
        assert dense(_lib.F32, 8, 4, 8, 1, fl) == -3, fl
    img = np.zeros(64, np.int64)
    ptrs = lambda dt, L, K, nblk, t, fl, im=img.ctypes.data: lib.fjagg_trim_ptrs(dt, im, L, K, nblk, t, 1.0, fl, None)
    assert ptrs(_lib.F32, 1, 129, 1, 1, 0) == -3
    assert ptrs(_lib.F32, 1, 4, 1, 2, 0) == -1
    assert ptrs(_lib.BF16, 1, 4, 1, 1, 0) == -3
    assert ptrs(_lib.F32, 0, 4, 1, 1, 0) == -1 and b"bad plan" in lib.fjagg_last_error()
    assert ptrs(_lib.F32, 1, 4, 0, 1, 0) == -1
    assert ptrs(_lib.F32, 1, 4, 1, 1, 0, im=None) == -1
    for fl in (_lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, 1 << 8):
        assert ptrs(_lib.F32, 1, 4, 1, 1, fl) == -3, fl


def test_aggregators_state_and_exports():
    import fedjax_amd
    from fedjax_amd import aggregators, slab, tree_util

    for name in ("trimmed_mean_aggregator", "median_aggregator", "RobustAggregatorState"):
        assert hasattr(aggregators, name), name
    for agg in (aggregators.trimmed_mean_aggregator(0.1), aggregators.trimmed_mean_aggregator(2),
                aggregators.median_aggregator()):
        assert isinstance(agg, aggregators.Aggregator)
        state = agg.init()
        assert isinstance(state, aggregators.RobustAggregatorState)
        assert fedjax_amd.pytree.leaves_of(state) == []
        got, state2 = agg.apply(iter([]), state)  # no clients: None, the state unchanged
        assert got is None and state2 is state
    for bad in (True, "x", None):
        with pytest.raises(TypeError):
            aggregators.trimmed_mean_aggregator(bad)
    for bad in (0.5, -0.1, -1):
        with pytest.raises(ValueError):
            aggregators.trimmed_mean_aggregator(bad)
    for name in ("tree_trimmed_mean", "tree_median"):
        assert name in tree_util.__all__ and callable(getattr(tree_util, name))
    for name in ("trimmed_mean", "median"):
        assert callable(getattr(slab.ClientDeltaSlab, name))
    assert "weights" in slab.ClientDeltaSlab.trimmed_mean.__doc__.lower()
    assert "ignores the weights" in aggregators.median_aggregator.__doc__.lower()


def test_symbols_and_abi():
    from fedjax_amd import _lib, kernels

    assert _lib.ABI_VERSION == 4
    for sym in ("fjagg_trim_dense", "fjagg_trim_ptrs"):
        assert sym in _lib.SYMBOLS
    assert callable(kernels.trim_dense) and callable(kernels.trim_ptrs)
    assert kernels.TRIM_MAX_CLIENTS == ref.K_MAX == 128
