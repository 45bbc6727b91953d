"""The numpy restatement of the grouped weighted mean (tests/grouped_mean_ref.py) against the
reference's own known answer and the IEEE edge cases. No GPU needed; the product is touched only
to show that it exposes the API the GPU tests exercise and refuses bad input on the host."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import tree_util_ref as oracle
from tests import algorithms_restated as ar
from tests import grouped_mean_ref as ref

F32 = np.float32

# hyp_cluster_test.py:366-403: clusters [1, -1, 3.14]; clients 0, 1, 4 chose cluster 0, clients
# 2, 3 cluster 1, nobody cluster 2; a client's weight is its number of examples
KAT_PARAMS = [1., -1., 3.14]
KAT_CLIENTS = ar._HC_CLIENTS + [(b"4", np.array([-0.1], F32))]
KAT_IDS = [0, 0, 1, 1, 0]


def kat_inputs():
    deltas = np.array([[ar._hc_delta(KAT_PARAMS[g], x)] for (_, x), g in zip(KAT_CLIENTS, KAT_IDS)], dtype=F32)
    weights = [len(x) for _, x in KAT_CLIENTS]
    return deltas, weights


def test_reference_kat():
    deltas, weights = kat_inputs()
    got = ref.grouped_mean_ref(deltas, weights, KAT_IDS, 3)
    npt.assert_allclose(got[0], [(-0.1 + 0.1 * 2 + 1.1) / 4], rtol=1e-7)
    npt.assert_allclose(got[1], [(0.1 - 0.1 * 3) / 4], rtol=1e-6)  # the reference's own rtol
    assert got[2] is None
    # and it is the running-sum loop on the oracle, bit for bit
    want = ar.hyp_cluster_expectation_round(oracle, lambda a: a, np.asarray, None)
    for g in range(2):
        assert ref.bits(got[g]).tolist() == ref.bits(np.ravel(want["cluster_deltas"][g])).tolist()
    assert want["empty_cluster"] is None


def test_signed_zero_sum_starts_from_plus_zero():
    x = np.full((2, 3), -0.0, dtype=F32)
    got = ref.grouped_mean_ref(x, [2, 3], [0, 0], 1)[0]
    assert not np.signbit(got).any() and (got == 0).all()
    mean = oracle.tree_mean([(x[0], 2), (x[1], 3)])
    assert np.signbit(mean).all()  # tree_mean copies the first product: -0 stays


def test_zero_negative_and_nan_totals_give_none():
    x = np.ones((4, 2), dtype=F32)
    assert ref.grouped_mean_ref(x, [2, -2, 1, 1], [0, 0, 1, 1], 2)[0] is None
    assert ref.grouped_mean_ref(x, [1, -2, 1, 1], [0, 0, 1, 1], 2)[0] is None
    assert ref.grouped_mean_ref(x, [1.0, float("nan"), 1, 1], [0, 0, 1, 1], 2)[0] is None
    assert ref.grouped_mean_ref(x, [2, -2, 1, 1], [0, 0, 1, 1], 2)[1] is not None


def test_no_group_client_is_never_indexed():
    x = np.array([[1.0], [np.nan], [3.0]], dtype=F32)
    got = ref.grouped_mean_ref(x, [1, 1, 1], [0, -1, 0], 1)[0]
    assert got.tolist() == [2.0]


def test_seeded_ids_force_the_edges():
    for K in (5, 9, 33):
        ids = ref.seeded_ids(K, 5, K)
        counts = np.bincount(ids[ids >= 0], minlength=5)
        assert (ids == -1).sum() >= 2 and (counts == 1).any() and (counts == 0).any()


def test_product_exposes_the_grouped_mean_api():
    from fedjax_amd import _lib, kernels, slab, tree_util

    for obj, name in ((kernels, "grouped_sum_dense"), (tree_util, "tree_grouped_mean"),
                      (slab.ClientDeltaSlab, "grouped_mean")):
        assert callable(getattr(obj, name)), name
    assert "tree_grouped_mean" in tree_util.__all__
    assert _lib.ABI_VERSION == 4
    for sym in ("fjagg_wsum_group_dense", "fjagg_wsum_group_ptrs"):
        assert sym in _lib.SYMBOLS


def test_no_clients_and_bad_ids_on_the_host():
    from fedjax_amd import tree_util

    assert tree_util.tree_grouped_mean([], [], 3) == [None, None, None]
    pairs = [(np.zeros(2, F32), 1.0), (np.zeros(2, F32), 2.0)]
    for bad in ([0], [0, 1, 0], [0.0, 1.0], [0, 3], [0, -2], [True, False], [[0, 1]]):
        with pytest.raises(ValueError):
            tree_util.tree_grouped_mean(pairs, bad, 3)
    with pytest.raises(ValueError):
        tree_util.tree_grouped_mean(pairs, [0, 0], 0)


def test_dense_shape_choice_on_the_host():
    """fjagg_group_dense_shape is a pure host function: 0 = element units (something is not
    16-byte aligned), else the variant 2 / 5 / 12 from the unit count and the mean member count."""
    from fedjax_amd import _lib

    shape = _lib.load().fjagg_group_dense_shape
    assert "fjagg_group_dense_shape" in _lib.SYMBOLS
    P = 600_003
    assert shape(16, P + 1, P, 40, 3, 3, 32, P + 1) == 5        # 150 000 units, 13 members per group
    assert shape(16, P + 1, P, 40, 3, 3, 32, P) == 0            # the result's row stride is not aligned
    assert shape(16, P + 1, P, 40, 1, 1, 32, P) == 5            # ... which one group does not use
    assert shape(16, P + 1, P, 40, 3, 1, 32, P) == -1           # more non-empty groups than groups
    assert shape(16, P, P, 40, 3, 3, 32, P + 1) == 0            # the slab's row stride
    assert shape(20, P + 1, P, 40, 3, 3, 32, P + 1) == 0        # the slab's base
    assert shape(16, P + 1, P, 21, 3, 3, 32, P + 1) == 2        # 7 members per group
    assert shape(16, 1 << 20, 1 << 20, 40, 3, 3, 32, 1 << 20) == 12
    assert shape(16, 1 << 19, (1 << 19) - 4, 40, 3, 3, 32, 1 << 19) == 2   # just under 128 Ki units
    assert shape(16, 8, 3, 2, 1, 1, 32, 8) == 0                 # P < 4
    assert shape(16, 8, 9, 2, 1, 1, 32, 16) == -1               # ld < P


def test_raw_entry_points_refuse_on_the_host():
    """Unsupported flags and dtypes return FJAGG_EUNSUPPORTED (-3) and malformed tables
    FJAGG_EINVAL (-1) before any HIP call: the dummy device pointers are never touched."""
    from fedjax_amd import _lib

    lib = _lib.load()
    order = np.array([0, 1], dtype=np.int32)
    seg = np.array([0, 1, 2], dtype=np.int32)

    def dense(dt=_lib.F32, fl=0, K=2, M=2, G=2, order=order, seg=seg):
        return lib.fjagg_wsum_group_dense(dt, 16, 8, K, 8, M, G, 16, 16, 16, 16, None, order.ctypes.data,
                                          seg.ctypes.data, 16, 8, fl, None)

    def ptrs(dt=_lib.F32, fl=0, K=2, M=2, G=2, seg=seg):
        return lib.fjagg_wsum_group_ptrs(dt, 16, 1, K, M, G, 1, 16, 16, 16, None, seg.ctypes.data, fl, None)

    for fl in (_lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.ACCUMULATE, _lib.UNBALANCED, 12 << 8):
        assert dense(fl=fl) == -3, fl
        assert ptrs(fl=fl) == -3, fl
    for dt in (_lib.BF16, _lib.I32):
        assert dense(dt=dt) == -3 and ptrs(dt=dt) == -3
    assert dense(fl=_lib.UNALIGNED) == -3  # the pytree entry alone takes FJAGG_UNALIGNED
    # malformed tables
    for bad_seg in ([0, 2, 1], [0, 1, 1], [1, 1, 2], [0, 1, 3]):  # not monotone / ends before or past M / seg[0]
        s = np.array(bad_seg, dtype=np.int32)
        assert dense(seg=s) == -1, bad_seg
        assert ptrs(seg=s) == -1, bad_seg
    assert dense(G=0) == -1 and ptrs(G=0) == -1
    assert b"G must be >= 1" in lib.fjagg_last_error()
    for bad_order in ([0, 2], [-1, 1]):
        assert dense(order=np.array(bad_order, dtype=np.int32)) == -1, bad_order
    assert b"outside" in lib.fjagg_last_error()
