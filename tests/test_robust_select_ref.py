"""Host side of the Gram-matrix aggregates (Krum / multi-Krum, the smoothed-Weiszfeld geometric
median): fedjax_amd.robust on an exact float64 Gram against restatements that work on the
vectors and use no Gram (tests/robust_select_ref.py); unusable clients; argument validation; the
library's host-side refusals; the public surface. No GPU needed."""
import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, robust
from tests import robust_select_ref as ref

KRUM_KS = [3, 5, 9, 16, 33]


def int_vectors(K, P, seed, twins=False):
    """Small-integer client vectors: their float64 Gram and all squared distances are exact."""
    x = np.random.RandomState(seed).randint(-7, 8, size=(K, P)).astype(np.float64)
    if twins and K >= 3:
        x[K - 1] = x[1]  # two identical clients: equal scores, distance 0
    return x


def krum_cases():
    for K in KRUM_KS:
        for f in range((K - 3) // 2 + 1):
            yield K, f


# ------------------------------------------------------------------ Krum, exactly
@pytest.mark.parametrize("K,f", list(krum_cases()))
@pytest.mark.parametrize("twins", [False, True])
def test_krum_equals_brute_force_exactly(K, f, twins):
    x = int_vectors(K, 37, 100 * K + f, twins)
    G = x @ x.T
    want_scores = ref.krum_scores(x, f)
    got_scores = robust.krum_scores(G, f)
    assert got_scores.dtype == np.float64 and got_scores.tolist() == want_scores.tolist()
    for m in sorted({1, 2, K - f} & set(range(1, K - f + 1))):
        want, _ = ref.krum_select(x, f, m)
        got = robust.krum_select(G, f, m)
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), (K, f, m)


def test_krum_ties_go_to_the_lower_index():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [9.0, 9.0], [1.0, 0.0], [0.0, 0.0]])
    G = x @ x.T
    scores = robust.krum_scores(G, 0)  # K - f - 2 = 3 nearest
    assert scores[0] == scores[4] and scores[1] == scores[3]
    assert robust.krum_select(G, 0, 5).tolist() == ref.krum_select(x, 0, 5)[0].tolist()
    assert robust.krum_select(G, 0, 1).tolist() == [0]


def test_sq_distances():
    x = int_vectors(6, 11, 3)
    d2 = robust.sq_distances(x @ x.T)
    want = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    assert d2.tolist() == want.tolist() and (np.diagonal(d2) == 0).all()
    # rounding may push a tiny distance below zero: clamped
    G = np.array([[1.0, 1.0 + 1e-16], [1.0 + 1e-16, 1.0]])
    assert (robust.sq_distances(G) >= 0).all()


# ------------------------------------------------------------------ Weiszfeld on G against the direct form
@pytest.mark.parametrize("K,P", [(9, 257), (16, 1000), (33, 1027), (128, 4099)])
@pytest.mark.parametrize("T", [0, 1, 4, 8])
def test_weiszfeld_on_gram_equals_the_direct_form(K, P, T):
    rng = np.random.default_rng(K * 10007 + P)
    x = ref.outlier_data(rng, K, P, max(1, K // 5)).astype(np.float64)
    for alpha in (np.ones(K), rng.uniform(0.5, 3.0, K)):
        want, _ = ref.weiszfeld(x, alpha, 1e-6, T)
        got, d = robust.weiszfeld_weights(x @ x.T, alpha, 1e-6, T)
        assert got.dtype == np.float64 and d.shape == (K,)
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"K={K} P={P} T={T}: relative weight difference {rel:.3g}")
        assert rel <= 1e-12
        assert abs(got.sum() - 1.0) <= 1e-14
    if T:
        assert got[K - 1] < got[0]  # an outlier is down-weighted


def test_weiszfeld_default_weights_are_uniform():
    x = int_vectors(7, 5, 1)
    a, d = robust.weiszfeld_weights(x @ x.T, None, 1e-6, 0)
    assert a.tolist() == [1.0 / 7] * 7 and d.tolist() == [0.0] * 7


def test_weiszfeld_smoothing_caps_the_weight_of_a_coincident_point():
    x = np.zeros((5, 3))
    x[4] = 1.0  # four clients at the origin: distance 0 from the iterate after one step
    a, _ = robust.weiszfeld_weights(x @ x.T, None, 1e-3, 6)
    assert np.isfinite(a).all() and a[:4].min() > a[4]


# ------------------------------------------------------------------ unusable clients
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_diagonal_is_unusable(bad):
    x = int_vectors(9, 13, 5)
    G = x @ x.T
    G[3, :] = bad
    G[:, 3] = bad
    ok = robust.usable(G)
    assert ok.tolist() == [k != 3 for k in range(9)]
    d2 = robust.sq_distances(G)
    assert np.isinf(d2[3, [0, 1, 2, 4]]).all() and np.isinf(d2[[0, 1, 2, 4], 3]).all() and d2[3, 3] == 0
    scores = robust.krum_scores(G, 1)
    assert np.isinf(scores[3]) and np.isfinite(np.delete(scores, 3)).all()
    xz = x.copy()
    xz[3] = np.nan
    assert scores.tolist() == ref.krum_scores(xz, 1).tolist()
    assert 3 not in robust.krum_select(G, 1, 8).tolist()
    assert len(robust.krum_select(G, 1, 8)) == 8
    a, d = robust.weiszfeld_weights(G, None, 1e-6, 3)
    assert a[3] == 0.0 and np.isinf(d[3]) and abs(a.sum() - 1.0) <= 1e-14
    want, _ = ref.weiszfeld(np.delete(x, 3, axis=0), np.ones(8), 1e-6, 3)
    assert np.abs(np.delete(a, 3) - want).max() <= 1e-12 * want.max()


def test_too_many_unusable_clients_leave_fewer_than_m():
    x = int_vectors(5, 7, 2)
    G = x @ x.T
    for k in (0, 1):
        G[k, :] = np.nan
        G[:, k] = np.nan
    # K - f - 2 = 3 neighbours, but a usable client has only 2 usable ones: every score is inf
    assert robust.krum_select(G, 0, 3).tolist() == []
    assert len(robust.krum_select(G, 1, 4)) == 3  # 2 neighbours suffice


def test_all_unusable():
    G = np.full((5, 5), np.nan)
    assert robust.krum_select(G, 1, 2).tolist() == [] and np.isinf(robust.krum_scores(G, 1)).all()
    a, d = robust.weiszfeld_weights(G, None, 1e-6, 4)
    assert a.tolist() == [0.0] * 5 and np.isinf(d).all()


# ------------------------------------------------------------------ argument validation
def test_argument_validation():
    G = np.eye(7)
    for f in (True, 1.0, "1", None):
        with pytest.raises(TypeError):
            robust.krum_scores(G, f)
    for m in (True, 1.0, None):
        with pytest.raises(TypeError):
            robust.krum_select(G, 1, m)
    with pytest.raises(ValueError):
        robust.krum_scores(G, -1)
    with pytest.raises(ValueError):
        robust.krum_scores(G, 3)  # K = 7 < 2 * 3 + 3
    robust.krum_scores(G, 2)  # K = 7 = 2 * 2 + 3
    with pytest.raises(ValueError):
        robust.krum_scores(np.eye(2), 0)
    for m in (0, -1, 6):  # K - f = 5
        with pytest.raises(ValueError):
            robust.krum_select(G, 2, m)
    robust.krum_select(G, 2, 5)
    with pytest.raises(ValueError):
        robust.krum_scores(np.zeros((3, 4)), 0)
    for nu in (0.0, -1e-6, np.nan, np.inf):
        with pytest.raises(ValueError):
            robust.weiszfeld_weights(G, None, nu, 1)
    with pytest.raises(TypeError):
        robust.weiszfeld_weights(G, None, True, 1)
    for alpha in ([1, 1, 1, 0, 1, 1, 1], [1, 1, 1, -2, 1, 1, 1], [1, 1, 1, np.nan, 1, 1, 1], [1, 1, 1, np.inf, 1, 1, 1]):
        with pytest.raises(ValueError):
            robust.weiszfeld_weights(G, alpha, 1e-6, 1)
    with pytest.raises(ValueError):
        robust.weiszfeld_weights(G, [1.0] * 6, 1e-6, 1)
    with pytest.raises(TypeError):
        robust.weiszfeld_weights(G, [True] * 7, 1e-6, 1)
    for it in (True, 1.5, None):
        with pytest.raises(TypeError):
            robust.weiszfeld_weights(G, None, 1e-6, it)
    with pytest.raises(ValueError):
        robust.weiszfeld_weights(G, None, 1e-6, -1)


# ------------------------------------------------------------------ the library refuses on the host
def test_gram_host_side_refusals_without_gpu():
    lib = _lib.load()
    x, g, ws = 4096, 8192, 12288  # never dereferenced: every call below is refused before a launch
    big = 1 << 40

    def dense(dt=_lib.F32, xp=x, ld=16, K=4, P=16, gp=g, wp=ws, wb=big, fl=0):
        return lib.fjagg_gram_dense(dt, xp, ld, K, P, gp, wp, wb, fl, None)

    def ptrs(dt=_lib.F32, img=x, L=2, K=4, nblk=3, gp=g, wp=ws, wb=big, fl=0):
        return lib.fjagg_gram_ptrs(dt, img, L, K, nblk, gp, wp, wb, fl, None)

    for call in (dense, ptrs):
        for dt in (_lib.BF16, _lib.I32):
            assert call(dt=dt) == -3 and b"float32" in lib.fjagg_last_error()
        for flag, word in ((_lib.ACCUMULATE, b"ACCUMULATE"), (_lib.NARROW, b"NARROW"), (_lib.HOST_TABLES, b"HOST_TABLES"),
                           (_lib.ZEROED_WS, b"ZEROED_WS"), (_lib.UNBALANCED, b"UNBALANCED"), (5 << 8, b"unsupported flags"),
                           (_lib.SCALE, b"unsupported flags"), (_lib.NONTEMPORAL, b"unsupported flags")):
            assert call(fl=flag) == -3 and word in lib.fjagg_last_error(), flag
        assert call(K=1025) == -3 and b"1024" in lib.fjagg_last_error()
        assert call(K=0) == -1 and b"K must be" in lib.fjagg_last_error()
        assert call(gp=None) == -1 and call(wp=None) == -1 and b"null" in lib.fjagg_last_error()
        assert call(wb=100) == -1 and b"workspace" in lib.fjagg_last_error()
    assert dense(fl=_lib.UNALIGNED) == -3  # rows need float32's alignment only: there is no such plan
    assert dense(xp=None) == -1 and ptrs(img=None) == -1
    assert dense(P=0) == -1 and dense(P=17) == -1 and b"ld" in lib.fjagg_last_error()
    assert dense(ld=1 << 29, P=(1 << 28) + 1) == -3 and b"1 GiB" in lib.fjagg_last_error()
    assert ptrs(nblk=0) == -1 and ptrs(L=0) == -1 and b"bad plan" in lib.fjagg_last_error()
    with pytest.raises(_lib.FjaggError):
        _lib.call("fjagg_gram_dense", _lib.BF16, x, 16, 4, 16, g, ws, big, 0, None)


def test_gram_workspace_and_chunk_sizing():
    lib = _lib.load()
    C = kernels.GRAM_CHAIN
    assert C == 256 and C & (C - 1) == 0 and 64 <= C <= 1024 and kernels.GRAM_MAX_CLIENTS == 1024
    block = 128 * 128 * 8
    for K, pairs in ((1, 1), (128, 1), (129, 3), (257, 6), (1024, 36)):
        for P in (1, C, 5 * C + 1, 20000, 4 << 20):
            cc = kernels.gram_chunk_columns(K, P)
            assert cc % C == 0 and cc >= C
            nchunks = -(-P // cc)
            assert lib.fjagg_gram_workspace_bytes(K, P, 0) == nchunks * pairs * block
            assert nchunks * pairs <= 512  # the workspace stays bounded: 64 MiB at the most
        assert lib.fjagg_gram_workspace_bytes(K, 0, 7) == min(7, max(1, 512 // pairs)) * pairs * block
    assert lib.fjagg_gram_workspace_bytes(0, 10, 0) < 0 and lib.fjagg_gram_workspace_bytes(4, 0, 0) < 0
    assert lib.fjagg_gram_chunk_columns(1025, 10) < 0
    with pytest.raises(ValueError):
        kernels.gram_chunk_columns(4, 0)


def test_wrappers_check_before_the_library_is_touched():
    x = torch.zeros(4, 16)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.gram_dense(x)
    with pytest.raises(TypeError, match="float32"):
        kernels.gram_dense(x.to(torch.bfloat16))
    with pytest.raises(ValueError):
        kernels.gram_dense(torch.zeros(16))
    with pytest.raises(ValueError):
        kernels.gram_dense(torch.zeros(4, 0))
    with pytest.raises(ValueError, match="1024"):
        kernels.gram_dense(torch.zeros(1025, 2))
    with pytest.raises(ValueError):
        kernels.gram_dense(torch.zeros(4, 16)[:, ::2])
    img = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(TypeError):
        kernels.gram_ptrs(img.to(torch.int32), 2, 4, 3)
    with pytest.raises(ValueError, match="bad plan"):
        kernels.gram_ptrs(img, 2, 4, 100)
    with pytest.raises(ValueError, match="1024"):
        kernels.gram_ptrs(img, 2, 1025, 3)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.gram_ptrs(img, 2, 4, 3)


# ------------------------------------------------------------------ the surface
def test_surface():
    import fedjax_amd
    from fedjax_amd import aggregators, tree_util
    from fedjax_amd.aggregators import aggregator

    for name in ("tree_gram", "tree_krum", "tree_geometric_median", "KrumResult", "GeometricMedianResult"):
        assert name in tree_util.__all__ and hasattr(tree_util, name)
    for name in ("usable", "sq_distances", "krum_scores", "krum_select", "weiszfeld_weights"):
        assert name in robust.__all__
    assert aggregators.krum_aggregator is aggregator.krum_aggregator
    assert aggregators.geometric_median_aggregator is aggregator.geometric_median_aggregator
    for name in ("gram", "krum", "geometric_median"):
        assert callable(getattr(fedjax_amd.ClientDeltaSlab, name))
    assert tree_util.KrumResult._fields == ("mean", "selected", "scores", "gram")
    assert tree_util.GeometricMedianResult._fields == ("median", "weights", "distances", "gram")
    for sym in ("fjagg_gram_dense", "fjagg_gram_ptrs", "fjagg_gram_workspace_bytes", "fjagg_gram_chunk_columns"):
        assert sym in _lib.SYMBOLS


def test_aggregator_arguments_and_empty_rounds():
    from fedjax_amd import aggregators, tree_util

    for bad in (True, 1.0, None):
        with pytest.raises(TypeError):
            aggregators.krum_aggregator(bad)
        with pytest.raises(TypeError):
            aggregators.krum_aggregator(1, bad)
        with pytest.raises(TypeError):
            aggregators.geometric_median_aggregator(iterations=bad)
    with pytest.raises(ValueError):
        aggregators.krum_aggregator(-1)
    with pytest.raises(ValueError):
        aggregators.krum_aggregator(1, 0)
    with pytest.raises(ValueError):
        aggregators.geometric_median_aggregator(nu=0.0)
    with pytest.raises(ValueError):
        aggregators.geometric_median_aggregator(iterations=-1)
    agg = aggregators.krum_aggregator(1, 2)
    state = agg.init()
    assert state.selected == () and state.scores == {}
    assert agg.apply(iter([]), state)[0] is None
    agg = aggregators.geometric_median_aggregator()
    assert agg.init().weights == {} and agg.apply([], agg.init())[0] is None
    assert tree_util.tree_gram([]) is None and tree_util.tree_krum(iter([]), 0) is None
    assert tree_util.tree_geometric_median([]) is None
    # the checks on K come before any pass over the deltas (host tensors would be refused later)
    trees = [{"w": torch.zeros(3)} for _ in range(4)]
    with pytest.raises(ValueError, match="2f \\+ 3"):
        tree_util.tree_krum(trees, 1)
    with pytest.raises(ValueError, match="num_selected"):
        tree_util.tree_krum(trees + trees, 1, 8)
    with pytest.raises(ValueError, match="weights"):
        tree_util.tree_geometric_median(trees, [1.0, 2.0])
    with pytest.raises(ValueError):
        tree_util.tree_geometric_median(trees, nu=-1.0)
