"""Krum / multi-Krum and the smoothed-Weiszfeld geometric median on the GPU, slab and pytrees:
the selection against restatements on the vectors (tests/robust_select_ref.py), the means bit for
bit against the grouped fold they are defined by, poisoned clients, and the aggregators."""
import functools

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import kernels, pytree, robust, slab as slab_mod, tree_util as tu
from tests import robust_select_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
TEMPLATE = {"a": (7, 11), "b": (150,), "one": (1,), "zero": (0,)}  # 228 parameters
SIZES = [77, 150, 1, 0]
P = sum(SIZES)


def template(shapes=TEMPLATE):
    return {k: torch.zeros(s) for k, s in shapes.items()}


def make_slab(x, dev, shapes=None):
    shapes = shapes or {"w": (x.shape[1],)}
    s = slab_mod.ClientDeltaSlab(template(shapes), x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return s


def make_clients(x, dev):
    """K client pytrees of TEMPLATE, every leaf its own allocation."""
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    return [{name: torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]], dtype=F32)).to(dev).view(shape)
             for l, (name, shape) in enumerate(TEMPLATE.items())} for k in range(x.shape[0])]


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def int_round(K):
    x = np.random.RandomState(K).randint(-7, 8, size=(K, P)).astype(F32)
    x.setflags(write=False)
    return x


def ids_of(selected, K):
    ids = np.full(K, -1, dtype=np.int64)
    ids[selected] = 0
    return ids


# ------------------------------------------------------------------ Krum
@pytest.mark.parametrize("K", [5, 9, 33, 128])
def test_krum_slab_and_pytrees(cuda, K):
    x = int_round(K)
    s = make_slab(x, cuda, TEMPLATE)
    clients = make_clients(x, cuda)
    for f in sorted({0, 1, (K - 3) // 2}):
        want_scores = ref.krum_scores(x, f)
        for m in sorted({1, 2, K - f}):
            want_sel, _ = ref.krum_select(x, f, m)
            got = s.krum(f, m)
            tree = tu.tree_krum(iter(clients), f, m)  # a one-shot iterable, consumed once
            for r, what in ((got, "slab"), (tree, "tree")):
                assert r.selected.tolist() == want_sel.tolist(), (what, K, f, m)
                assert r.scores.tolist() == want_scores.tolist(), (what, K, f, m)
                assert r.gram.dtype == torch.float64 and r.gram.is_cuda
            ids = ids_of(want_sel, K)
            want_mean = flat_of(s.grouped_mean([1] * K, ids, 1)[0])
            assert same_bits(flat_of(got.mean), want_mean)
            assert same_bits(flat_of(tree.mean), flat_of(tu.tree_grouped_mean([(c, 1) for c in clients], ids, 1)[0]))
            assert same_bits(flat_of(tree.mean), want_mean)
            assert tree.mean["zero"].numel() == 0 and tree.mean["a"].shape == (7, 11)
            if m == 1:  # the chosen client's row, up to the sign of a zero (the fold starts at +0)
                assert np.array_equal(flat_of(got.mean), x[want_sel[0]])
    assert same_bits(s.rows.cpu().numpy(), x)  # the inputs are never written
    assert same_bits(np.stack([flat_of(c) for c in clients]), x)


@pytest.mark.parametrize("poison", [np.nan, np.inf, 1e30])
def test_krum_ignores_poisoned_clients(cuda, poison):
    K, f, bad = 9, 2, [2, 6]
    x = np.array(int_round(K))
    x[bad] = poison
    zeroed = x.copy()
    zeroed[bad] = 0
    honest = np.array([k for k in range(K) if k not in bad])
    for m in (1, 3, K - f):
        want_sel, want_scores = ref.krum_select(x.astype(np.float64), f, m)
        assert not set(want_sel.tolist()) & set(bad)
        want = flat_of(make_slab(zeroed, cuda, TEMPLATE).grouped_mean([1] * K, ids_of(want_sel, K), 1)[0])
        s = make_slab(x, cuda, TEMPLATE)
        for r in (s.krum(f, m), tu.tree_krum(make_clients(x, cuda), f, m)):
            assert r.selected.tolist() == want_sel.tolist()
            assert r.scores[honest].tolist() == want_scores[honest].tolist()
            assert (r.scores[bad] > 1e50).all()  # inf: a non-finite value, or a squared norm that overflows
            mean = flat_of(r.mean)
            assert np.isfinite(mean).all() and same_bits(mean, want)
        plain = flat_of(s.mean([1] * K))
        assert not np.isfinite(plain).all() or np.abs(plain - want).max() > 1e20  # what the plain mean does


def test_krum_with_no_selectable_client(cuda):
    x = np.full((5, P), np.nan, dtype=F32)
    r = make_slab(x, cuda, TEMPLATE).krum(1, 2)
    assert r.mean is None and r.selected.tolist() == [] and np.isinf(r.scores).all()
    assert tu.tree_krum(make_clients(x, cuda), 1, 2).mean is None


# ------------------------------------------------------------------ geometric median
def fold_f32(x, w32):
    """The grouped fold in numpy: s = +0; s = s + x_k * w_k (float32, no FMA); s * f32(1 / W)."""
    W = 0
    for w in w32:
        W += w
    s = np.zeros(x.shape[1], dtype=F32)
    for k in range(x.shape[0]):
        s = (s + (x[k] * w32[k]).astype(F32)).astype(F32)
    return (s * F32(tu._inverse(W))).astype(F32)


@pytest.mark.parametrize("K,cols", [(9, 257), (16, 1000), (33, 1027)])
def test_geometric_median(cuda, K, cols):
    rng = np.random.default_rng(K * 10007 + cols)
    x = ref.outlier_data(rng, K, cols, max(1, K // 5))
    s = make_slab(x, cuda)
    clients = [{"w": torch.from_numpy(x[k]).to(cuda)} for k in range(K)]
    emulated = ref.chain_gram(x, kernels.GRAM_CHAIN)
    worst = 0.0
    for T in (0, 1, 4, 8):
        for alpha in (None, rng.uniform(0.5, 3.0, K).tolist()):
            got = s.geometric_median(alpha, iterations=T, nu=1e-6)
            G = got.gram.cpu().numpy()
            a, d = robust.weiszfeld_weights(G, alpha, 1e-6, T)
            assert got.weights.dtype == np.float32 and same_bits(got.weights, a.astype(F32))
            assert same_bits(got.distances, d)
            ids = np.zeros(K, dtype=np.int64)
            assert same_bits(flat_of(got.median), flat_of(s.grouped_mean(got.weights, ids, 1)[0]))
            tree = tu.tree_geometric_median(iter(clients), alpha, iterations=T, nu=1e-6)
            assert same_bits(tree.weights, robust.weiszfeld_weights(tree.gram.cpu().numpy(), alpha, 1e-6, T)[0].astype(F32))
            assert same_bits(flat_of(tree.median),
                             flat_of(tu.tree_grouped_mean(list(zip(clients, tree.weights)), ids, 1)[0]))
            # end to end against the direct form on the vectors, in float64
            _, want = ref.weiszfeld(x, np.ones(K) if alpha is None else alpha, 1e-6, T)
            # the yardstick: the same pipeline in numpy on the emulated float32-chain Gram
            ya, _ = robust.weiszfeld_weights(emulated, alpha, 1e-6, T)
            yard = np.abs(fold_f32(x, ya.astype(F32)) - want).max() / np.abs(want).max()
            for r, what in ((got, "slab"), (tree, "tree")):
                err = np.abs(flat_of(r.median).astype(np.float64) - want).max() / np.abs(want).max()
                print(f"K={K} P={cols} T={T} {what}: error {err:.3g}, yardstick {yard:.3g}")
                assert err <= 8 * yard
                worst = max(worst, err)
    print(f"K={K} P={cols}: largest end-to-end error {worst:.3g}")
    assert same_bits(s.rows.cpu().numpy(), x)  # the inputs are never written
    assert all(same_bits(c["w"].cpu().numpy(), x[k]) for k, c in enumerate(clients))


def test_geometric_median_drops_a_nan_client(cuda):
    K = 9
    x = ref.outlier_data(np.random.default_rng(3), K, 300, 2)
    x[4, 17] = np.nan
    for r in (make_slab(x, cuda).geometric_median(),
              tu.tree_geometric_median([{"w": torch.from_numpy(x[k]).to(cuda)} for k in range(K)])):
        assert r.weights[4] == 0 and np.isinf(r.distances[4]) and (np.delete(r.weights, 4) > 0).all()
        assert np.isfinite(flat_of(r.median)).all()
        ids = np.zeros(K, dtype=np.int64)
        ids[4] = -1
        assert same_bits(flat_of(r.median), flat_of(make_slab(x, cuda).grouped_mean(r.weights, ids, 1)[0]))
    # no iterations, uniform weights: the unit-weight mean of the usable clients. Bit for bit with
    # 8 usable clients: the weights f32(1/8) only scale by a power of two.
    r = make_slab(x, cuda).geometric_median(iterations=0)
    usable_rows = np.delete(x, 4, axis=0)
    assert same_bits(flat_of(r.median), flat_of(make_slab(usable_rows, cuda).mean([1] * 8)))
    # 5 usable clients: f32(1/5) rounds, so the two means differ by a few roundings of their terms
    x5 = usable_rows[:5]
    got = flat_of(make_slab(x5, cuda).geometric_median(iterations=0).median).astype(np.float64)
    want = flat_of(make_slab(x5, cuda).mean([1] * 5)).astype(np.float64)
    assert (np.abs(got - want) <= 2 * (5 + 2) * 2.0 ** -24 * np.abs(x5).mean(axis=0)).all()
    assert make_slab(np.full((3, 8), np.inf, dtype=F32), cuda).geometric_median().median is None


# ------------------------------------------------------------------ capture, aggregators
def test_refused_under_capture(cuda):
    x = int_round(9)
    s = make_slab(x, cuda, TEMPLATE)
    clients = make_clients(x, cuda)
    s.krum(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    seen = []
    with torch.cuda.graph(graph):
        for call in (lambda: s.krum(1), lambda: s.geometric_median(), lambda: tu.tree_krum(clients, 1),
                     lambda: tu.tree_geometric_median(clients),
                     lambda: fedjax_amd.aggregators.krum_aggregator(1).apply([(k, c, 1.0) for k, c in enumerate(clients)], None)):
            with pytest.raises(RuntimeError, match="not capturable"):
                call()
            seen.append(True)
    assert len(seen) == 5


def test_aggregators(cuda):
    K, f, m = 9, 2, 3
    x = np.array(int_round(K))
    x[5] = np.nan
    clients = make_clients(x, cuda)
    names = [f"client-{k}".encode() for k in range(K)]
    triples = [(names[k], clients[k], 1000.0 * (k + 1)) for k in range(K)]  # the weights are ignored
    want = tu.tree_krum(clients, f, m)
    agg = fedjax_amd.aggregators.krum_aggregator(f, m)
    mean, state = agg.apply(iter(triples), agg.init())
    assert same_bits(flat_of(mean), flat_of(want.mean))
    assert state.selected == tuple(names[k] for k in want.selected) and names[5] not in state.selected
    assert [state.scores[n] for n in names] == want.scores.tolist()
    want = tu.tree_geometric_median(clients, iterations=3, nu=1e-5)
    agg = fedjax_amd.aggregators.geometric_median_aggregator(3, 1e-5)
    median, state = agg.apply(iter(triples), agg.init())
    assert same_bits(flat_of(median), flat_of(want.median))
    assert [state.weights[n] for n in names] == [float(w) for w in want.weights] and state.weights[names[5]] == 0.0
