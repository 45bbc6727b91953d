"""Bulyan's host selection (fedjax_amd.robust.bulyan_select) against the brute-force restatement
on the vectors (tests/bulyan_ref.py), and the product's host surface for Bulyan: the refusals
on K and f alone, before the library is touched; the aggregator; the exports. No GPU needed."""
import numpy as np
import pytest
import torch

from fedjax_amd import robust
from tests import bulyan_ref as ref
from tests import robust_select_ref as sel

F32 = np.float32


def gram(x):
    """The exact float64 Gram of small-integer rows; a row that is not usable gets the
    non-finite diagonal the Gram pass gives it."""
    x64 = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        G = x64 @ x64.T
    bad = ~ref.usable(x)
    G[bad, :] = np.nan
    G[:, bad] = np.nan
    return G


def random_pairs(n=12, seed=5):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        f = int(rng.randint(0, 7))
        out.append((int(rng.randint(4 * f + 3, 4 * f + 3 + 30)), f))
    return out


@pytest.mark.parametrize("K,f", list(ref.SELECT_CASES) + random_pairs())
def test_selection_is_the_brute_force(K, f):
    rng = np.random.RandomState(1000 * K + f)
    x = ref.small_ints(rng, K, 37)
    G = gram(x)
    got = robust.bulyan_select(G, f)
    assert got.dtype == np.int64 and got.tolist() == ref.select(x, f).tolist()
    assert len(got) == K - 2 * f and len(set(got.tolist())) == len(got)
    assert got[0] == robust.krum_select(G, f, 1)[0] == sel.int_krum(x, f, 1)[0][0]


@pytest.mark.parametrize("K,f", [(7, 1), (23, 5), (64, 15), (40, 3)])
def test_unusable_clients_are_never_selected(K, f):
    rng = np.random.RandomState(K)
    x = ref.small_ints(rng, K, 29)
    bad = ref.poison(rng, x, f)
    assert not ref.usable(x)[bad].any() and ref.usable(x).sum() == K - f
    got = robust.bulyan_select(gram(x), f)
    assert got.tolist() == ref.select(x, f).tolist()
    assert not set(got.tolist()) & set(bad.tolist())
    assert len(got) == min(K - 2 * f, K - f)
    mean, _, keep = ref.bulyan(x, f)
    assert keep == len(got) - 2 * f and np.isfinite(mean).all()


def test_too_many_unusable_clients_give_a_short_selection_and_no_mean():
    K, f = 11, 2  # theta = 7, keep = 3: more than K - 2f - 1 = 6 unusable rows leave at most 4 = 2f to select
    rng = np.random.RandomState(3)
    x = ref.small_ints(rng, K, 19)
    x[[0, 2, 3, 5, 6, 8, 10]] = np.nan
    got = robust.bulyan_select(gram(x), f)
    assert sorted(got.tolist()) == [1, 4, 7, 9] and got.tolist() == ref.select(x, f).tolist()
    assert ref.bulyan(x, f)[0] is None
    x[:] = np.inf
    assert robust.bulyan_select(gram(x), f).tolist() == [] and ref.select(x, f).tolist() == []
    # exactly K - 2f - 1 unusable rows still leave 2f + 1 clients: a mean of one value per coordinate
    y = ref.small_ints(rng, K, 19)
    y[[0, 2, 3, 5, 6, 8]] = 1e30
    got = robust.bulyan_select(gram(y), f)
    assert sorted(got.tolist()) == [1, 4, 7, 9, 10]
    mean, S, keep = ref.bulyan(y, f)
    assert keep == 1 and S.tolist() == got.tolist() and np.isfinite(mean).all()


def test_ties_go_to_the_lower_index():
    # identical clients: every score is 0 at every step, so the selection is 0, 1, 2, ...
    G = np.ones((11, 11))
    assert robust.bulyan_select(G, 2).tolist() == list(range(7))
    # two mirrored clusters of three and one client at the origin, f = 1. Step 1, c = 4: a cluster
    # member scores 0 + 0 + 1 + 4 = 5, the origin 1 + 1 + 1 + 1 = 4: client 3. Step 2, c = 3: all six
    # score 0 + 0 + 4: client 0. Step 3, c = 2: clients 1, 2 score 0 + 4, the others 0 + 0: client 4.
    x = np.array([[1, 0], [1, 0], [1, 0], [0, 0], [-1, 0], [-1, 0], [-1, 0]], F32)
    got = robust.bulyan_select(gram(x), 1)
    assert got.tolist() == ref.select(x, 1).tolist()
    assert got[:3].tolist() == [3, 0, 4]


def test_the_clamp_keeps_one_neighbour():
    """K = 3, f = 0: n - f - 2 is 1, 0 and -1 at the three steps; the clamp makes it 1, 1 and (one client
    left) no neighbour at all: score 0."""
    x = np.array([[0, 0], [1, 0], [5, 0]], F32)
    # step 1: nearest neighbours 1, 1, 16 -> client 0 (tie with 1, lower index); step 2: R = {1, 2},
    # both score 16 -> client 1; step 3: client 2 alone, score 0.0
    assert robust.bulyan_select(gram(x), 0).tolist() == [0, 1, 2] == ref.select(x, 0).tolist()


def test_select_refusals():
    G = np.eye(7)
    for bad in (True, np.bool_(False), 1.0, "1", None):
        with pytest.raises(TypeError, match="num_byzantine"):
            robust.bulyan_select(G, bad)
    with pytest.raises(ValueError, match=">= 0"):
        robust.bulyan_select(G, -1)
    with pytest.raises(ValueError, match=r"4f \+ 3"):
        robust.bulyan_select(G, 2)
    with pytest.raises(ValueError, match=r"4f \+ 3"):
        robust.bulyan_select(np.eye(2), 0)
    with pytest.raises(ValueError, match="square"):
        robust.bulyan_select(np.zeros((3, 4)), 0)
    assert robust.bulyan_select(np.eye(7), 1).dtype == np.int64


def test_separated_normal_cases_exist():
    cases = ref.separated_normal_cases()
    assert len(cases) >= 6
    for K, f, P, seed in cases:
        x = ref.normal_round(K, f, P, seed)
        x64 = x.astype(np.float64)
        assert robust.bulyan_select(x64 @ x64.T, f).tolist() == ref.select(x, f).tolist()


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


def test_slab_and_tree_refuse_on_k_and_f_alone(no_library):
    from fedjax_amd import tree_util

    with pytest.raises(TypeError, match="float32"):
        _fake_slab(7, torch.bfloat16).bulyan(1)
    with pytest.raises(TypeError, match="float32"):
        _fake_slab(7, torch.int32).bulyan(1)
    trees = lambda K: [{"w": np.zeros(3, F32)}] * K
    for call in (lambda K, f: _fake_slab(K).bulyan(f), lambda K, f: tree_util.tree_bulyan(trees(K), f)):
        with pytest.raises(ValueError, match="1024"):
            call(1025, 224)  # K <= 1024: the Gram pass
        with pytest.raises(ValueError, match=r"4f \+ 3"):
            call(10, 2)
        with pytest.raises(ValueError, match="128"):
            call(160, 15)  # theta = 130 > 128: the column routine
        with pytest.raises(ValueError, match="128"):
            call(129, 0)
        with pytest.raises(ValueError, match=">= 0"):
            call(7, -1)
        for bad in (True, 1.0, None):
            with pytest.raises(TypeError, match="num_byzantine"):
                call(7, bad)
    assert tree_util.tree_bulyan([], 1) is None and tree_util.tree_bulyan(iter([]), 99) is None
    assert tree_util._check_bulyan_args(160, 16) == 16 and tree_util._check_bulyan_args(252, 62) == 62


def test_aggregator_state_and_exports():
    from fedjax_amd import aggregators, slab, tree_util

    for name in ("bulyan_aggregator", "BulyanAggregatorState", "mean_around_median_aggregator"):
        assert hasattr(aggregators, name), name
    agg = aggregators.bulyan_aggregator(2)
    assert isinstance(agg, aggregators.Aggregator)
    state = agg.init()
    assert isinstance(state, aggregators.BulyanAggregatorState) and state.selected == () and state.keep == 0
    got, state2 = agg.apply(iter([]), state)  # no clients: None and an empty state
    assert got is None and state2.selected == ()
    for bad in (True, 0.5, "x", None):
        with pytest.raises(TypeError):
            aggregators.bulyan_aggregator(bad)
    with pytest.raises(ValueError):
        aggregators.bulyan_aggregator(-1)
    for name in ("tree_bulyan", "tree_mean_around_median", "BulyanResult"):
        assert name in tree_util.__all__ and hasattr(tree_util, name)
    assert tree_util.BulyanResult._fields == ("mean", "selected", "keep", "gram")
    assert "bulyan_select" in robust.__all__
    assert callable(slab.ClientDeltaSlab.bulyan)
    assert "ignores the weights" in aggregators.bulyan_aggregator.__doc__.lower()
    assert "clamp" in robust.bulyan_select.__doc__
