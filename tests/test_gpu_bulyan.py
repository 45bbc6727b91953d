"""Bulyan end to end on the GPU (slab.bulyan, tree_bulyan, the aggregator) against the restatement
on the vectors (tests/bulyan_ref.py: brute-force selection, then the mean around the median), and
the seeded fuzz over both new aggregates and both routes. Integer deltas make the Gram matrix
exact, so the selection and the bits are the restatement's on either route."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import pytree, slab as slab_mod, tree_util as tu
from tests import around_median_ref as am
from tests import bulyan_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


def assert_bits(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    g, w = am.canon(got).reshape(-1), am.canon(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def slab_of(x, dev, leaves=None):
    leaves = [x.shape[1]] if leaves is None else leaves
    s = slab_mod.ClientDeltaSlab({f"l{j}": torch.zeros(n) for j, n in enumerate(leaves)}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x)))
    return s


def clients_of(x, dev, leaves=None, views=False):
    """K client pytrees: every leaf its own allocation, or (views) slices of one row a client that
    starts one element into its buffer."""
    leaves = [x.shape[1]] if leaves is None else leaves
    offs = np.concatenate([[0], np.cumsum(leaves)])
    out = []
    for k in range(x.shape[0]):
        if views and k % 2:
            buf = torch.empty(x.shape[1] + 1, dtype=torch.float32, device=dev)
            buf[1:].copy_(torch.from_numpy(x[k]))
            out.append({f"l{j}": buf[1 + offs[j]:1 + offs[j + 1]] for j in range(len(leaves))})
        else:
            out.append({f"l{j}": torch.from_numpy(x[k, offs[j]:offs[j + 1]].copy()).to(dev) for j in range(len(leaves))})
    return out


def check_round(x, f, dev, what, leaves=None, views=False):
    want, S, keep = ref.bulyan(x, f)
    got_s = slab_of(x, dev, leaves).bulyan(f)
    got_t = tu.tree_bulyan(iter(clients_of(x, dev, leaves, views)), f)
    for got, route in ((got_s, "slab"), (got_t, "tree")):
        assert isinstance(got, tu.BulyanResult)
        assert got.selected.tolist() == S.tolist(), f"{what} {route}: selection"
        assert got.keep == keep and tuple(got.gram.shape) == (x.shape[0], x.shape[0])
        if want is None:
            assert got.mean is None
        else:
            assert_bits(flat_of(got.mean), want, f"{what} {route}")
    return got_s, want


@pytest.mark.parametrize("K,f,P", ref.ROUND_CASES)
def test_integer_rounds_bitwise(cuda, K, f, P):
    rng = np.random.RandomState(K + P)
    x = ref.small_ints(rng, K, P)
    got, _ = check_round(x, f, cuda, f"K={K} f={f} P={P}")
    assert len(got.selected) == K - 2 * f and got.keep == K - 4 * f


@pytest.mark.parametrize("K,f,P", ref.ROUND_CASES)
def test_byzantine_rows_do_not_reach_the_result(cuda, K, f, P):
    rng = np.random.RandomState(3 * K + P)
    x = ref.small_ints(rng, K, P)
    honest = x.copy()
    bad = ref.poison(rng, x, int(rng.randint(1, f + 1)))
    got, want = check_round(x, f, cuda, f"K={K} f={f} P={P} poisoned")
    assert not set(got.selected.tolist()) & set(bad.tolist())
    mean = flat_of(got.mean)
    assert np.isfinite(mean).all() and np.abs(mean).max() <= 8
    plain = flat_of(slab_of(x, cuda).mean([1] * K))
    with np.errstate(invalid="ignore"):
        assert ((~np.isfinite(plain)) | (np.abs(plain - honest.mean(0)) > 1e20)).all()


def test_one_hidden_coordinate_is_cut(cuda):
    """What Krum alone lets through: a client close to the others in distance with its whole error in
    one coordinate. The coordinate-wise stage drops that value."""
    K, f, P = 23, 5, 400
    rng = np.random.RandomState(4)
    x = ref.small_ints(rng, K, P)
    x[:, 17] = rng.randint(-2, 3, K)
    # the attacker sits at the centre of the honest clients (squared distance about 24 P = 9600 to each,
    # where two honest clients are about 19200 apart) and spends 3600 of that margin on one coordinate
    x[3] = 0.0
    x[3, 17] = 60.0
    got, want = check_round(x, f, cuda, "hidden coordinate")
    assert got.selected[0] == 3  # Krum's stage picks the attacker first
    assert abs(flat_of(got.mean)[17]) <= 2  # the second stage drops its coordinate


def test_too_many_unusable_clients_give_no_mean(cuda):
    K, f, P = 11, 2, 130
    x = ref.small_ints(np.random.RandomState(5), K, P)
    x[[0, 2, 3, 5, 6, 8, 10]] = np.nan
    got, want = check_round(x, f, cuda, "short selection")
    assert want is None and got.mean is None and got.keep == 0 and sorted(got.selected.tolist()) == [1, 4, 7, 9]
    agg = fedjax_amd.aggregators.bulyan_aggregator(f)
    mean, state = agg.apply([(f"c{k}", c, 1.0) for k, c in enumerate(clients_of(x, cuda))], agg.init())
    assert mean is None and sorted(state.selected) == ["c1", "c4", "c7", "c9"] and state.keep == 0


def test_normal_rounds_select_as_the_brute_force(cuda):
    cases = ref.separated_normal_cases()
    assert len(cases) >= 6
    for K, f, P, seed in cases:
        x = ref.normal_round(K, f, P, seed)
        check_round(x, f, cuda, f"N(0,1) K={K} f={f} P={P} seed={seed}")


def test_aggregator_keeps_the_selection(cuda):
    K, f, P = 23, 5, 300
    x = ref.small_ints(np.random.RandomState(6), K, P)
    want, S, keep = ref.bulyan(x, f)
    agg = fedjax_amd.aggregators.bulyan_aggregator(f)
    state = agg.init()
    for weight in (1, 17, 0.5):  # the weights change nothing
        mean, state = agg.apply(((f"c{k}", c, weight * (1 + k % 3)) for k, c in enumerate(clients_of(x, cuda))), state)
        assert_bits(flat_of(mean), want, f"weight {weight}")
        assert state.selected == tuple(f"c{k}" for k in S) and state.keep == keep


def test_both_routes_raise_under_capture(cuda):
    x = ref.small_ints(np.random.RandomState(7), 7, 64)
    s, clients = slab_of(x, cuda), clients_of(x, cuda)
    s.bulyan(1)
    torch.cuda.synchronize()
    for call in (lambda: s.bulyan(1), lambda: tu.tree_bulyan(clients, 1)):
        g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(st):
            with pytest.raises(RuntimeError, match="not capturable"):
                with torch.cuda.graph(g, stream=st):
                    call()
        torch.cuda.synchronize()
    check_round(x, 1, cuda, "eager after the refused captures")


def test_refusals_launch_nothing(cuda):
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 160, device=cuda)
    with pytest.raises(ValueError, match="128"):
        s.bulyan(15)
    with pytest.raises(ValueError, match=r"4f \+ 3"):
        s.bulyan(40)
    b = slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 7, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        b.bulyan(1)
    with pytest.raises(TypeError, match="float32"):
        tu.tree_bulyan([{"w": torch.zeros(2, device=cuda, dtype=torch.int32)}] * 7, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the seeded fuzz
def test_seeded_fuzz(cuda):
    cases = am.fuzz_cases()
    assert len(cases) == 60
    for i, (agg, K, arg, leaves, kind, seed) in enumerate(cases):
        rng = np.random.RandomState(seed)
        P = sum(leaves)
        what = f"case {i} {agg} K={K} arg={arg} leaves={leaves} {kind}"
        if agg == "bulyan":
            x = ref.small_ints(rng, K, P)
            if i % 2 and arg:
                ref.poison(rng, x, int(rng.randint(1, arg + 1)))
            check_round(x, arg, cuda, what, leaves, views=bool(i % 4 == 1))
            continue
        x = am.DATA[kind](rng, K, P)
        want = am.mean_around_median(x, arg)
        assert_bits(flat_of(slab_of(x, cuda, leaves).mean_around_median(arg)), want, f"{what} slab")
        got = tu.tree_mean_around_median(clients_of(x, cuda, leaves, views=bool(i % 2)), arg)
        assert_bits(flat_of(got), want, f"{what} tree")
