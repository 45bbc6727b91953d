"""Bulyan with the selection on the device (select="device"): bit for bit the host route on the
same deltas (both read the same Gram bits), short selections that cross a kernel width, poisoned
and hidden-coordinate clients, the select entry's tables, the second stage's clamps, run-to-run
bits, a captured slab round replayed over rewritten deltas, and a seeded fuzz."""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, aggregators, kernels, pytree, slab as slab_mod, tree_util as tu
from tests import bulyan_select_ref as ref

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
# the four widths of the second stage (theta = 3, 5 | 17 | 33 | 65, 128), their edges, odd P, P below one workgroup
ROUNDS = [(3, 0, 1), (7, 1, 255), (23, 3, 257), (43, 5, 1000), (83, 9, 1027), (160, 16, 4099), (252, 62, 257)]
RANDOM_ROUNDS = [(23, 3, 4099), (160, 16, 1000)]
LEAVES = [1, 3, 32, 1027]


def make_slab(x, dev, leaves=None):
    leaves = [x.shape[1]] if leaves is None else leaves
    s = slab_mod.ClientDeltaSlab({f"l{j}": torch.zeros(n) for j, n in enumerate(leaves)}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return s


def make_clients(x, dev, leaves=None):
    """K client pytrees. Even clients: every leaf its own allocation (aligned). Odd clients: views
    of one buffer that starts one element in, so their leaves are not 16-byte aligned."""
    leaves = [x.shape[1]] if leaves is None else leaves
    offs = np.concatenate([[0], np.cumsum(leaves)])
    out = []
    for k in range(x.shape[0]):
        if k % 2:
            buf = torch.empty(x.shape[1] + 1, dtype=torch.float32, device=dev)
            buf[1:].copy_(torch.from_numpy(np.array(x[k], dtype=F32)))
            out.append({f"l{j}": buf[1 + offs[j]:1 + offs[j + 1]] for j in range(len(leaves))})
        else:
            out.append({f"l{j}": torch.from_numpy(np.array(x[k, offs[j]:offs[j + 1]], dtype=F32)).to(dev)
                        for j in range(len(leaves))})
    return out


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def rows_of(K, P, kind):
    rng = np.random.RandomState(11 * K + P)
    x = rng.randint(-8, 9, (K, P)).astype(F32) if kind == "integer" else rng.standard_normal((K, P)).astype(F32)
    x.setflags(write=False)
    return x


def poison(x, rows):
    """NaN, inf and 1e30 rows in turn."""
    for n, r in enumerate(rows):
        x[r] = [np.nan, np.inf, 1e30][n % 3]
    return x


def check_bulyan(dev_r, host_r, f, what):
    """A DeviceBulyanResult against the host route's BulyanResult on the same deltas. Returns
    (count, keep)."""
    assert isinstance(dev_r, tu.DeviceBulyanResult) and isinstance(host_r, tu.BulyanResult)
    assert dev_r.selected.dtype == torch.int64 and dev_r.count.dtype == torch.int32
    assert dev_r.keep.dtype == torch.int32 and dev_r.step_scores.dtype == torch.float64
    count, keep = int(dev_r.count), int(dev_r.keep)
    selected = dev_r.selected.cpu().numpy()
    K = dev_r.gram.shape[0]
    assert selected.shape == (K - 2 * f,) and dev_r.step_scores.shape == (K - 2 * f,)
    assert same_bits(dev_r.gram.cpu().numpy(), host_r.gram.cpu().numpy()), what
    assert count == len(host_r.selected), what
    assert selected[:count].tolist() == host_r.selected.tolist(), what
    assert (selected[count:] == -1).all(), what
    scores = dev_r.step_scores.cpu().numpy()
    assert np.isfinite(scores[:count]).all() and np.isposinf(scores[count:]).all(), what
    assert keep == host_r.keep == (count - 2 * f if count >= 2 * f + 1 else 0), what
    mean = flat_of(dev_r.mean)
    if keep:
        assert same_bits(mean, flat_of(host_r.mean)), what
    else:
        assert host_r.mean is None and not mean.view(np.uint32).any(), what  # all +0: the sign bits too
    return count, keep


# ------------------------------------------------------------ device route against host route
@pytest.mark.parametrize("K,f,P", ROUNDS)
def test_integer_slab_rounds_are_the_host_route_bit_for_bit(cuda, K, f, P):
    x = rows_of(K, P, "integer")
    s = make_slab(x, cuda)
    assert check_bulyan(s.bulyan(f, select="device"), s.bulyan(f), f, (K, f, P)) == (K - 2 * f, K - 4 * f)
    assert same_bits(s.rows.cpu().numpy(), x)  # the inputs are never written


@pytest.mark.parametrize("K,f,P", RANDOM_ROUNDS)
def test_random_slab_rounds_are_the_host_route_bit_for_bit(cuda, K, f, P):
    s = make_slab(rows_of(K, P, "random"), cuda)
    assert check_bulyan(s.bulyan(f, select="device"), s.bulyan(f), f, (K, f, P)) == (K - 2 * f, K - 4 * f)


@pytest.mark.parametrize("K,f,kind", [(K, f, "integer") for K, f, _ in ROUNDS] +
                         [(K, f, "random") for K, f, _ in RANDOM_ROUNDS])
def test_pytree_rounds_are_the_host_route_bit_for_bit(cuda, K, f, kind):
    x = rows_of(K, sum(LEAVES), kind)
    clients = make_clients(x, cuda, LEAVES)
    assert clients[1]["l3"].data_ptr() % 16 != 0 and clients[0]["l3"].data_ptr() % 16 == 0
    got = tu.tree_bulyan(iter(clients), f, select="device")  # a one-shot iterable, consumed once
    assert check_bulyan(got, tu.tree_bulyan(clients, f), f, (K, f, kind)) == (K - 2 * f, K - 4 * f)
    assert [got.mean[f"l{j}"].shape for j in range(4)] == [(n,) for n in LEAVES]
    assert same_bits(np.stack([flat_of(c) for c in clients]), x)
    # and the slab route over the same deltas: another Gram order, the same integer Gram
    if kind == "integer":
        s = make_slab(x, cuda, LEAVES)
        assert same_bits(flat_of(s.bulyan(f, select="device").mean), flat_of(got.mean))


# --------------------------------------------------------- short selections crossing a width
@pytest.mark.parametrize("route", ["slab", "tree"])
def test_short_selection_runs_at_thetas_width_with_the_host_routes_bits(cuda, route):
    """K = 23, f = 3, 7 poisoned: 16 clients are selected, so the host route sorts at N = 16 and the
    device route, which knows only theta = 17, at N = 32. The column routine ranks by (key, client
    index) and adds in client order: the same bits."""
    K, f = 23, 3
    x = poison(np.array(rows_of(K, sum(LEAVES), "integer")), [0, 3, 4, 9, 15, 21, 22])
    if route == "slab":
        s = make_slab(x, cuda)
        dev_r, host_r = s.bulyan(f, select="device"), s.bulyan(f)
    else:
        clients = make_clients(x, cuda, LEAVES)
        dev_r, host_r = tu.tree_bulyan(clients, f, select="device"), tu.tree_bulyan(clients, f)
    assert check_bulyan(dev_r, host_r, f, route) == (16, 10)
    assert not set(dev_r.selected.tolist()) & {0, 3, 4, 9, 15, 21, 22}
    assert np.isfinite(flat_of(dev_r.mean)).all()


@pytest.mark.parametrize("route", ["slab", "tree"])
def test_too_short_a_selection_gives_a_zero_mean(cuda, route):
    """K = 7, f = 1 with 5 poisoned: count = 2 < 2f + 1, keep = 0; then all poisoned: count = 0."""
    K, f = 7, 1
    for bad, want in (([0, 1, 3, 4, 6], 2), (list(range(K)), 0)):
        x = poison(np.array(rows_of(K, sum(LEAVES), "integer")), bad)
        if route == "slab":
            s = make_slab(x, cuda)
            dev_r, host_r = s.bulyan(f, select="device"), s.bulyan(f)
        else:
            clients = make_clients(x, cuda, LEAVES)
            dev_r, host_r = tu.tree_bulyan(clients, f, select="device"), tu.tree_bulyan(clients, f)
        assert host_r.mean is None
        assert check_bulyan(dev_r, host_r, f, (route, want)) == (want, 0)
        mean = flat_of(dev_r.mean)
        assert mean.shape == (sum(LEAVES),) and not mean.view(np.uint32).any()  # +0: no sign bit either
        assert sorted(dev_r.selected[:want].tolist()) == sorted(set(range(K)) - set(bad))


# ------------------------------------------------------------------------- Byzantine clients
@pytest.mark.parametrize("K,f,P", [(7, 1, 257), (23, 5, 1000), (64, 15, 515), (160, 16, 2049)])
def test_byzantine_rows_do_not_reach_the_result(cuda, K, f, P):
    rng = np.random.RandomState(3 * K + P)
    x = rng.randint(-8, 9, (K, P)).astype(F32)
    honest = x.copy()
    bad = np.sort(rng.choice(K, size=int(rng.randint(1, f + 1)), replace=False))
    poison(x, bad)
    s = make_slab(x, cuda)
    got = s.bulyan(f, select="device")
    check_bulyan(got, s.bulyan(f), f, (K, f, P))
    assert not set(got.selected.tolist()) & set(bad.tolist())
    mean = flat_of(got.mean)
    assert np.isfinite(mean).all() and np.abs(mean).max() <= 8
    plain = flat_of(s.mean([1] * K))
    with np.errstate(invalid="ignore"):
        assert ((~np.isfinite(plain)) | (np.abs(plain - honest.mean(0)) > 1e20)).all()


def test_one_hidden_coordinate_is_cut(cuda):
    """A client close to the others in distance with its whole error in one coordinate: the first
    stage picks it first, the coordinate-wise stage drops that value."""
    K, f, P = 23, 5, 400
    rng = np.random.RandomState(4)
    x = rng.randint(-8, 9, (K, P)).astype(F32)
    x[:, 17] = rng.randint(-2, 3, K)
    x[3] = 0.0
    x[3, 17] = 60.0
    s = make_slab(x, cuda)
    got = s.bulyan(f, select="device")
    check_bulyan(got, s.bulyan(f), f, "hidden coordinate")
    assert int(got.selected[0]) == 3
    assert abs(flat_of(got.mean)[17]) <= 2


# -------------------------------------------------------------------- the select entry alone
def test_select_kernel_writes_the_tables_of_the_rule(cuda):
    for K, f, bad in ((7, 1, []), (23, 3, [2, 5, 11, 12, 13, 20, 22]), (23, 3, list(range(20))), (43, 5, [1, 40]),
                      (9, 1, list(range(9))), (252, 62, [0, 100, 251])):
        x = np.array(rows_of(K, 40, "integer"))
        x[K - 1] = x[0]  # a duplicated client: ties
        poison(x, bad)
        G = make_slab(x, cuda).gram()
        selected, count, step_scores, tables = kernels.bulyan_select_device(G, f)
        w_selected, w_count, w_scores, w_keep, w_scale, w_rows = ref.select(G.cpu().numpy(), f)
        what = (K, f, len(bad))
        assert int(count) == w_count and int(tables.keep) == w_keep and tables.M_max == K - 2 * f, what
        assert same_bits(selected.cpu().numpy(), w_selected), what  # the -1 padding too
        assert same_bits(step_scores.cpu().numpy(), w_scores), what  # the +inf padding too
        assert same_bits(tables.scale.cpu().numpy().reshape(1), w_scale), what
        assert same_bits(tables.rows.cpu().numpy(), w_rows), what  # the repeated last row too


# ------------------------------------------------------------------- the second stage's clamps
def test_second_stage_clamps_a_garbage_table(cuda):
    """count > M_max, keep > count, a row index >= K_rows and negative ones: the kernel clamps the
    count to M_max = 5, keep to 5 and the rows to 0, 7, 2, 7, 7 (fjrobust.hip: meamed_tables and the
    load of k_meamed_dense_dev clamp before any address is formed), so the result is the plain sum
    of those rows in table order times the scale."""
    K_rows, P = 8, 1000
    x = np.array(rows_of(K_rows, P, "integer"))
    xd = torch.from_numpy(x).to(cuda)
    ints = torch.tensor([-3, 100, 2, 2 ** 30, 7, 9, 50], dtype=torch.int32, device=cuda)
    scale = torch.tensor(0.25, dtype=torch.float32, device=cuda)
    tables = kernels.DeviceRowTables(ints[:5], ints[5], ints[6], scale, 5)
    got = kernels.meamed_dense_device(xd, tables).cpu().numpy()
    want = ((((x[0] + x[7]) + x[2]) + x[7]) + x[7]) * F32(0.25)
    assert np.isfinite(got).all() and same_bits(got, want)
    # a negative count is no client at all: +0 everywhere
    ints2 = torch.tensor([0, 1, 2, 3, 4, -7, 3], dtype=torch.int32, device=cuda)
    got = kernels.meamed_dense_device(xd, kernels.DeviceRowTables(ints2[:5], ints2[5], ints2[6], scale, 5))
    assert not got.cpu().numpy().view(np.uint32).any()
    # a consistent table is the host entry's bits at another width (M = 3 of M_max = 5 / 20)
    for M_max in (5, 20):
        rows = [1, 4, 6] + [6] * (M_max - 3)
        ints3 = torch.tensor(rows + [3, 2], dtype=torch.int32, device=cuda)
        half = torch.tensor(0.5, dtype=torch.float32, device=cuda)
        big = torch.from_numpy(np.array(rows_of(24, P, "random"))).to(cuda)
        got = kernels.meamed_dense_device(big, kernels.DeviceRowTables(ints3[:M_max], ints3[M_max], ints3[M_max + 1],
                                                                       half, M_max))
        assert same_bits(got.cpu().numpy(), kernels.meamed_dense(big, 2, [1, 4, 6], scale=0.5).cpu().numpy())


# ----------------------------------------------------------------------------------- other
def test_two_eager_runs_give_identical_bits(cuda):
    x = poison(np.array(rows_of(83, sum(LEAVES), "random")), [7, 50])
    s = make_slab(x, cuda)
    clients = make_clients(x, cuda, LEAVES)

    def everything():
        out = []
        for r in (s.bulyan(9, select="device"), tu.tree_bulyan(clients, 9, select="device")):
            out += [flat_of(r.mean), r.selected.cpu().numpy(), r.count.cpu().numpy(), r.keep.cpu().numpy(),
                    r.step_scores.cpu().numpy(), r.gram.cpu().numpy()]
        return out

    first, second = everything(), everything()
    assert all(same_bits(a, b) for a, b in zip(first, second))


def test_captured_slab_round_selects_afresh_on_replay(cuda):
    """slab.bulyan(f, select="device") recorded once (a linear graph); the slab rewritten so that
    other clients are chosen, or too few can be; every replay gives the bits of an eager host-route
    call on the new data, the all-zero mean included."""
    K, P, f = 11, 1028, 2
    rng = np.random.RandomState(11)
    first = rng.randint(-8, 9, (K, P)).astype(F32)
    second = rng.randint(-8, 9, (K, P)).astype(F32)
    second[[0, 1, 2]] *= 40.0  # far from everyone: left for last, or out
    short = poison(second.copy(), [0, 2, 3, 5, 6, 8, 10])  # 4 usable: count = 4, keep = 0
    s = make_slab(first, cuda)
    before = s.bulyan(f)
    s.bulyan(f, select="device")  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s.bulyan(f, select="device")  # this stream's workspaces
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            r = s.bulyan(f, select="device")
    seen = []
    for data in (second, short, first, second):
        s.rows.copy_(torch.from_numpy(data))
        g.replay()
        torch.cuda.synchronize()
        want = s.bulyan(f)
        seen.append(check_bulyan(r, want, f, "replay"))
    assert seen == [(7, 3), (4, 0), (7, 3), (7, 3)]
    assert before.selected.tolist() != want.selected.tolist()  # another selection


def test_tree_route_still_refuses_capture(cuda):
    clients = make_clients(rows_of(7, 37, "integer"), cuda)
    tu.tree_bulyan(clients, 1, select="device")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with pytest.raises(RuntimeError, match="pinned staging"):
            with torch.cuda.graph(g, stream=st):
                tu.tree_bulyan(clients, 1, select="device")
    torch.cuda.synchronize()


def test_aggregator_on_the_device_route(cuda):
    K, f = 23, 5
    x = rows_of(K, 300, "integer")
    clients = make_clients(x, cuda)
    triples = [(f"c{k}", c, 1 + k) for k, c in enumerate(clients)]
    agg = aggregators.bulyan_aggregator(f, select="device")
    mean, state = agg.apply(iter(triples), agg.init())
    want, want_state = aggregators.bulyan_aggregator(f).apply(triples, None)
    assert isinstance(state, aggregators.DeviceBulyanAggregatorState)
    assert same_bits(flat_of(mean), flat_of(want))
    assert state.client_ids == tuple(c for c, _, _ in triples)
    assert int(state.count) == K - 2 * f and int(state.keep) == want_state.keep == K - 4 * f
    assert tuple(state.client_ids[k] for k in state.selected.tolist()) == want_state.selected
    # too few selectable clients: +0 instead of None, the state says why
    bad = [(cid, {"l0": torch.full_like(c["l0"], float("nan"))} if k < 20 else c, w)
           for k, (cid, c, w) in enumerate(triples)]
    mean, state = agg.apply(bad, state)
    assert int(state.count) == 3 and int(state.keep) == 0 and not flat_of(mean).view(np.uint32).any()
    assert aggregators.bulyan_aggregator(f).apply(bad, None)[0] is None


def test_templates_without_elements(cuda):
    """Every inner product is the empty sum: all scores 0, the lowest index wins every step."""
    K, f = 7, 1
    s = slab_mod.ClientDeltaSlab({"z": torch.zeros(0)}, K, device=cuda)
    clients = [{"z": torch.zeros(0, device=cuda)} for _ in range(K)]
    for r, host_r in ((s.bulyan(f, select="device"), s.bulyan(f)),
                      (tu.tree_bulyan(clients, f, select="device"), tu.tree_bulyan(clients, f))):
        assert int(r.count) == 5 and int(r.keep) == 3
        assert r.selected.tolist() == host_r.selected.tolist() == [0, 1, 2, 3, 4]
        assert r.step_scores.tolist() == [0.0] * 5 and r.mean["z"].numel() == 0


def test_the_new_entries_are_exported(cuda):
    lib = _lib.load()
    for sym in ("fjagg_bulyan_select", "fjagg_bulyan_select_workspace_bytes", "fjagg_meamed_dense_dev",
                "fjagg_meamed_ptrs_dev"):
        assert getattr(lib, sym) is not None
    assert "DeviceBulyanResult" in tu.__all__ and hasattr(aggregators, "DeviceBulyanAggregatorState")
    assert hasattr(kernels, "DeviceRowTables") and hasattr(kernels, "bulyan_select_device")


def test_seeded_fuzz(cuda):
    """40 rounds: K in [3, 64], every valid f (the first 16 rounds walk f = 0 .. 15), P in [1, 3000],
    random poisoned sets and duplicated clients, slab and pytrees, against the host route. No round
    is skipped: both routes read the same Gram bits, so nothing is ambiguous."""
    rng = np.random.RandomState(20240)
    rounds = [(int(rng.randint(4 * f + 3, 65)), f) for f in range(16)]
    while len(rounds) < 40:
        K = int(rng.randint(3, 65))
        rounds.append((K, int(rng.randint(0, (K - 3) // 4 + 1))))
    assert {f for _, f in rounds} >= set(range(16))
    counts = set()
    for n, (K, f) in enumerate(rounds):
        P = int(rng.randint(1, 3001))
        x = rng.randint(-8, 9, (K, P)).astype(F32) if n % 2 else rng.standard_normal((K, P)).astype(F32)
        for _ in range(int(rng.randint(0, 4))):  # duplicated clients
            a, b = rng.randint(0, K, 2)
            x[a] = x[b]
        n_bad = int(rng.choice([0, rng.randint(0, f + 1), rng.randint(0, K + 1)]))
        poison(x, rng.choice(K, size=n_bad, replace=False))
        what = (n, K, f, P, n_bad)
        s = make_slab(x, cuda)
        counts.add(check_bulyan(s.bulyan(f, select="device"), s.bulyan(f), f, what + ("slab",))[0] == K - 2 * f)
        cut = sorted(set(rng.randint(0, P + 1, 3).tolist()) | {0, P})
        leaves = [b - a for a, b in zip(cut[:-1], cut[1:])]  # up to four leaves, empty ones dropped
        clients = make_clients(x, cuda, leaves)
        check_bulyan(tu.tree_bulyan(clients, f, select="device"), tu.tree_bulyan(clients, f), f, what + ("tree",))
    assert counts == {True, False}  # full and short selections were both seen
