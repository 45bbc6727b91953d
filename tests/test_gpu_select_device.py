"""Krum and the geometric median with the selection on the device (select="device"): bit for bit
the host route's Krum, the numpy restatement's Weiszfeld weights on the device's own Gram matrix,
the grouped fold the results are defined by, poisoned and unusable clients, run-to-run bits, and a
captured slab round replayed over rewritten deltas."""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, pytree, robust, slab as slab_mod, tree_util as tu
from tests import select_device_ref as ref

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
KS = [3, 5, 33, 129, 257]
PS = [3, 1028]  # 3: element units; 1028: 16-byte units and a tail


def make_slab(x, dev):
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(x.shape[1])}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return s


def make_clients(x, dev):
    """K client pytrees of two leaves; leaf "b" starts 4 bytes into its allocation, so it is not
    16-byte aligned and walks element units."""
    n_a = x.shape[1] // 2
    out = []
    for row in x:
        a = torch.from_numpy(np.array(row[:n_a], dtype=F32)).to(dev)
        buf = torch.empty(x.shape[1] - n_a + 1, dtype=torch.float32, device=dev)
        b = buf[1:]
        b.copy_(torch.from_numpy(np.array(row[n_a:], dtype=F32)))
        assert b.data_ptr() % 16 == 4
        out.append({"a": a, "b": b})
    return out


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def rows_of(K, P):
    x = np.random.RandomState(7 * K + P).standard_normal((K, P)).astype(F32)
    x.setflags(write=False)
    return x


def krum_params(K):
    return [(f, m) for f in sorted({0, (K - 3) // 2}) for m in sorted({1, K - f})]


def check_krum(dev_r, host_r, what):
    """A DeviceKrumResult against the host route's KrumResult on the same deltas."""
    count = int(dev_r.count)
    selected = dev_r.selected.cpu().numpy()
    assert dev_r.selected.dtype == torch.int64 and dev_r.count.dtype == torch.int32 and dev_r.scores.dtype == torch.float64
    assert count == len(host_r.selected), what
    assert selected[:count].tolist() == host_r.selected.tolist(), what
    assert (selected[count:] == -1).all(), what
    assert same_bits(dev_r.scores.cpu().numpy(), host_r.scores), what
    assert same_bits(dev_r.gram.cpu().numpy(), host_r.gram.cpu().numpy()), what
    mean = flat_of(dev_r.mean)
    if count:
        assert same_bits(mean, flat_of(host_r.mean)), what
    else:
        assert host_r.mean is None and not mean.view(np.uint32).any(), what  # all +0 bits
    return count


# ------------------------------------------------------------------------------------ Krum
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_krum_slab_is_the_host_route_bit_for_bit(cuda, K, P):
    s = make_slab(rows_of(K, P), cuda)
    for f, m in krum_params(K):
        assert check_krum(s.krum(f, m, select="device"), s.krum(f, m), (K, P, f, m)) == m
    assert same_bits(s.rows.cpu().numpy(), rows_of(K, P))  # the inputs are never written


@pytest.mark.parametrize("K", KS)
def test_krum_pytrees_is_the_host_route_bit_for_bit(cuda, K):
    x = rows_of(K, 37)
    clients = make_clients(x, cuda)
    for f, m in krum_params(K):
        got = tu.tree_krum(iter(clients), f, m, select="device")  # a one-shot iterable, consumed once
        assert check_krum(got, tu.tree_krum(clients, f, m), (K, f, m)) == m
        assert got.mean["a"].shape == (18,) and got.mean["b"].shape == (19,)
    assert same_bits(np.stack([flat_of(c) for c in clients]), x)


def test_krum_1024_clients(cuda):
    K, P = 1024, 64
    s = make_slab(rows_of(K, P), cuda)
    for f, m in ((0, 1), (510, 514)):
        assert check_krum(s.krum(f, m, select="device"), s.krum(f, m), (f, m)) == m


def test_krum_duplicated_clients_tie_to_the_lower_index(cuda):
    x = np.random.RandomState(5).randint(-7, 8, size=(9, 40)).astype(F32)  # integers: exact inner products
    x[8] = x[0]
    x[5] = x[2]
    s = make_slab(x, cuda)
    for f, m in ((0, 1), (0, 9), (3, 6), (2, 3)):
        r = s.krum(f, m, select="device")
        check_krum(r, s.krum(f, m), (f, m))
        scores = r.scores.cpu().numpy()
        assert scores[8] == scores[0] and scores[5] == scores[2]


@pytest.mark.parametrize("route", ["slab", "tree"])
def test_krum_never_selects_a_poisoned_client(cuda, route):
    K, f = 11, 3
    x = np.array(rows_of(K, 37))
    x[2] = np.nan
    x[6] = np.inf
    x[9] = 1e30
    s = make_slab(x, cuda)
    clients = make_clients(x, cuda)
    for m in (1, K - f):
        if route == "slab":
            dev_r, host_r = s.krum(f, m, select="device"), s.krum(f, m)
        else:
            dev_r, host_r = tu.tree_krum(clients, f, m, select="device"), tu.tree_krum(clients, f, m)
        assert check_krum(dev_r, host_r, (route, m)) == m
        assert not set(dev_r.selected.tolist()) & {2, 6, 9}
        assert np.isfinite(flat_of(dev_r.mean)).all()


@pytest.mark.parametrize("route", ["slab", "tree"])
def test_krum_with_fewer_selectable_clients_than_m(cuda, route):
    """K - f - 1 usable clients: each still has K - f - 2 finite neighbours, but m = K - f asks for
    one more than there are; then no usable client at all."""
    K, f = 9, 2
    x = np.array(rows_of(K, 37))
    x[[1, 4, 7]] = np.nan
    for data, want in ((x, K - f - 1), (np.full_like(x, np.nan), 0)):
        if route == "slab":
            s = make_slab(data, cuda)
            dev_r, host_r = s.krum(f, K - f, select="device"), s.krum(f, K - f)
        else:
            clients = make_clients(data, cuda)
            dev_r, host_r = tu.tree_krum(clients, f, K - f, select="device"), tu.tree_krum(clients, f, K - f)
        assert check_krum(dev_r, host_r, (route, want)) == want
        if want == 0:
            assert np.isinf(dev_r.scores.cpu().numpy()).all()
            assert not flat_of(dev_r.mean).view(np.uint32).any()


def test_krum_select_kernel_writes_the_tables_of_the_rules(cuda):
    x = np.array(rows_of(33, 37))
    x[4] = np.nan
    G = make_slab(x, cuda).gram()
    for f, m in ((0, 1), (0, 33), (15, 18), (3, 7)):
        scores, selected, count, tables = kernels.krum_select_device(G, f, m)
        want = ref.krum_tables(G.cpu().numpy(), f, m)
        got = (scores, selected, count, tables.order, tables.seg, tables.wperm, tables.gscale)
        assert int(count) == want[2]
        for g, w in zip(got, want):
            if not isinstance(w, int):
                assert same_bits(g.cpu().numpy(), w), (f, m)


# ------------------------------------------------------------------------- geometric median
def median_tolerance(x, a32, K):
    """|device median - host-route median| per element. The two routes fold float32 weights that
    differ by at most 1 ulp each (2^-23 relative), each fold's K sequential float32 additions and
    products err by at most (K + 1) 2^-24 of sum_k |x_k| a_k, and the scales differ by the host's
    float32 sum of the weights (K 2^-24), the weights' own ulp (2^-23) and three roundings:
    (3K + 10) 2^-24 of sum_k |x_k| a_k / W covers them."""
    a = a32.astype(F64)
    usable = a > 0
    mag = (np.abs(x[usable].astype(F64)) * a[usable, None]).sum(0) / a[usable].sum()
    return (3 * K + 10) * 2.0 ** -24 * mag


def check_median(r, x, host_r, alpha, T, what, regroup):
    """A DeviceGeometricMedianResult: the restatement's bits on the device's own Gram, the grouped
    fold's bits with those weights, and the host route within the bound of the CPU tests."""
    K = x.shape[0]
    G = r.gram.cpu().numpy()
    a, d, a32, count = ref.weiszfeld(G, alpha, 1e-6, T)[:4]
    assert r.weights.dtype == torch.float32 and r.distances.dtype == torch.float64 and r.count.dtype == torch.int32
    assert same_bits(r.weights.cpu().numpy(), a32), what
    assert same_bits(r.distances.cpu().numpy(), d), what
    assert int(r.count) == count, what
    ids = np.where(a32 > 0, 0, -1)
    median = flat_of(r.median)
    if count:
        # Python floats: grouped_mean then adds the total in float64, in member order, as the kernel does
        assert same_bits(median, flat_of(regroup([float(w) for w in a32], ids))), what
    else:
        assert not median.view(np.uint32).any(), what
    if host_r is not None:
        assert same_bits(G, host_r.gram.cpu().numpy())
        assert ref.ulp_distance32(a32, host_r.weights).max() <= 1, what
        fin = np.isfinite(d)
        assert np.allclose(d[fin], host_r.distances[fin], rtol=1e-9, atol=1e-12), what
        tol = median_tolerance(x, a32, K)
        assert (np.abs(median.astype(F64) - flat_of(host_r.median).astype(F64)) <= tol).all(), what


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_geometric_median_slab(cuda, K, P):
    x = rows_of(K, P)
    s = make_slab(x, cuda)
    regroup = lambda w, ids: s.grouped_mean(w, ids, 1)[0]
    for T in (0, 4):
        check_median(s.geometric_median(iterations=T, select="device"), x, s.geometric_median(iterations=T), None, T,
                     (K, P, T), regroup)
    alpha = np.random.RandomState(K).randint(1, 500, K).tolist()
    check_median(s.geometric_median(alpha, select="device"), x, s.geometric_median(alpha), np.array(alpha, F64), 4,
                 (K, P, "alpha"), regroup)


@pytest.mark.parametrize("K", KS)
def test_geometric_median_pytrees(cuda, K):
    x = rows_of(K, 37)
    clients = make_clients(x, cuda)
    regroup = lambda w, ids: tu.tree_grouped_mean(list(zip(clients, w)), ids, 1)[0]
    got = tu.tree_geometric_median(iter(clients), select="device")
    check_median(got, x, tu.tree_geometric_median(clients), None, 4, K, regroup)
    assert got.median["a"].shape == (18,) and got.median["b"].shape == (19,)


def test_geometric_median_weights_against_robust_py(cuda):
    """The kernel's float64 weights against robust.weiszfeld_weights on the same Gram, which adds
    in another order: relative 1e-12, as the CPU test of the two references (measured there:
    1.6e-15)."""
    for K in (33, 257, 1024):
        x = np.array(rows_of(K, 64))
        x[0] *= 50.0  # the outlier
        G = make_slab(x, cuda).gram()
        a, d, a32, count, tables = kernels.weiszfeld_select_device(G)
        a_ref, d_ref = robust.weiszfeld_weights(G.cpu().numpy())
        a = a.cpu().numpy()
        rel = np.abs(a - a_ref) / a_ref
        print(f"K={K}: worst relative difference of a {rel.max():.3g}")
        assert rel.max() <= 1e-12
        assert ref.ulp_distance32(a32.cpu().numpy(), a_ref.astype(F32)).max() <= 1
        want = ref.weiszfeld(G.cpu().numpy())
        got = (a, d, a32, count, tables.order, tables.seg, tables.wperm, tables.gscale)
        assert int(count) == want[3] == K
        for g, w in zip(got, want):
            if not isinstance(w, int):
                assert same_bits(g if isinstance(g, np.ndarray) else g.cpu().numpy(), w), K


@pytest.mark.parametrize("route", ["slab", "tree"])
def test_geometric_median_unusable_clients(cuda, route):
    K = 9
    x = np.array(rows_of(K, 37))
    x[3] = np.nan
    x[5] = np.inf
    for data, usable in ((x, K - 2), (np.full_like(x, np.nan), 0)):
        if route == "slab":
            s = make_slab(data, cuda)
            r, host_r = s.geometric_median(select="device"), s.geometric_median()
            regroup = lambda w, ids: s.grouped_mean(w, ids, 1)[0]
        else:
            clients = make_clients(data, cuda)
            r, host_r = tu.tree_geometric_median(clients, select="device"), tu.tree_geometric_median(clients)
            regroup = lambda w, ids: tu.tree_grouped_mean(list(zip(clients, w)), ids, 1)[0]
        check_median(r, np.nan_to_num(data, nan=0.0, posinf=0.0), host_r if usable else None, None, 4, (route, usable),
                     regroup)
        assert int(r.count) == usable
        w = r.weights.cpu().numpy()
        if usable:
            assert w[3] == 0 and w[5] == 0 and np.isfinite(flat_of(r.median)).all()
        else:
            assert host_r.median is None and not w.any() and np.isinf(r.distances.cpu().numpy()).all()


# ----------------------------------------------------------------------------------- other
def test_two_eager_runs_give_identical_bits(cuda):
    x = np.array(rows_of(129, 1028))
    x[7] = np.nan
    s = make_slab(x, cuda)
    clients = make_clients(x[:, :37], cuda)

    def everything():
        out = []
        for r in (s.krum(20, 5, select="device"), tu.tree_krum(clients, 20, 5, select="device")):
            out += [flat_of(r.mean), r.selected.cpu().numpy(), r.count.cpu().numpy(), r.scores.cpu().numpy(),
                    r.gram.cpu().numpy()]
        for r in (s.geometric_median(select="device"), tu.tree_geometric_median(clients, select="device")):
            out += [flat_of(r.median), r.weights.cpu().numpy(), r.distances.cpu().numpy(), r.count.cpu().numpy()]
        return out

    first, second = everything(), everything()
    assert all(same_bits(a, b) for a, b in zip(first, second))


def test_templates_without_elements(cuda):
    """Every inner product is the empty sum: all scores 0, the lowest indices win, nothing to fold."""
    K = 5
    s = slab_mod.ClientDeltaSlab({"z": torch.zeros(0)}, K, device=cuda)
    clients = [{"z": torch.zeros(0, device=cuda)} for _ in range(K)]
    for r, host_r in ((s.krum(1, 2, select="device"), s.krum(1, 2)),
                      (tu.tree_krum(clients, 1, 2, select="device"), tu.tree_krum(clients, 1, 2))):
        assert int(r.count) == 2 and r.selected.tolist() == host_r.selected.tolist() == [0, 1]
        assert r.scores.tolist() == [0.0] * K and r.mean["z"].numel() == 0
    for r in (s.geometric_median(select="device"), tu.tree_geometric_median(clients, select="device")):
        assert int(r.count) == K and r.median["z"].numel() == 0
        assert same_bits(r.weights.cpu().numpy(), np.full(K, 0.2, F32))


def test_aggregators_on_the_device_route(cuda):
    from fedjax_amd import aggregators

    x = rows_of(9, 37)
    clients = make_clients(x, cuda)
    triples = [(f"c{k}", c, 1 + k) for k, c in enumerate(clients)]
    mean, state = aggregators.krum_aggregator(2, 3, select="device").apply(triples, None)
    want, want_state = aggregators.krum_aggregator(2, 3).apply(triples, None)
    assert same_bits(flat_of(mean), flat_of(want))
    assert tuple(state.client_ids[k] for k in state.selected.tolist()) == want_state.selected
    assert int(state.count) == 3 and state.scores.tolist() == [want_state.scores[c] for c in state.client_ids]
    median, state = aggregators.geometric_median_aggregator(select="device").apply(triples, None)
    want, want_state = aggregators.geometric_median_aggregator().apply(triples, None)
    assert int(state.count) == 9 and state.client_ids == tuple(c for c, _, _ in triples)
    got_w = state.weights.cpu().numpy()
    assert ref.ulp_distance32(got_w, np.array([want_state.weights[c] for c in state.client_ids], F32)).max() <= 1
    tol = median_tolerance(x, got_w, 9)
    assert (np.abs(flat_of(median).astype(F64) - flat_of(want).astype(F64)) <= tol).all()


def test_tree_route_still_refuses_capture(cuda):
    clients = make_clients(rows_of(5, 37), cuda)
    tu.tree_krum(clients, 1, 2, select="device")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with pytest.raises(RuntimeError, match="pinned staging"):
            with torch.cuda.graph(g, stream=st):
                tu.tree_krum(clients, 1, 2, select="device")
    torch.cuda.synchronize()


def test_captured_slab_round_selects_afresh_on_replay(cuda):
    """slab.krum(f, 2, select="device") recorded once; the slab rewritten so that other clients
    win; the replay gives the bits of an eager host-route call on the new data."""
    K, P, f = 9, 1028, 2
    rng = np.random.RandomState(11)
    base = rng.standard_normal(P).astype(F32)

    def cluster(members):
        x = (10 * rng.standard_normal((K, P))).astype(F32)  # far from everyone
        for k in members:
            x[k] = base + 0.01 * rng.standard_normal(P).astype(F32)
        return x

    first, second = cluster([0, 1, 2, 3, 4, 5]), cluster([3, 4, 5, 6, 7, 8])
    for x in (first, second):  # 3, 4 and 5 sit in both clusters, but looser: the winners move from 0-2 to 6-8
        x[[3, 4, 5]] += 0.05 * rng.standard_normal((3, P)).astype(F32)
    s = make_slab(first, cuda)
    before = s.krum(f, 2)
    s.krum(f, 2, select="device")  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s.krum(f, 2, select="device")  # this stream's Gram workspace
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            r = s.krum(f, 2, select="device")
    for data in (second, first, second):
        s.rows.copy_(torch.from_numpy(data))
        g.replay()
        torch.cuda.synchronize()
        want = s.krum(f, 2)
        assert check_krum(r, want, "replay") == 2
    assert set(before.selected.tolist()) != set(want.selected.tolist())  # different clients won


def test_the_new_entries_are_exported(cuda):
    lib = _lib.load()
    for sym in ("fjagg_krum_select", "fjagg_weiszfeld_select", "fjagg_wsum_group_dense_dev",
                "fjagg_wsum_group_ptrs_dev", "fjagg_gather_member_ptrs"):
        assert getattr(lib, sym) is not None
