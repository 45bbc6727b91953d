"""FLTrust on the GPU (fjagg_dotsq_rows / _dense, fjagg_fltrust_select, fjagg_fltrust_dense / _ptrs and
the Python surfaces over them) against the numpy restatement of tests/fltrust_ref.py and the host
build of the selection rule, bit for bit: the row pass's two sums, the selection's tables and
diagnostics, and every field of a whole round on both routes."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, tree_util as tu
from tests import fltrust_cases as fc
from tests import fltrust_host as host
from tests import fltrust_ref as ref

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
LENGTHS = [1, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537, 2 * 65536 + 3]
EMNIST_SIZES = tuple(fc.leaf_sizes(fc.EMNIST_128))


def l2sq_rows(rows_ptrs, ns, rows_per_group, dev):
    """fjagg_l2sq_rows itself over rows at ``rows_ptrs`` of ``ns`` elements."""
    R = len(rows_ptrs)
    image = torch.from_numpy(np.concatenate([rows_ptrs, ns]).astype(np.int64)).to(dev)
    out = torch.empty(R // rows_per_group, dtype=torch.float32, device=dev)
    need = int(_lib.load().fjagg_l2sq_rows_workspace_bytes(R, int(max(ns))))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _lib.call("fjagg_l2sq_rows", _lib.F32, image.data_ptr(), R, int(max(ns)), rows_per_group, 0, out.data_ptr(),
              ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    return out


# ------------------------------------------------------------------ 1. the row pass
@pytest.mark.parametrize("n", LENGTHS)
def test_row_pass_bitwise(cuda, n):
    K = 3
    rng = np.random.RandomState(n)
    x, g = rng.standard_normal((K, n)).astype(F32), rng.standard_normal(n).astype(F32)
    want_a, want_q = ref.product_order_sums([x], [g]), ref.product_order_sums([x], [x])
    xd = fc.on_device(x, cuda, ld=n + 5, offset=1)  # ld > P, rows and g 4 bytes off a 16-byte boundary
    gd = fc.dev_vec(g, cuda, offset=1)
    assert xd.data_ptr() % 16 == 4 and gd.data_ptr() % 16 == 4
    for nt in (False, True):
        a, q = kernels.dotsq_dense(xd, gd, nontemporal=nt)
        fc.assert_same_bits(a, want_a, f"n={n} nt={nt} dense dot")
        fc.assert_same_bits(q, want_q, f"n={n} nt={nt} dense squares")
    rows = xd.data_ptr() + 4 * xd.stride(0) * np.arange(K, dtype=np.int64)
    image = torch.from_numpy(np.concatenate([rows, np.full(K, n), np.full(K, gd.data_ptr())]).astype(np.int64)).to(cuda)
    a, q = kernels.dotsq_rows(image, K, n)
    fc.assert_same_bits(a, want_a, f"n={n} rows dot")
    fc.assert_same_bits(q, want_q, f"n={n} rows squares")
    fc.assert_same_bits(q, fc.np_of(l2sq_rows(rows, np.full(K, n), 1, cuda)), f"n={n} squares against fjagg_l2sq_rows")


def test_row_pass_over_leaves_with_an_empty_one(cuda):
    K, sizes = 4, (300, 0, 700)
    rng = np.random.RandomState(5)
    x, g = rng.standard_normal((K, 1000)).astype(F32), rng.standard_normal(1000).astype(F32)
    xs, gs = fc.split(x, sizes), fc.split(g, sizes)
    want_a, want_q = ref.product_order_sums(xs, gs), ref.product_order_sums(xs, xs)
    xd, gd = fc.on_device(x, cuda, ld=1003, offset=1), fc.dev_vec(g, cuda, offset=1)
    tab = torch.tensor([0, 300, 300, 300, 0, 700], dtype=torch.int64, device=cuda)
    a, q = kernels.dotsq_dense(xd, gd, leaf_table=tab, max_n=700)
    fc.assert_same_bits(a, want_a, "leaves, dense dot")
    fc.assert_same_bits(q, want_q, "leaves, dense squares")
    offs = np.array([0, 300, 300], dtype=np.int64)
    rows = (xd.data_ptr() + 4 * xd.stride(0) * np.arange(K, dtype=np.int64)[:, None] + 4 * offs[None]).reshape(-1)
    ns = np.tile(np.array(sizes, dtype=np.int64), K)
    image = torch.from_numpy(np.concatenate([rows, ns, np.tile(gd.data_ptr() + 4 * offs, K)])).to(cuda)
    a, q = kernels.dotsq_rows(image, K * 3, 700, rows_per_group=3)
    fc.assert_same_bits(a, want_a, "leaves, rows dot")
    fc.assert_same_bits(q, want_q, "leaves, rows squares")
    fc.assert_same_bits(q, fc.np_of(l2sq_rows(rows, ns, 3, cuda)), "leaves, squares against fjagg_l2sq_rows")
    # one leaf over the same row is another order: the leaf table is what the sums follow
    one = ref.product_order_sums([x], [g])
    a1, _ = kernels.dotsq_dense(xd, gd)
    fc.assert_same_bits(a1, one, "one leaf, dense dot")


# ------------------------------------------------------------------ 2. the selection
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return host.build(tmp_path_factory.mktemp("fltrust_select_gpu"))


def selection_cases(K):
    rng = np.random.RandomState(K)
    q = (rng.uniform(0.1, 4.0, K) ** 2).astype(F32)
    qs = F32(2.25)
    mag = np.sqrt(q.astype(F64) * F64(qs)) * rng.uniform(0.05, 1.0, K)
    one = -mag
    one[K // 2] = -one[K // 2]
    return {"nobody": (-mag.astype(F32), q, qs), "one": (one.astype(F32), q, qs), "all": (mag.astype(F32), q, qs),
            "mixed": host.seeded_rows(K, K), "server zero": (mag.astype(F32), q, F32(0))}


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1024, 4096])
def test_selection_bitwise_against_the_host_build(cuda, host_program, tmp_path, K):
    cases = selection_cases(K)
    wants = host.run(host_program, list(cases.values()), tmp_path)
    for (name, (a, q, qs)), want in zip(cases.items(), wants):
        d, tables = kernels.fltrust_select(torch.from_numpy(a).to(cuda), torch.from_numpy(q).to(cuda),
                                           torch.from_numpy(np.array([qs], F32)).to(cuda))
        got = dict(cos=d.cosines, trust=d.trust, factors=d.factors, norms=d.norms, server_norm=d.server_norm,
                   total=d.total, count=d.count, order=tables.order, seg=tables.seg, wperm=tables.wperm,
                   gscale=tables.gscale)
        for field in host.FIELDS:
            fc.assert_same_bits(got[field], want[field], f"K={K} {name} {field}")
        assert tables.M_max == K
        count = int(want["count"])
        assert count == {"nobody": 0, "one": 1, "all": K, "server zero": 0}.get(name, count)
        order = fc.np_of(tables.order)
        assert (order >= 0).all() and (order < K).all()


# ------------------------------------------------------------------ 3. whole rounds
def test_whole_round_slab_and_pytrees(cuda):
    K, P = 10, sum(EMNIST_SIZES)
    x, g = fc.mixed_round(K, P)
    want = fc.mixed_reference(K, P, EMNIST_SIZES)
    assert 0 < int(want["count"]) < K
    s = fc.slab_of(x, fc.EMNIST_128, cuda)
    gd = torch.from_numpy(np.array(g)).to(cuda)
    a = s.fltrust(gd)
    fc.check_result(a, want, "slab")
    clients = fc.separate_clients(x, fc.EMNIST_128, cuda)
    assert clients[0]["conv2_d_1"]["w"].data_ptr() % 16 == 4  # the misaligned view
    gtree = fc.tree_of(g, fc.EMNIST_128, cuda)
    before = [fc.flat_of(c) for c in clients[:2]]
    b = tu.tree_fltrust(iter(clients), gtree)  # a one-shot iterable
    fc.check_result(b, want, "tree")
    for name in ("mean",) + fc.RESULT_FIELDS:  # the two routes, bit for bit
        ga, gb = (fc.flat_of(r.mean) if name == "mean" else fc.np_of(getattr(r, name)) for r in (a, b))
        fc.assert_same_bits(ga, gb, f"slab against tree: {name}")
    # the server delta as a pytree, and an out of the caller's
    out = torch.full((P,), float("nan"), dtype=torch.float32, device=cuda)
    c = s.fltrust(gtree, out=out)
    fc.check_result(c, want, "slab, pytree server delta", mean=fc.np_of(out))
    assert pytree_leaf(c.mean).data_ptr() == out.data_ptr()
    fc.assert_same_bits(gd, g, "the server delta is not written")
    for cl, b0 in zip(clients[:2], before):
        fc.assert_same_bits(fc.flat_of(cl), b0, "the inputs are not written")
    # the dense driver on its own: the row as one leaf (another order, the same contract)
    xd = fc.on_device(x, cuda, ld=P + 3, offset=1)
    out1, d1 = kernels.fltrust_dense(xd, fc.dev_vec(g, cuda, offset=1))
    one = ref.fltrust([x], [g])
    fc.assert_same_bits(out1, one["mean"][0], "dense driver, one leaf: mean")
    fc.assert_same_bits(d1.trust, one["trust"], "dense driver, one leaf: trust")
    fc.assert_same_bits(d1.total, one["total"], "dense driver, one leaf: total")


def pytree_leaf(tree):
    from fedjax_amd import pytree
    return pytree.leaves_of(tree)[0]


def test_whole_round_4096_clients(cuda):
    K, P = 4096, 64
    x, g = fc.mixed_round(K, P)
    want = fc.mixed_reference(K, P, (P,))
    s = fc.slab_of(x, {"w": (P,)}, cuda)
    got = s.fltrust(torch.from_numpy(np.array(g)).to(cuda))
    fc.check_result(got, want, "4096 x 64 slab")
    assert 1000 < int(want["count"]) < K
    clients = [{"w": row} for row in torch.from_numpy(np.array(x)).to(cuda).unbind(0)]
    tree = tu.tree_fltrust(clients, {"w": torch.from_numpy(np.array(g)).to(cuda)})
    fc.check_result(tree, want, "4096 x 64 tree")


def test_attack_set(cuda):
    P = sum(EMNIST_SIZES)
    x, g, names = fc.attack_round(P)
    want = ref.fltrust(fc.split(x, EMNIST_SIZES), fc.split(g, EMNIST_SIZES))
    got = fc.slab_of(x, fc.EMNIST_128, cuda).fltrust(torch.from_numpy(g).to(cuda))
    fc.check_result(got, want, "attack set, slab")
    tree = tu.tree_fltrust(fc.separate_clients(x, fc.EMNIST_128, cuda), fc.tree_of(g, fc.EMNIST_128, cuda))
    fc.check_result(tree, want, "attack set, tree")
    y = fc.flat_of(got.mean)
    assert np.isfinite(y).all()
    assert np.linalg.norm(y.astype(F64)) <= np.linalg.norm(g.astype(F64)) * (1 + 1e-5)
    trust, factors = fc.np_of(got.trust), fc.np_of(got.factors)
    assert int(fc.np_of(got.count)) == 3
    for k, name in enumerate(names):
        assert (trust[k] > 0.9 and factors[k] > 0) if name in ("h0", "h1", "h2") else (trust[k] == 0 and factors[k] == 0)
    # a server delta that trusts nobody: all +0, never None
    for bad in (np.zeros(P, F32), np.full(P, np.inf, F32)):
        none = fc.slab_of(x, fc.EMNIST_128, cuda).fltrust(torch.from_numpy(bad).to(cuda))
        assert int(fc.np_of(none.count)) == 0 and not host.bits(fc.flat_of(none.mean)).any()


# ------------------------------------------------------------------ 4. excluded clients are never read
def test_gated_clients_are_never_loaded_by_the_fold(cuda):
    K, P = 12, sum(EMNIST_SIZES)
    x, g = fc.mixed_round(K, P, seed=1)
    want = fc.mixed_reference(K, P, EMNIST_SIZES, seed=1)
    gated = fc.np_of(want["factors"]) == 0
    assert 0 < gated.sum() < K
    gd = torch.from_numpy(np.array(g)).to(cuda)
    # the whole round: the gated rows hold NaN (which gates them too), or any other gated values
    for what, fill in (("NaN", np.nan), ("-3 g", None)):
        y = np.array(x)
        y[gated] = fill if fill is not None else -3 * g
        got = fc.slab_of(y, fc.EMNIST_128, cuda).fltrust(gd)
        fc.assert_same_bits(fc.flat_of(got.mean), np.concatenate(want["mean"]), f"gated rows hold {what}: mean")
        fc.assert_same_bits(got.factors, want["factors"], f"gated rows hold {what}: factors")
    # the fold alone over the tables of the clean round, with the gated rows rewritten to NaN after the selection
    xd = fc.on_device(x, cuda, ld=P + 4)
    a, q = kernels.dotsq_dense(xd, gd)
    qs = torch.from_numpy(np.array([ref.product_order_sums([g[None]], [g[None]])[0]], F32)).to(cuda)
    d, tables = kernels.fltrust_select(a, q, qs)
    clean = kernels.grouped_sum_dense_device(xd, tables, torch.zeros(P, dtype=torch.float32, device=cuda))
    clean = fc.np_of(clean).copy()
    gone = fc.np_of(d.factors) == 0
    assert 0 < gone.sum() < K and np.isfinite(clean).all()
    xd[torch.from_numpy(gone).to(cuda)] = float("nan")
    again = kernels.grouped_sum_dense_device(xd, tables, torch.zeros(P, dtype=torch.float32, device=cuda))
    fc.assert_same_bits(again, clean, "the fold with NaN in every gated row")


# ------------------------------------------------------------------ 5. no host synchronisation, capture
def test_no_host_synchronisation(cuda):
    K, P = 9, sum(EMNIST_SIZES)
    x, g = fc.mixed_round(K, P, seed=2)
    s = fc.slab_of(x, fc.EMNIST_128, cuda)
    gd = torch.from_numpy(np.array(g)).to(cuda)
    first = s.fltrust(gd)  # first call: the leaf table upload
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = s.fltrust(gd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    fc.assert_same_bits(fc.flat_of(got.mean), fc.flat_of(first.mean), "under sync debug mode")
    fc.assert_same_bits(got.trust, fc.np_of(first.trust), "trust under sync debug mode")


def test_capture_and_replay(cuda):
    K, P = 8, sum(EMNIST_SIZES)
    x, g = fc.mixed_round(K, P, seed=3)
    s = fc.slab_of(x, fc.EMNIST_128, cuda)
    gd = torch.from_numpy(np.array(g)).to(cuda)
    out = torch.empty(P, dtype=torch.float32, device=cuda)
    s.fltrust(gd, out=out)  # the eager call: the leaf table is on the device
    torch.cuda.synchronize()
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            res = s.fltrust(gd, out=out)
    counts = []
    for seed in (4, 5):  # rewritten deltas AND a rewritten server delta: each replay selects afresh
        x2, g2 = fc.mixed_round(K, P, seed=seed)
        if seed == 5:
            x2 = -np.array(x2)  # the trusted and the gated swap
        s.rows.copy_(torch.from_numpy(np.array(x2)))
        gd.copy_(torch.from_numpy(np.array(g2)))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = ref.fltrust(fc.split(np.array(x2), EMNIST_SIZES), fc.split(np.array(g2), EMNIST_SIZES))
        fc.check_result(res, want, f"replay {seed}", mean=fc.np_of(out))
        counts.append(int(want["count"]))
    assert counts[0] != counts[1] and all(0 < c < K for c in counts)
    # the tree route uploads its plan image, a slab's first call its leaf table: both refuse a capture
    clients = fc.separate_clients(np.array(x), fc.EMNIST_128, cuda)
    gtree = fc.tree_of(np.array(g), fc.EMNIST_128, cuda)
    fresh = fc.slab_of(x, fc.EMNIST_128, cuda)
    torch.cuda.synchronize()
    for call in (lambda: tu.tree_fltrust(clients, gtree), lambda: fresh.fltrust(gtree)):
        g1, st1 = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(st1):
            with pytest.raises(RuntimeError, match="not capturable"):
                with torch.cuda.graph(g1, stream=st1):
                    call()
        torch.cuda.synchronize()
        fc.check_result(call(), fc.mixed_reference(K, P, EMNIST_SIZES, seed=3), "eager after the refused capture")


# ------------------------------------------------------------------ 6. the aggregator
def test_aggregator_two_rounds(cuda):
    K, P = 6, sum(EMNIST_SIZES)
    agg = fedjax_amd.aggregators.fltrust_aggregator()
    state = agg.init()
    with pytest.raises(ValueError, match="server_delta"):
        agg.apply([("a", fc.tree_of(np.zeros(P, F32), fc.EMNIST_128, cuda), 1.0)], state)
    for rnd in (0, 1):
        x, g = fc.mixed_round(K, P, seed=10 + rnd)
        want = fc.mixed_reference(K, P, EMNIST_SIZES, seed=10 + rnd)
        ids = [f"r{rnd}c{k}" for k in range(K)]
        triples = [(cid, c, 1000.0 * (k + 1)) for k, (cid, c) in  # the weights are ignored
                   enumerate(zip(ids, fc.separate_clients(x, fc.EMNIST_128, cuda)))]
        gtree = fc.tree_of(g, fc.EMNIST_128, cuda)
        mean, state = agg.apply(triples, state.replace(server_delta=gtree))
        fc.assert_same_bits(fc.flat_of(mean), np.concatenate(want["mean"]), f"round {rnd} mean")
        assert state.server_delta is gtree and sorted(state.trust) == sorted(ids) == sorted(state.factors)
        for k, cid in enumerate(ids):  # this round's diagnostics by client id, the last round's gone
            assert state.trust[cid].dim() == 0 and state.trust[cid].is_cuda
            fc.assert_same_bits(state.trust[cid], want["trust"][k], f"round {rnd} trust of {cid}")
            fc.assert_same_bits(state.factors[cid], want["factors"][k], f"round {rnd} factors of {cid}")
