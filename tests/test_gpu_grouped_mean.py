"""Grouped weighted mean on the GPU (fjagg_wsum_group_dense / _ptrs and the Python surface over
them: kernels.grouped_sum_dense, ClientDeltaSlab.grouped_mean, tree_util.tree_grouped_mean)
against the numpy float32 restatement in tests/grouped_mean_ref.py, bit for bit.

Bit patterns are compared with every NaN mapped to one pattern: IEEE 754 leaves the sign and
payload of a generated NaN to the implementation, and neither XLA nor the reference pins them.
"""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import kernels, pytree, slab as slab_mod, tree_util as tu
from tests import algorithms_restated as ar
from tests import grouped_mean_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = F32(-1234.5)


def assert_bits(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    g, w = ref.bits(got).reshape(-1), ref.bits(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} against {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


@functools.lru_cache(maxsize=None)
def deltas(K, P, seed=0):
    """Seeded CPU normal deltas, client k scaled by 2**((k % 5) - 2): float32 [K, P]."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * K + P)
    x = torch.randn(K, P, generator=g, dtype=torch.float32)
    x *= torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], dtype=torch.float32)[:, None]
    x = x.numpy()
    x.setflags(write=False)
    return x


def weights_for(K, fractional, seed=0):
    rng = np.random.RandomState(17 * K + seed)
    if fractional:
        return [float(v) for v in rng.uniform(0.1, 3.0, K)]
    return [int(v) for v in rng.randint(1, 500, K)]


def on_device(x, dev, ld):
    """x [K, P] as a device view with row stride ld > P (the padding holds NaN: never read)."""
    K, P = x.shape
    store = torch.full((K, ld), float("nan"), dtype=torch.float32, device=dev)
    store[:, :P].copy_(torch.from_numpy(np.array(x)))
    return store[:, :P]


def check_grouped(got, want, sentinel_rows=None, what=""):
    """``want``: the restatement's list (None = no result). ``got`` [G, P] device tensor."""
    got = got.detach().cpu().numpy()
    for g, wg in enumerate(want):
        if wg is None:
            if sentinel_rows is not None:
                assert (got[g] == SENTINEL).all(), f"{what}: group {g} has no result but its row was written"
        else:
            assert_bits(got[g], wg, f"{what} group {g}")


# --------------------------------------------- 1. dense against the restatement
DENSE_K = [1, 3, 4, 5, 9, 33, 65]  # the fold's client-group boundaries for U = 4 and U = 8


@pytest.mark.parametrize("P", [1, 7, 1001, 4099, 20483])
def test_dense_grouped_sum_bitwise(cuda, P):
    case = 0
    for K in DENSE_K:
        x = deltas(K, P)
        for G in (1, 2, 5):
            case += 1
            ids = ref.seeded_ids(K, G, seed=100 * K + G)
            w = np.array(weights_for(K, fractional=case % 2 == 0), dtype=F32)
            scales = (F32(1) / np.arange(1, G + 1, dtype=F32)).astype(F32)
            want = ref.grouped_sum_ref(x, w, ids, G, scales)
            # an aligned stride (16-byte units + tail) and an odd one (element units)
            for ld in ((P + 3) // 4 * 4 + 4, P + 1 + (P % 2)):
                xd = on_device(x, cuda, ld)
                out = torch.full((G, ld), float(SENTINEL), dtype=torch.float32, device=cuda)
                got = kernels.grouped_sum_dense(xd, w, ids, G, scales=scales, out=out[:, :P])
                check_grouped(got, want, sentinel_rows=True, what=f"K={K} P={P} G={G} ld={ld}")
                assert (out[:, P:] == float(SENTINEL)).all(), "wrote past P"
            # and without scales: the sums
            got = kernels.grouped_sum_dense(on_device(x, cuda, P + 4 - P % 4), w, ids, G)
            check_grouped(got, ref.grouped_sum_ref(x, w, ids, G))


# ------------------------------------------------ 2. regimes of the variant choice
# 16-byte units need 16-byte aligned row strides of x AND of the result; the shape the launch
# takes is asserted (fjagg_group_dense_shape), so a result that falls back to element units cannot
# pass for a regime. 600 003: E=4 x U=4; 1 048 579: E=8 x U=4 with the burst schedule (128 tiles x
# 3 groups < 2 x 256 CUs); 1 500 003: E=8 x U=4 interleaved (184 tiles x 3 groups).
@pytest.mark.parametrize("P,shape", [(600_003, 5), (1_048_579, 12), (1_500_003, 12)])
def test_dense_grouped_sum_regimes(cuda, P, shape):
    K, G = 40, 3
    ld = (P + 3) // 4 * 4 + 4
    gen = torch.Generator(device=cuda).manual_seed(P)
    store = torch.randn(K, ld, device=cuda, generator=gen)
    xd = store[:, :P]
    rng = np.random.RandomState(P)
    cols = np.unique(np.concatenate([rng.randint(0, P, 4096), np.arange(P - 16, P)]))
    ids = ref.seeded_ids(K, G, seed=P, force_edges=False)
    assert np.bincount(ids, minlength=G).min() >= 8
    w = np.array(weights_for(K, fractional=True), dtype=F32)
    scales = np.array([0.5, 0.25, 0.125], dtype=F32)
    tables = kernels.GroupTables(w, ids, G, scales).upload(cuda)
    out = torch.full((G, ld), float(SENTINEL), dtype=torch.float32, device=cuda)
    assert kernels.grouped_dense_shape(xd, out[:, :P], tables) == shape
    got = kernels.grouped_sum_dense(xd, w, ids, G, scales=scales, nontemporal=True, out=out[:, :P])
    cols_d = torch.from_numpy(cols).to(cuda)
    want = ref.grouped_sum_ref(xd[:, cols_d].cpu().numpy(), w, ids, G, scales)
    check_grouped(got[:, cols_d], want, what=f"P={P}")
    assert (out[:, P:] == float(SENTINEL)).all(), "wrote past P"
    # every column: the element-unit launch (a result with an odd row stride) partitions the axis
    # differently and must give the same bits
    odd = torch.empty(G, P + 1 + (P % 2), dtype=torch.float32, device=cuda)[:, :P]
    assert kernels.grouped_dense_shape(xd, odd, tables) == 0
    kernels.grouped_sum_dense(xd, w, ids, G, scales=scales, out=odd)
    assert torch.equal(odd.contiguous().view(torch.int32), got.contiguous().view(torch.int32))
    # the default result keeps 16-byte units whatever P is
    dflt = kernels.grouped_sum_dense(xd, w, ids, G, scales=scales)
    assert dflt.shape == (G, P) and kernels.grouped_dense_shape(xd, dflt, tables) == shape
    assert torch.equal(dflt.contiguous().view(torch.int32), got.contiguous().view(torch.int32))


def test_dense_small_shapes_take_one_unit_per_lane(cuda):
    """Below 128 Ki units, or below 8 members per group on average: E=1 x U=8 over 16-byte units."""
    w = np.ones(40, dtype=F32)
    x = torch.zeros(40, 20484, device=cuda)
    t = kernels.GroupTables(w, ref.seeded_ids(40, 3, 1, force_edges=False), 3, None).upload(cuda)
    assert kernels.grouped_dense_shape(x[:, :20483], torch.empty(3, 20484, device=cuda)[:, :20483], t) == 2
    big = torch.empty(40, 600_004, device=cuda)[:, :600_003]
    few = kernels.GroupTables(w, np.array([0, 1, 2, 0, 1] + [-1] * 35), 3, None).upload(cuda)
    assert kernels.grouped_dense_shape(big, torch.empty(3, 600_004, device=cuda)[:, :600_003], few) == 2
    assert kernels.grouped_dense_shape(big, torch.empty(3, 600_004, device=cuda)[:, :600_003], t) == 5


# ------------------------------------------------------------------ 3. isolation
def test_client_in_no_group_and_other_groups_are_isolated(cuda):
    K, P, G = 9, 1001, 2
    x = np.array(deltas(K, P))
    ids = np.array([0, 1, 0, -1, 1, 0, 1, -1, 0])
    w = np.array(weights_for(K, False), dtype=F32)
    clean = kernels.grouped_sum_dense(on_device(x, cuda, P + 3), w, ids, G).cpu().numpy()
    for poison in (np.nan, np.inf):
        y = x.copy()
        y[3, :] = poison
        y[7, ::2] = -poison
        got = kernels.grouped_sum_dense(on_device(y, cuda, P + 3), w, ids, G)
        assert_bits(got, clean, f"a -1 client's {poison} rows")
    y = x.copy()
    y[4, :] = np.nan  # a member of group 1
    got = kernels.grouped_sum_dense(on_device(y, cuda, P + 3), w, ids, G).cpu().numpy()
    assert np.isnan(got[1]).all()
    assert_bits(got[0], clean[0], "group 0 beside a NaN group 1")


# ------------------------------------- 4. signed zero, zero totals, empty groups
def test_signed_zero_zero_total_and_empty_groups(cuda):
    template = {"a": torch.zeros(5), "b": torch.zeros(1001)}
    K, G = 6, 4
    s = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    x = np.array(deltas(K, s.num_params))
    x[0] = -0.0
    x[1] = -0.0
    s.storage[:, : s.num_params].copy_(torch.from_numpy(x))
    ids = [0, 0, 1, 1, 2, -1]       # group 3 is empty
    weights = [2, 3, 2, -2, -1, 4]  # group 1 sums to 0, group 2 to -1
    out = torch.full((G, s.row_stride), float(SENTINEL), dtype=torch.float32, device=cuda)
    got = s.grouped_mean(weights, ids, G, out=out)
    want = ref.grouped_mean_ref(x, weights, ids, G)
    assert [g is None for g in got] == [w is None for w in want] == [False, True, True, True]
    flat0 = torch.cat([t.reshape(-1) for t in pytree.leaves_of(got[0])]).cpu().numpy()
    assert (flat0 == 0).all() and not np.signbit(flat0).any()  # +0, where tree_mean gives -0
    assert_bits(flat0, want[0], "group 0")
    mean = tu.tree_mean([(s.client(0), 2), (s.client(1), 3)])
    assert all(np.signbit(t.cpu().numpy()).all() for t in pytree.leaves_of(mean))
    assert (out[1:] == float(SENTINEL)).all(), "a group without a result had its row written"


# ------------------------------------------------------------- 5. pytree route
def _trees(K, cuda, seed):
    """K trees of 3 leaves (1, 1001 and 4099 elements); leaf "b" is a view at an odd element
    offset of its buffer, so it takes the per-leaf unaligned path."""
    x = deltas(K, 1 + 1001 + 4099, seed)
    trees = []
    for k in range(K):
        buf = torch.empty(1002, device=cuda)
        b = buf[1:]
        assert b.data_ptr() % 16 != 0
        b.copy_(torch.from_numpy(np.array(x[k, 1:1002])))
        trees.append({"a": torch.from_numpy(np.array(x[k, :1])).to(cuda), "b": b,
                      "c": torch.from_numpy(np.array(x[k, 1002:])).to(cuda).view(4099, 1)})
    return x, trees


def _running_sums(trees, weights, ids, G):
    """hyp_cluster.expectation_step (hyp_cluster.py:268-303) on the library's own tree ops: the
    loop of tests/algorithms_restated.py:_hc_expectation with tu = fedjax_amd.tree_util."""
    sums = [tu.tree_zeros_like(trees[0]) for _ in range(G)]
    totals = [0] * G
    for t, w, g in zip(trees, weights, ids):
        if g < 0:
            continue
        sums[g] = tu.tree_add(sums[g], tu.tree_weight(t, w))
        totals[g] += w
    return [tu.tree_inverse_weight(s, W) if W > 0 else None for s, W in zip(sums, totals)]


def _flat(tree):
    return np.concatenate([np.asarray(t.detach().cpu().numpy(), dtype=F32).reshape(-1)
                           for t in pytree.leaves_of(tree)])


@pytest.mark.parametrize("K", [5, 33])
@pytest.mark.parametrize("G", [2, 5])
def test_tree_grouped_mean_bitwise(cuda, K, G):
    x, trees = _trees(K, cuda, seed=G)
    ids = ref.seeded_ids(K, G, seed=K + G)
    weights = weights_for(K, fractional=(K + G) % 2 == 0)
    if G == 5:  # a group whose total is 0: two members, weights w and -w
        ids[:2] = 1
        weights[1] = -weights[0]
    got = tu.tree_grouped_mean(list(zip(trees, weights)), ids, G)
    want = ref.grouped_mean_ref(x, weights, ids, G)
    loop = _running_sums(trees, weights, ids, G)
    assert [g is None for g in got] == [w is None for w in want] == [r is None for r in loop]
    assert any(w is None for w in want) or G == 2
    for g in range(G):
        if want[g] is None:
            continue
        assert pytree.flatten(got[g])[1] == pytree.flatten(trees[0])[1]
        assert [tuple(t.shape) for t in pytree.leaves_of(got[g])] == [(1,), (1001,), (4099, 1)]
        assert_bits(_flat(got[g]), want[g], f"group {g} against the restatement")
        assert_bits(_flat(got[g]), _flat(loop[g]), f"group {g} against the running-sum loop")


def test_tree_grouped_mean_reference_kat(cuda):
    """hyp_cluster_test.py:366-403 through _hc_expectation on the library (one running sum per
    cluster) and through tree_grouped_mean: the same bits, and the reference's numbers."""
    to_leaf = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(cuda)
    host = lambda t: np.asarray(pytree.leaves_of(t)[0].detach().cpu().numpy())
    clients = ar._HC_CLIENTS + [(b"4", np.array([-0.1], F32))]
    idmap = {b"0": 0, b"1": 0, b"2": 1, b"3": 1, b"4": 0}
    params = [1., -1., 3.14]
    loop = ar._hc_expectation(tu, to_leaf, host, params, idmap, clients)
    pairs = [(to_leaf(ar._hc_delta(params[idmap[cid]], x)), len(x)) for cid, x in clients]
    got = tu.tree_grouped_mean(pairs, [idmap[cid] for cid, _ in clients], 3)
    assert got[2] is None and loop[2] is None
    for g in range(2):
        assert_bits(got[g], loop[g], f"cluster {g}")
    np.testing.assert_allclose(got[0].cpu().numpy(), (-0.1 + 0.1 * 2 + 1.1) / 4, rtol=1e-7)
    np.testing.assert_allclose(got[1].cpu().numpy(), (0.1 - 0.1 * 3) / 4, rtol=1e-6)


def test_tree_grouped_mean_rejects_other_dtypes(cuda):
    pairs = [({"a": torch.zeros(4, dtype=torch.bfloat16, device=cuda)}, 1.0)]
    with pytest.raises(TypeError):
        tu.tree_grouped_mean(pairs, [0], 1)
    s = slab_mod.ClientDeltaSlab({"a": torch.zeros(4)}, 2, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(TypeError):
        s.grouped_mean([1, 1], [0, 0], 1)


# -------------------------------------------------------------- 6. slab surface
def test_slab_grouped_mean_surface(cuda):
    template = {"w": torch.zeros(33, 31), "b": torch.zeros(7), "s": torch.zeros(())}
    K, G = 33, 5
    s = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    x = deltas(K, s.num_params, seed=3)
    s.storage[:, : s.num_params].copy_(torch.from_numpy(np.array(x)))
    ids = ref.seeded_ids(K, G, seed=6)
    weights = weights_for(K, fractional=False)
    got = s.grouped_mean(weights, ids, G)
    want = ref.grouped_mean_ref(x, weights, ids, G)
    views = tu.tree_grouped_mean([(s.client(k), weights[k]) for k in range(K)], ids, G)
    assert [g is None for g in got] == [w is None for w in want] == [v is None for v in views]
    for g in range(G):
        if want[g] is None:
            continue
        assert pytree.flatten(got[g])[1] == pytree.flatten(template)[1]
        assert [tuple(t.shape) for t in pytree.leaves_of(got[g])] == [tuple(t.shape) for t in
                                                                       pytree.leaves_of(s.client(0))]
        assert_bits(_flat(got[g]), want[g], f"group {g} against the restatement")
        assert_bits(_flat(got[g]), _flat(views[g]), f"group {g} against tree_grouped_mean")
    # one group of everybody, positive products: slab.mean's bits
    s.storage.abs_()
    one = s.grouped_mean(weights, [0] * K, 1)[0]
    assert_bits(_flat(one), _flat(s.mean(weights)), "all clients in group 0 against slab.mean")


# ------------------------------------------------------------- 7. graph capture
def test_slab_grouped_mean_graph_capture(cuda):
    template = {"w": torch.zeros(4099), "b": torch.zeros(5)}
    K, G = 9, 3
    s = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    s.fill_synthetic(seed=1)
    ids = [0, 1, 0, -1, 1, 0, 1, 2, 0]
    weights = weights_for(K, fractional=False)
    out = torch.zeros(G, s.row_stride, device=cuda)
    st = torch.cuda.Stream()
    s.grouped_mean(weights, ids, G, out=out)  # eager: the tables go up once and stay
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = s.grouped_mean(weights, ids, G, out=out)
    for seed in (2, 3):
        s.fill_synthetic(seed=seed)
        out.fill_(float(SENTINEL))
        g.replay()
        torch.cuda.synchronize()
        got = [_flat(r) for r in res]
        want = [_flat(r) for r in s.grouped_mean(weights, ids, G)]
        for a, b in zip(got, want):
            assert_bits(a, b, f"replay with seed {seed}")
    # a capture that would need a table upload (other weights than the latest eager call's) would
    # replay a stale staging buffer: it is refused at capture time, and the stream works afterwards
    s.grouped_mean(weights, ids, G)  # (the eager calls above left these tables behind)
    other = [w + 1 for w in weights]
    g1, st1 = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st1):
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g1, stream=st1):
                s.grouped_mean(other, ids, G)
    torch.cuda.synchronize()
    x = s.rows.cpu().numpy()
    for a, b in zip(s.grouped_mean(other, ids, G), ref.grouped_mean_ref(x, other, ids, G)):
        assert_bits(_flat(a), b, "eager after the refused capture")
