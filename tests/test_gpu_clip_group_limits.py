"""The clipped and the grouped weighted mean at their documented limits, and every kernel
instantiation behind their pytree entry points, against the numpy restatements
(tests/clipped_mean_ref.py, tests/grouped_mean_ref.py). All shapes are small on purpose.

* the fused clipped squares up to their 4096 clients (four waves x 4096 floats of dynamic LDS:
  exactly 64 KiB) and the refusal at 4097; the fold without squares beyond it;
* the norm pass of tree_clipped_mean / tree_l2_norms over more than 65535 (client, leaf) rows
  (several fjagg_l2sq_rows launches);
* fjagg_wsum_clip_ptrs and fjagg_wsum_group_ptrs called with raw plan images so that every
  k_ptrs_clip<V, NT, L2, BURST> and k_ptrs_group<V, NT, BURST> the library can launch runs:
  16-byte and element units, non-temporal loads, squares on and off, the burst and the
  interleaved schedule (chosen from the plan's own workgroup count, asserted);
* groups of more than 1000 members, more groups than clients, 65535 groups, the refusal of
  65536, no members at all;
* tree_grouped_mean over 64 leaves of every kind it canonicalises.

Means are compared bit for bit with every NaN one pattern; norms and squares are held to 2e-6
of their float64 values, the bound the project holds all its norms to.
"""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, pytree, slab as slab_mod, tree_util as tu
from tests import clipped_mean_ref as cref
from tests import grouped_mean_ref as gref
from tests.clipped_mean_ref import l2sq_rows_ref
from tests.test_gpu_clip_group_fuzz import assert_bits, check_clipped, flat

pytestmark = pytest.mark.gpu
F32 = np.float32
NORM_RTOL = 2e-6
SENTINEL = -1234.5
EUNSUPPORTED = -3


@functools.lru_cache(maxsize=None)
def deltas(K, P, seed=0):
    """Seeded CPU normal deltas, client k scaled by 2**((k % 5) - 2): float32 [K, P]."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * K + P)
    x = torch.randn(K, P, generator=g, dtype=torch.float32)
    x *= torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], dtype=torch.float32)[:, None]
    x = x.numpy()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def factors(K, seed=0):
    """Arbitrary factors in [0.25, 1] with every third exactly 1, and integer weights."""
    rng = np.random.RandomState(31 * K + seed)
    c = rng.uniform(0.25, 1.0, K).astype(F32)
    c[::3] = 1.0
    w = rng.randint(1, 500, K).astype(F32)
    return c, w


def on_device(x, dev, ld):
    """x [K, P] as a device view with row stride ld > P (the padding holds NaN: never read)."""
    K, P = x.shape
    store = torch.full((K, ld), float("nan"), dtype=torch.float32, device=dev)
    store[:, :P].copy_(torch.from_numpy(np.array(x)))
    return store[:, :P]


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the cached deltas are read-only)


def squares_close(got, products, what):
    p = np.asarray(products, dtype=np.float64)
    want = (p * p).sum(axis=1)
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    assert (err <= NORM_RTOL * want).all(), f"{what}: squares off by {(err / want).max():.3e}"


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------- 1. client limit of the clipped fold
@pytest.mark.parametrize("K", [129, 1024, 4096])
def test_clipped_dense_with_squares_up_to_the_client_limit(cuda, K):
    P = 1027
    x = deltas(K, P)
    c, w = factors(K)
    scale = F32(1.0 / float(w.astype(np.float64).sum()))
    want = cref.clipped_fold_ref(x, w, c, scale)
    wd, cd = to_dev(w, cuda), to_dev(c, cuda)
    for ld in (1032, 1029):  # 16-byte units + tail, and element units
        xd = on_device(x, cuda, ld)
        out, l2sq = kernels.clipped_sum_dense(xd, wd, cd, scale=float(scale), with_clipped_l2sq=True)
        assert_bits(out, want, f"K={K} ld={ld} mean")
        squares_close(l2sq, cref.clipped_products(x, c), f"K={K} ld={ld}")


def test_clipped_squares_beyond_the_client_limit_are_refused(cuda):
    K, P = 4097, 64
    x = torch.ones(K, P, device=cuda)
    w, c = torch.ones(K, device=cuda), torch.full((K,), 0.5, device=cuda)
    out = torch.full((P,), SENTINEL, device=cuda)
    l2 = torch.full((K,), SENTINEL, device=cuda)
    lib = _lib.load()
    need = max(int(lib.fjagg_wsum_clip_workspace_bytes(K, P)), 1 << 16)
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    rc = lib.fjagg_wsum_clip_dense(_lib.F32, x.data_ptr(), P, K, P, w.data_ptr(), c.data_ptr(), 1.0, out.data_ptr(),
                                   l2.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream_of(cuda))
    assert rc == EUNSUPPORTED
    image = torch.tensor([x[k].data_ptr() for k in range(K)] + [out.data_ptr(), P, 0, P // 4], dtype=torch.int64,
                         device=cuda)
    rc = lib.fjagg_wsum_clip_ptrs(_lib.F32, image.data_ptr(), 1, K, 1, w.data_ptr(), c.data_ptr(), 1.0,
                                  l2.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream_of(cuda))
    assert rc == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (l2 == SENTINEL).all()
    with pytest.raises(_lib.FjaggError):
        kernels.clipped_sum_dense(x, w, c, with_clipped_l2sq=True)
    sl = slab_mod.ClientDeltaSlab({"a": np.zeros(P, F32)}, K, device=cuda)
    sl.rows.copy_(x)
    with pytest.raises(ValueError):
        sl.clipped_mean([1] * K, 1.0)
    with pytest.raises(ValueError):
        tu.tree_clipped_mean([({"a": x[k]}, 1) for k in range(K)], 1.0)
    # the same image without the squares is a valid call: 4097 rows of ones, halved and summed
    _lib.call("fjagg_wsum_clip_ptrs", _lib.F32, image.data_ptr(), 1, K, 1, w.data_ptr(), c.data_ptr(), 1.0,
              None, 0, None, 0, stream_of(cuda))
    assert (out == 0.5 * K).all()


def test_clipped_dense_without_squares_has_no_client_limit(cuda):
    K, P = 5000, 1027
    x = deltas(K, P)
    c, w = factors(K)
    scale = F32(1.0 / float(w.astype(np.float64).sum()))
    want = cref.clipped_fold_ref(x, w, c, scale)
    for ld in (1032, 1029):
        got = kernels.clipped_sum_dense(on_device(x, cuda, ld), to_dev(w, cuda), to_dev(c, cuda), scale=float(scale))
        assert_bits(got, want, f"K={K} ld={ld}")


def row_trees(xd, sizes, shapes=None):
    """One tree (a list of leaves) per row of the device tensor xd: leaf i is the view of the
    next sizes[i] elements of the row."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    shapes = shapes or [(n,) for n in sizes]
    return [[xd[k, o:o + n].view(s) for o, n, s in zip(offs[:-1], sizes, shapes)] for k in range(xd.shape[0])]


def test_tree_clipped_mean_at_the_client_limit(cuda):
    K, sizes = 4096, [1, 67, 1001]
    x = deltas(K, sum(sizes), seed=1)
    xd = on_device(x, cuda, 1072)
    trees = row_trees(xd, sizes, [(), (67,), (7, 143)])
    weights = [int(v) for v in np.random.RandomState(3).randint(1, 500, K)]
    case = dict(x=x, K=K, weights=weights, max_norm=float(np.median(cref.f64_norms(x))))
    got = tu.tree_clipped_mean(list(zip(trees, weights)), case["max_norm"])
    assert [tuple(t.shape) for t in got.mean] == [(), (67,), (7, 143)]
    fac = check_clipped(case, got, cuda, "pytree K=4096")
    assert (fac < 1).any() and (fac == 1).any()


# --------------------------------------------------------- 2. row split of the norm pass
def test_norm_pass_over_more_than_65535_rows(cuda):
    K, L = 1100, 64
    sizes = [i % 10 for i in range(L)]
    assert K * L > 65535 and 65535 // L < K  # two fjagg_l2sq_rows launches
    P = sum(sizes)
    x = deltas(K, P, seed=2)
    xd = on_device(x, cuda, P + 5)  # one buffer per client: its row
    trees = row_trees(xd, sizes)
    n64 = cref.f64_norms(x)
    norms = tu.tree_l2_norms(trees).cpu().numpy()
    assert norms.shape == (K,) and (np.abs(norms - n64) <= NORM_RTOL * n64).all(), "tree_l2_norms"
    weights = [int(v) for v in np.random.RandomState(4).randint(1, 500, K)]
    case = dict(x=x, K=K, weights=weights, max_norm=float(np.median(n64)))
    got = tu.tree_clipped_mean(list(zip(trees, weights)), case["max_norm"])
    fac = check_clipped(case, got, cuda, "pytree K=1100 L=64")
    assert (fac < 1).any() and (fac == 1).any()
    # clients on both sides of the split (row 1023 is the first launch's last) are clipped or not by
    # their OWN norm: a norm written to another client's slot would fail the 2e-6 bound above
    assert [tuple(t.shape) for t in got.mean] == [(n,) for n in sizes]


def test_norm_rows_keep_their_summation_order(cuda):
    """The norms of tree_l2_norms, tree_clipped_mean and ClientDeltaSlab.clipped_mean, bit for
    bit: the correctly rounded root of l2sq_rows_ref. Leaves below and above the eight loads a
    lane keeps in flight (2048 elements), with a remainder, and of more than one block."""
    K, sizes = 5, [1, 67, 2047, 2048, 2049, 0, 6000, 65536 + 4097]
    x = deltas(K, sum(sizes), seed=21)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    want = np.sqrt(np.array([l2sq_rows_ref([x[k, o:o + n] for o, n in zip(offs[:-1], sizes)]) for k in range(K)],
                            dtype=F32))
    xd = on_device(x, cuda, sum(sizes) + 3)
    trees = row_trees(xd, sizes)
    assert_bits(tu.tree_l2_norms(trees), want, "tree_l2_norms")
    big = 1e30  # nothing is clipped
    assert_bits(tu.tree_clipped_mean([(t, 1) for t in trees], big).norms, want, "tree_clipped_mean norms")
    sl = slab_mod.ClientDeltaSlab([np.zeros(n, F32) for n in sizes], K, device=cuda)
    sl.rows.copy_(to_dev(x, cuda))
    assert_bits(sl.clipped_mean([1] * K, big).norms, want, "slab clipped_mean norms")


# -------------------------------------------- 3. every k_ptrs_clip / k_ptrs_group instantiation
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def leaves_for_plan(dev, unaligned, want_blocks, groups=1):
    """Leaf sizes whose plan has fewer (want_blocks == "few") or at least (== "many") 2 x CUs
    workgroups over ``groups`` slots, from the plan's own block count."""
    limit = 2 * cus(dev)
    if want_blocks == "few":
        sizes = [1027, 5, 4099]
        nblk = len(kernels.ptrs_plan(_lib.F32, sizes, unaligned)) // 2
        assert nblk * groups < limit
        return sizes, nblk
    for big in (70_001, 140_003, 300_001, 600_003, 1_100_003, 2_200_003, 4_400_003, 8_800_003):
        sizes = [big, 7, 1027]
        nblk = len(kernels.ptrs_plan(_lib.F32, sizes, unaligned)) // 2
        if nblk * groups >= limit:
            return sizes, nblk
    raise AssertionError(f"no leaf size reaches {limit} workgroups")


def leaf_buffers(x, sizes, dev, misalign):
    """x [K, P] on the device as K x L leaves: [K][L] tensors, each 16-byte aligned or (misalign)
    at element offset 1 of its allocation (4-byte aligned only)."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    xd = to_dev(x, dev)
    rows = []
    for k in range(x.shape[0]):
        row = []
        for o, n in zip(offs[:-1], sizes):
            buf = torch.empty(n + 8, dtype=torch.float32, device=dev)
            leaf = buf[1:1 + n] if misalign else buf[:n]
            leaf.copy_(xd[k, o:o + n])
            assert leaf.data_ptr() % 16 == (4 if misalign else 0)
            row.append(leaf)
        rows.append(row)
    return rows


def out_buffers(G, sizes, dev, misalign, init=None):
    """[G][L] output leaves inside sentinel-filled allocations (returned too, to check the rims)."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    outs, stores = [], []
    for g in range(G):
        row = []
        for i, n in enumerate(sizes):
            buf = torch.full((n + 12,), SENTINEL, dtype=torch.float32, device=dev)
            leaf = buf[5:5 + n] if misalign else buf[4:4 + n]
            if init is not None:
                leaf.copy_(to_dev(init[offs[i]:offs[i] + n], dev))
            row.append(leaf)
            stores.append((buf, leaf))
        outs.append(row)
    return outs, stores


def assert_rims(stores, what):
    for buf, leaf in stores:
        a = (leaf.data_ptr() - buf.data_ptr()) // 4
        assert (buf[:a] == SENTINEL).all() and (buf[a + leaf.numel():] == SENTINEL).all(), f"{what}: wrote past a leaf"


@pytest.mark.parametrize("blocks", ["few", "many"])
@pytest.mark.parametrize("unaligned", [False, True])
def test_every_clip_ptrs_kernel(cuda, unaligned, blocks):
    """fjagg_wsum_clip_ptrs over a raw image (in_ptrs[K*L] | out_ptrs[L] | leaf_n[L] | blocks):
    FJAGG_UNALIGNED x NONTEMPORAL x squares x schedule x SCALE / ACCUMULATE, each against the
    restatement bit for bit (so all of them agree with each other)."""
    K = 3
    sizes, nblk = leaves_for_plan(cuda, unaligned, blocks)
    assert (nblk < 2 * cus(cuda)) == (blocks == "few")  # the non-square launch's schedule rule
    P, L = sum(sizes), len(sizes)
    x = deltas(K, P, seed=7)
    init = deltas(1, P, seed=8)[0]
    c = np.array([0.37, 1.0, 0.81], dtype=F32)
    w = np.array([3.0, 211.0, 0.625], dtype=F32)
    scale = F32(1.0 / 214.625)
    rows = leaf_buffers(x, sizes, cuda, misalign=unaligned)
    plan = kernels.ptrs_plan(_lib.F32, sizes, unaligned)
    assert len(plan) == 2 * nblk
    wd, cd = to_dev(w, cuda), to_dev(c, cuda)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.fjagg_wsum_clip_ptrs_workspace_bytes(K, nblk)), 4), dtype=torch.uint8, device=cuda)
    products = cref.clipped_products(x, c)
    wants = {fl: cref.clipped_fold_ref(x, w, c, scale if fl & _lib.SCALE else None,
                                       init=init if fl & _lib.ACCUMULATE else None)
             for fl in (0, _lib.SCALE, _lib.SCALE | _lib.ACCUMULATE, _lib.ACCUMULATE)}
    ran = 0
    for nt in (False, True):
        for squares in (True, False):
            for fl in (0, _lib.SCALE, _lib.SCALE | _lib.ACCUMULATE, _lib.ACCUMULATE):
                acc = bool(fl & _lib.ACCUMULATE)
                outs, stores = out_buffers(1, sizes, cuda, misalign=unaligned, init=init if acc else None)
                image = np.concatenate([np.array([[t.data_ptr() for t in r] for r in rows], dtype=np.int64).ravel(),
                                        np.array([t.data_ptr() for t in outs[0]], dtype=np.int64),
                                        np.array(sizes, dtype=np.int64), plan])
                image_dev = to_dev(image, cuda)
                l2 = torch.full((K,), SENTINEL, device=cuda)
                flags = fl | (_lib.NONTEMPORAL if nt else 0) | (_lib.UNALIGNED if unaligned else 0)
                _lib.call("fjagg_wsum_clip_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk, wd.data_ptr(),
                          cd.data_ptr(), float(scale) if fl & _lib.SCALE else 1.0, l2.data_ptr() if squares else None,
                          flags, ws.data_ptr() if squares else None, ws.numel() if squares else 0, stream_of(cuda))
                what = f"unaligned={unaligned} {blocks} nt={nt} squares={squares} flags={fl}"
                assert_bits(torch.cat(outs[0]), wants[fl], what)
                assert_rims(stores, what)
                if squares:
                    squares_close(l2, products, what)
                else:
                    assert (l2 == SENTINEL).all(), what
                ran += 1
    assert ran == 16


def group_case(K, G, seed):
    """ids with two clients in no group and group G-1 empty; fractional weights; scales."""
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, G - 1, size=K).astype(np.int64)
    ids[:G - 1] = np.arange(G - 1)  # every other group has a member
    ids[rng.permutation(K)[G - 1:][:2]] = -1
    w = rng.uniform(0.1, 3.0, K).astype(F32)
    scales = (F32(1) / np.arange(2, G + 2, dtype=F32)).astype(F32)
    return ids, w, scales


@pytest.mark.parametrize("blocks", ["few", "many"])
@pytest.mark.parametrize("unaligned", [False, True])
def test_every_group_ptrs_kernel(cuda, unaligned, blocks):
    """fjagg_wsum_group_ptrs over a raw image (in_ptrs[M*L] in member order | out_ptrs[G*L] |
    leaf_n[L] | blocks) and device tables seg | gorder | wperm | gscale: FJAGG_UNALIGNED x
    NONTEMPORAL x schedule x SCALE against grouped_sum_ref, bit for bit; a group without members
    keeps its sentinel."""
    K, G = 12, 4
    ids, w, scales = group_case(K, G, seed=5)
    nonempty = 3
    assert len(set(ids[ids >= 0])) == nonempty and (ids == -1).sum() >= 1
    sizes, nblk = leaves_for_plan(cuda, unaligned, blocks, groups=nonempty)
    assert (nblk * nonempty < 2 * cus(cuda)) == (blocks == "few")  # launch_ptrs_group's schedule rule
    P, L = sum(sizes), len(sizes)
    x = deltas(K, P, seed=9)
    rows = leaf_buffers(x, sizes, cuda, misalign=unaligned)
    plan = kernels.ptrs_plan(_lib.F32, sizes, unaligned)
    tables = kernels.GroupTables(w, ids, G, scales)
    M = tables.M
    in_ptrs = np.array([[t.data_ptr() for t in rows[k]] for k in tables.order], dtype=np.int64)
    t32 = tables.host[M:]  # seg | gorder | wperm | gscale
    words = np.zeros((t32.size + 1) // 2, dtype=np.int64)
    words.view(np.int32)[: t32.size] = t32
    ran = 0
    for nt in (False, True):
        for scaled in (False, True):
            outs, stores = out_buffers(G, sizes, cuda, misalign=unaligned)
            out_ptrs = np.array([[t.data_ptr() for t in r] for r in outs], dtype=np.int64)
            image = np.concatenate([in_ptrs.ravel(), out_ptrs.ravel(), np.array(sizes, dtype=np.int64), plan, words])
            image_dev = to_dev(image, cuda)
            seg_p = image_dev.data_ptr() + 8 * (image.size - words.size)
            gorder_p, wperm_p, gscale_p = seg_p + 4 * (G + 1), seg_p + 4 * (2 * G + 1), seg_p + 4 * (2 * G + 1 + M)
            flags = (_lib.SCALE if scaled else 0) | (_lib.NONTEMPORAL if nt else 0) | (_lib.UNALIGNED if unaligned else 0)
            _lib.call("fjagg_wsum_group_ptrs", _lib.F32, image_dev.data_ptr(), L, K, M, G, nblk, seg_p, wperm_p,
                      gscale_p, gorder_p, tables.seg.ctypes.data, flags, stream_of(cuda))
            what = f"unaligned={unaligned} {blocks} nt={nt} scaled={scaled}"
            want = gref.grouped_sum_ref(x, w, ids, G, scales if scaled else None)
            assert [v is None for v in want] == [False, False, False, True]
            for g in range(G):
                got = torch.cat(outs[g])
                if want[g] is None:
                    assert (got == SENTINEL).all(), f"{what}: the empty group's leaves were written"
                else:
                    assert_bits(got, want[g], f"{what} group {g}")
            assert_rims(stores, what)
            ran += 1
    assert ran == 4


@pytest.mark.parametrize("blocks", ["few", "many"])
def test_tree_grouped_mean_with_nontemporal_loads(cuda, blocks):
    K, G = 12, 4
    ids, w, _ = group_case(K, G, seed=6)
    sizes, _ = leaves_for_plan(cuda, [False, True, False], blocks, groups=3)
    x = deltas(K, sum(sizes), seed=10)
    rows = leaf_buffers(x, sizes, cuda, misalign=False)
    for k in range(K):  # the middle leaf at an odd element offset: per-leaf element units
        buf = torch.empty(sizes[1] + 8, device=cuda)
        buf[1:1 + sizes[1]].copy_(rows[k][1])
        rows[k][1] = buf[1:1 + sizes[1]]
    weights = [float(v) for v in w]
    want = gref.grouped_mean_ref(x, weights, ids, G)
    plain = tu.tree_grouped_mean(list(zip(rows, weights)), ids, G)
    before = tu.NONTEMPORAL_MIN_BYTES
    tu.set_nontemporal_min_bytes(0)
    try:
        got = tu.tree_grouped_mean(list(zip(rows, weights)), ids, G)
    finally:
        tu.set_nontemporal_min_bytes(before)
    assert tu.NONTEMPORAL_MIN_BYTES == before == 256 << 20
    assert [v is None for v in got] == [v is None for v in want] == [v is None for v in plain]
    for g in range(G):
        if want[g] is not None:
            assert_bits(flat(got[g], cuda), want[g], f"{blocks} nontemporal group {g}")
            assert_bits(flat(plain[g], cuda), want[g], f"{blocks} group {g}")


# -------------------------------------------------------------------- 4. group limits
def check_both_routes(cuda, x, weights, ids, G, sizes, what):
    """kernels.grouped_sum_dense (sentinel rows), ClientDeltaSlab.grouped_mean and
    tree_grouped_mean over the same rows against the restatement; returns the restatement."""
    K, P = x.shape
    want = gref.grouped_mean_ref(x, weights, ids, G)
    xd = on_device(x, cuda, (P + 3) // 4 * 4 + 4)
    w32 = np.array([F32(v) for v in weights], dtype=F32)
    # dense: the raw sums of every group with members, untouched rows elsewhere
    sums = gref.grouped_sum_ref(x, w32, ids, G)
    out = torch.full((G, P + 3), SENTINEL, dtype=torch.float32, device=cuda)
    got = kernels.grouped_sum_dense(xd, w32, ids, G, out=out[:, :P]).cpu().numpy()
    empty = np.array([s is None for s in sums])
    assert (got[empty] == SENTINEL).all(), f"{what}: dense rows of empty groups were written"
    full = np.flatnonzero(~empty)
    assert_bits(got[full], np.stack([sums[g] for g in full]) if full.size else np.zeros((0, P), F32), what + " dense")
    assert (out[:, P:] == SENTINEL).all(), f"{what}: dense wrote past P"
    # slab
    sl = slab_mod.ClientDeltaSlab([np.zeros(n, F32) for n in sizes], K, device=cuda)
    sl.rows.copy_(to_dev(x, cuda))
    sout = torch.full((G, sl.row_stride), SENTINEL, dtype=torch.float32, device=cuda)
    means = sl.grouped_mean(weights, ids, G, out=sout)
    assert [m is None for m in means] == [m is None for m in want], f"{what}: slab None pattern"
    none = np.array([m is None for m in want])
    shost = sout.cpu().numpy()
    assert (shost[none] == SENTINEL).all(), f"{what}: slab rows of groups without a mean were written"
    alive = np.flatnonzero(~none)
    if alive.size:
        assert_bits(shost[alive][:, :P], np.stack([want[g] for g in alive]), what + " slab")
    # pytree: every client's row as leaves of these sizes
    trees = row_trees(xd, sizes)
    tmeans = tu.tree_grouped_mean(list(zip(trees, weights)), ids, G)
    assert [m is None for m in tmeans] == [m is None for m in want], f"{what}: pytree None pattern"
    if alive.size:
        rows = torch.stack([torch.cat([t.reshape(-1) for t in tmeans[g]]) for g in alive])
        assert_bits(rows, np.stack([want[g] for g in alive]), what + " pytree")
        assert [tuple(t.shape) for t in tmeans[alive[0]]] == [(n,) for n in sizes]
    return want


def test_groups_of_more_than_a_thousand_members(cuda):
    K, G, sizes = 4096, 3, [1, 67, 1001]
    x = deltas(K, sum(sizes), seed=11)
    rng = np.random.RandomState(12)
    ids = rng.randint(0, G, size=K).astype(np.int64)
    ids[rng.rand(K) < 0.02] = -1
    assert np.bincount(ids[ids >= 0], minlength=G).min() > 1000
    weights = [int(v) for v in rng.randint(1, 500, K)]
    want = check_both_routes(cuda, x, weights, ids, G, sizes, "K=4096 G=3")
    assert all(m is not None for m in want)


def test_more_groups_than_clients(cuda):
    K, sizes = 300, [1, 67, 1001]
    G = K + 5
    x = deltas(K, sum(sizes), seed=13)
    rng = np.random.RandomState(14)
    ids = rng.permutation(G)[:K].astype(np.int64)  # every client alone in its group, 5 groups empty
    weights = [float(v) for v in rng.uniform(0.1, 3.0, K)]
    want = check_both_routes(cuda, x, weights, ids, G, sizes, "K=300 G=305")
    assert sum(m is None for m in want) == 5


def test_the_most_groups_the_grid_takes(cuda):
    K, G, sizes = 9, 65535, [5]
    x = deltas(K, 5, seed=15)
    ids = np.array([0, 65534, 1, -1, 32768, 65534, 0, 4097, 65533], dtype=np.int64)
    weights = [3, 1, 4, 1, 5, 9, 2, 6, 5]
    want = check_both_routes(cuda, x, weights, ids, G, sizes, "G=65535")
    assert sum(m is not None for m in want) == 6 and want[65534] is not None


def test_one_group_too_many_is_refused(cuda):
    K, G, P = 9, 65536, 5
    x = deltas(K, P, seed=15)
    xd = on_device(x, cuda, 8)
    ids = np.array([0, 65535, 1, -1, 32768, 65535, 0, 4097, 65533], dtype=np.int64)
    w = np.arange(1, K + 1, dtype=F32)
    out = torch.full((G, 8), SENTINEL, dtype=torch.float32, device=cuda)
    with pytest.raises(_lib.FjaggError, match="65535"):
        kernels.grouped_sum_dense(xd, w, ids, G, out=out[:, :P])
    sl = slab_mod.ClientDeltaSlab([np.zeros(P, F32)], K, device=cuda)
    sl.rows.copy_(to_dev(x, cuda))
    with pytest.raises(_lib.FjaggError, match="65535"):
        sl.grouped_mean([float(v) for v in w], ids, G, out=out)
    with pytest.raises(_lib.FjaggError, match="65535"):
        tu.tree_grouped_mean([([xd[k]], float(w[k])) for k in range(K)], ids, G)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_no_members_at_all(cuda):
    K, G, sizes = 9, 4, [5, 1001]
    x = deltas(K, sum(sizes), seed=16)
    ids = np.full(K, -1, dtype=np.int64)
    want = check_both_routes(cuda, x, list(range(1, K + 1)), ids, G, sizes, "M=0")
    assert want == [None] * G


# --------------------------------------------- 5. leaf kinds of tree_grouped_mean
def test_tree_grouped_mean_leaf_kinds(cuda):
    K, G, L = 9, 3, 64
    shapes = [(0,), (), (3, 5), (67,), (2, 3, 4)] + [((i * 7) % 23 + 1,) for i in range(L - 5)]
    kinds = ["own", "own", "host", "f64", "noncontig"] + ["own", "host", "f64", "noncontig", "view"] * 12
    kinds = kinds[:L]
    sizes = [int(np.prod(s, dtype=np.int64)) for s in shapes]
    assert len(shapes) == L and sizes[0] == 0 and shapes[1] == ()
    x = deltas(K, sum(sizes), seed=17)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    trees = []
    for k in range(K):
        leaves = {}
        for i, (s, n, kind) in enumerate(zip(shapes, sizes, kinds)):
            v = np.array(x[k, offs[i]:offs[i] + n])
            if kind == "host":
                leaf = v.reshape(s)
            elif kind == "f64":
                leaf = to_dev(v.astype(np.float64), cuda).reshape(s)
            elif kind == "noncontig":
                b = torch.zeros(2 * n, device=cuda)
                b[::2] = to_dev(v, cuda)
                leaf = b[::2].reshape(s)
                assert n <= 1 or not leaf.is_contiguous()
            elif kind == "view":
                b = torch.zeros(n + 3, device=cuda)
                b[1:1 + n] = to_dev(v, cuda)
                leaf = b[1:1 + n].view(s)
            else:
                leaf = to_dev(v, cuda).reshape(s)
            leaves["leaf%02d" % i] = leaf
        trees.append(leaves)
    ids = np.array([0, 1, 0, -1, 1, 0, 1, 0, 1], dtype=np.int64)  # group 2 is empty
    weights = [2, 3.5, 1, 7, 4, 0.25, 6, 5, 1]
    want = gref.grouped_mean_ref(x, weights, ids, G)
    got = tu.tree_grouped_mean(list(zip(trees, weights)), ids, G)
    assert [m is None for m in got] == [m is None for m in want] == [False, False, True]
    for g in range(2):
        assert list(got[g]) == sorted(trees[0])
        assert [tuple(t.shape) for t in pytree.leaves_of(got[g])] == shapes
        assert all(t.dtype == torch.float32 and t.is_cuda for t in pytree.leaves_of(got[g]))
        assert_bits(flat(got[g], cuda), want[g], f"group {g}")
    for k in range(K):  # the inputs are as they were
        assert_bits(flat(trees[k], cuda), x[k], f"client {k}'s leaves")
