"""Clipped weighted mean on the GPU: per-client norm clipping inside the fold
(fjagg_clip_scales, fjagg_wsum_clip_dense / _ptrs, fjagg_clip_finish and the Python surface
over them) against the numpy float32 restatement in tests/clipped_mean_ref.py.

The fold is held to the restatement bit for bit for ANY device factor vector c; norms are
held to 2e-6 of a float64 norm, the bound the project holds all its norms to (their
reduction order is the library's own). Bit patterns are compared with every NaN mapped to
one pattern: IEEE 754 leaves the sign and payload of a generated NaN to the implementation
(x86 makes inf * 0 a negative quiet NaN; a GPU need not), and neither XLA nor the reference
pins them.
"""
import functools

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, pytree, slab as slab_mod, tree_util as tu
from tests import clipped_mean_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
NORM_RTOL = 2e-6


def nbits(a):
    """uint32 bit patterns with every NaN mapped to 0x7fc00000."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def assert_bits(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    g, w = nbits(got).reshape(-1), nbits(want).reshape(-1)
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


@functools.lru_cache(maxsize=None)
def factors(K, seed=0):
    """Arbitrary factors in [0.25, 1] with a few entries exactly 1, and integer weights."""
    rng = np.random.RandomState(31 * K + seed)
    c = rng.uniform(0.25, 1.0, K).astype(F32)
    c[::3] = 1.0
    w = rng.randint(1, 500, K).astype(F32)
    c.setflags(write=False)
    w.setflags(write=False)
    return c, w


def on_device(x, dev, ld):
    """x [K, P] as a device view with row stride ld > P (the padding holds NaN: never read)."""
    K, P = x.shape
    store = torch.full((K, ld), float("nan"), dtype=torch.float32, device=dev)
    store[:, :P].copy_(torch.from_numpy(np.array(x)))
    return store[:, :P]


# ----------------------------------------------------------------- 1. clip_scales
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_clip_scales_bitwise(cuda, K):
    rng = np.random.RandomState(K)
    q = (rng.lognormal(0.0, 3.0, K)).astype(F32)
    for C in (1.0, 0.37, 12.5, 0.0, 1e-30, float("inf")):
        norms, c = kernels.clip_scales(torch.from_numpy(q).to(cuda), C)
        n_ref, c_ref = ref.clip_scales_ref(q, C)
        assert_bits(norms, n_ref, f"norms K={K} C={C}")
        assert_bits(c, c_ref, f"c K={K} C={C}")


def test_clip_scales_special_values(cuda):
    q = np.array([0.0, np.inf, np.nan, 0.25, 4.0, F32(1) + F32(2.0 ** -22), np.nextafter(F32(1), F32(2)),
                  1e-45, 3.0e38, 1e-30], dtype=F32)
    for C in (1.0, 0.0, 1e-30, float("inf")):
        norms, c = kernels.clip_scales(torch.from_numpy(q).to(cuda), C)
        n_ref, c_ref = ref.clip_scales_ref(q, C)
        assert_bits(norms, n_ref, f"norms C={C}")
        assert_bits(c, c_ref, f"c C={C}")
    _, c = kernels.clip_scales(torch.from_numpy(q).to(cuda), 1.0)
    c = c.cpu().numpy()
    assert c[0] == 1 and c[1] == 0 and np.isnan(c[2]) and c[3] == 1 and c[4] == 0.5 and c[5] < 1 and c[6] == 1


# ------------------------------------------------------------------ 2. dense fold
DENSE_K = [1, 2, 5, 8, 9, 33]


@pytest.mark.parametrize("P", [1, 3, 4, 1027, 8197, (1 << 20) + 3])
def test_dense_fold_bitwise(cuda, P):
    Ks = [9] if P > (1 << 20) else DENSE_K
    for K in Ks:
        x = deltas(K, P)
        c, w = factors(K)
        scale = F32(1.0 / float(w.astype(np.float64).sum()))
        # an aligned stride (16-byte units + tail) and an odd one (element units)
        strides = [(P + 3) // 4 * 4 + 4] + ([P + 1 + (P % 2)] if P <= 8197 else [])
        for ld in strides:
            xd = on_device(x, cuda, ld)
            assert xd.stride(0) == ld > P
            wd, cd = torch.from_numpy(np.array(w)).to(cuda), torch.from_numpy(np.array(c)).to(cuda)
            tag = f"K={K} P={P} ld={ld}"
            assert_bits(kernels.clipped_sum_dense(xd, wd, cd), ref.clipped_fold_ref(x, w, c, None), tag)
            assert_bits(kernels.clipped_sum_dense(xd, wd, cd, scale=float(scale)),
                        ref.clipped_fold_ref(x, w, c, scale), tag + " scale")
            assert_bits(kernels.clipped_sum_dense(xd, wd, cd, scale=float(scale), nontemporal=True),
                        ref.clipped_fold_ref(x, w, c, scale), tag + " nontemporal")
            init = deltas(1, P, seed=5)[0]
            out = torch.from_numpy(np.array(init)).to(cuda)
            got = kernels.clipped_sum_dense(xd, wd, cd, scale=float(scale), out=out, accumulate=True)
            assert got is out
            assert_bits(out, ref.clipped_fold_ref(x, w, c, scale, init=init), tag + " accumulate")


@pytest.mark.parametrize("P", [3, 1027, 8197])
def test_dense_fold_special_values(cuda, P):
    K = 9
    x = np.array(deltas(K, P))
    x[1, 0] = np.inf
    x[2, P // 2] = np.nan
    x[3, P - 1] = -np.inf
    x[5, 0] = 0.0
    c, w = (np.array(a) for a in factors(K))
    c[1], c[4], c[5], c[7] = 0.0, 1e-40, np.nan, 0.0  # inf * 0, a denormal factor, NaN
    xd = on_device(x, cuda, (P + 3) // 4 * 4 + 4)
    got = kernels.clipped_sum_dense(xd, torch.from_numpy(w).to(cuda), torch.from_numpy(c).to(cuda), scale=0.25)
    want = ref.clipped_fold_ref(x, w, c, F32(0.25))
    assert np.isnan(want).all()  # client 5's NaN factor reaches every element
    assert_bits(got, want)
    c[5] = 0.5
    got = kernels.clipped_sum_dense(xd, torch.from_numpy(w).to(cuda), torch.from_numpy(c).to(cuda), scale=0.25)
    want = ref.clipped_fold_ref(x, w, c, F32(0.25))
    assert np.isnan(want).sum() in (2, 3) and np.isfinite(want).sum() >= P - 3
    assert_bits(got, want)


# ---------------------------------------------------------- 3. fused clipped squares
@pytest.mark.parametrize("K,P", [(5, 1027), (33, 8197), (130, 70001)])
def test_fused_clipped_squares(cuda, K, P):
    x = deltas(K, P)
    c, w = factors(K)
    scale = F32(1.0 / float(w.astype(np.float64).sum()))
    xd = on_device(x, cuda, (P + 3) // 4 * 4 + 4)
    wd, cd = torch.from_numpy(np.array(w)).to(cuda), torch.from_numpy(np.array(c)).to(cuda)
    out, l2sq = kernels.clipped_sum_dense(xd, wd, cd, scale=float(scale), with_clipped_l2sq=True)
    assert_bits(out, ref.clipped_fold_ref(x, w, c, scale), "mean with fused squares")
    prod = ref.clipped_products(x, c).astype(np.float64)
    want = (prod * prod).sum(axis=1)
    got = l2sq.cpu().numpy().astype(np.float64)
    err = np.abs(got - want) / want
    print(f"fused clipped squares K={K} P={P}: max rel err {err.max():.3e}")
    assert (err <= NORM_RTOL).all(), err.max()
    # an infinite factor on a client: its squares are inf, not NaN from the masked lanes
    if K == 5:
        c2 = np.array(c)
        c2[2] = np.inf
        _, l2 = kernels.clipped_sum_dense(xd, wd, torch.from_numpy(c2).to(cuda), with_clipped_l2sq=True)
        l2 = l2.cpu().numpy()
        assert np.isinf(l2[2]) and np.isfinite(np.delete(l2, 2)).all()


# --------------------------------------------------------- shared checks of 4. and 5.
def check_clipped_mean(got, x, weights, C, what):
    """The assertions of the slab and pytree APIs on a ClippedMean ``got`` over deltas
    x [K, P] (flattened in leaf order). Returns the restated factors."""
    K = x.shape[0]
    norms = got.norms.cpu().numpy()
    assert norms.dtype == F32 and norms.shape == (K,)
    n64 = ref.f64_norms(x)
    assert (np.abs(norms - n64) <= NORM_RTOL * n64).all(), what
    c = ref.clip_factors_ref(norms, C)
    clipped = got.clipped.cpu().numpy()
    assert clipped.dtype == np.bool_ and (clipped == (c != 1)).all(), what
    assert clipped.any() and not clipped.all(), f"{what}: the case must clip some clients and not others"
    w32 = np.array([F32(v) for v in weights], dtype=F32)
    W = 0.0
    for v in weights:
        W += v
    scale = F32((1.0 / W) if W > 0.0 else 0.0)
    flat = torch.cat([t.reshape(-1) for t in pytree.leaves_of(got.mean)])
    assert_bits(flat, ref.clipped_fold_ref(x, w32, c, scale), what + " mean")
    cn = got.clipped_norms.cpu().numpy()
    assert (nbits(cn)[~clipped] == nbits(norms)[~clipped]).all(), what  # verbatim where nothing was clipped
    p64 = ref.f64_norms(ref.clipped_products(x, c))
    assert (np.abs(cn - p64)[clipped] <= NORM_RTOL * p64[clipped]).all(), what
    return c


def weight_sets(K, seed):
    rng = np.random.RandomState(seed)
    return {"int": [int(v) for v in rng.randint(1, 500, K)],
            "float": [float(v) for v in rng.uniform(0.5, 40.0, K)],
            "zero_total": [0] * K}


# ------------------------------------------------------------------- 4. slab API
@pytest.mark.parametrize("K,P", [(9, 1027), (33, 70001)])
def test_slab_clipped_mean(cuda, K, P):
    x = deltas(K, P, seed=2)
    template = {"a": np.zeros((), F32), "b": np.zeros(P - 11, F32), "c": np.zeros((2, 5), F32)}
    sl = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    assert sl.num_params == P
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    C = float(np.median(ref.f64_norms(x)))
    for name, weights in weight_sets(K, K).items():
        got = sl.clipped_mean(weights, C)
        assert isinstance(got, tu.ClippedMean)
        assert [tuple(t.shape) for t in pytree.leaves_of(got.mean)] == [(), (P - 11,), (2, 5)]
        check_clipped_mean(got, x, weights, C, f"slab K={K} P={P} {name}")
    out = torch.empty(P, dtype=torch.float32, device=cuda)
    got = sl.clipped_mean(weight_sets(K, K)["int"], C, out=out)
    assert pytree.leaves_of(got.mean)[1].data_ptr() == out.data_ptr() + 4
    assert_bits(sl.rows, x, "the slab is not written")


# ----------------------------------------------------------------- 5. pytree API
LEAF_SHAPES = [(), (1,), (3,), (64,), (13, 79), (70001,), (0,)]
LEAF_NAMES = ["a", "b", "c", "d", "e", "f", "g"]  # sorted: the flatten order
LEAF_P = sum(int(np.prod(s)) for s in LEAF_SHAPES)


def client_trees(x, dev):
    """Every client's row of x as a dict of separately allocated leaves; leaf "d" is a view
    at element offset 1 of a larger buffer (4-byte aligned only)."""
    trees = []
    for k in range(x.shape[0]):
        tree, o = {}, 0
        for name, s in zip(LEAF_NAMES, LEAF_SHAPES):
            n = int(np.prod(s))
            v = torch.from_numpy(np.array(x[k, o:o + n]))
            if name == "d":
                buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
                buf[1:1 + n].copy_(v)
                leaf = buf[1:1 + n]
                assert leaf.data_ptr() % 16 == 4
            else:
                leaf = v.to(dev).reshape(s)
            tree[name] = leaf
            o += n
        trees.append(tree)
    return trees


@pytest.mark.parametrize("K", [1, 3, 9, 33])
def test_tree_clipped_mean(cuda, K):
    x = deltas(K, LEAF_P, seed=3)
    trees = client_trees(x, cuda)
    n64 = ref.f64_norms(x)
    # K = 1: a norm just above the clip norm and nothing unclipped is not a case of the issue's
    # assertion (some clipped, some not): clip at 0.75 of the only norm and check it alone
    C = float(np.median(n64)) if K > 1 else 0.75 * float(n64[0])
    before = [[(t.clone(), t._version) for t in pytree.leaves_of(tr)] for tr in trees]
    for name, weights in weight_sets(K, 100 + K).items():
        got = tu.tree_clipped_mean(list(zip(trees, weights)), C)
        assert set(got.mean) == set(LEAF_NAMES)
        assert [tuple(got.mean[n].shape) for n in LEAF_NAMES] == LEAF_SHAPES
        if K > 1:
            check_clipped_mean(got, x, weights, C, f"pytree K={K} {name}")
        else:
            norms = got.norms.cpu().numpy()
            c = ref.clip_factors_ref(norms, C)
            assert c[0] < 1 and bool(got.clipped.cpu().numpy()[0])
            assert abs(norms[0] - n64[0]) <= NORM_RTOL * n64[0]
            W = float(weights[0])
            flat = torch.cat([t.reshape(-1) for t in pytree.leaves_of(got.mean)])
            assert_bits(flat, ref.clipped_fold_ref(x, [F32(weights[0])], c, F32(1.0 / W if W > 0 else 0.0)))
            p64 = ref.f64_norms(ref.clipped_products(x, c))
            assert abs(got.clipped_norms.cpu().numpy()[0] - p64[0]) <= NORM_RTOL * p64[0]
    for tr, saved in zip(trees, before):
        for t, (copy, version) in zip(pytree.leaves_of(tr), saved):
            assert t._version == version
            assert torch.equal(t.view(torch.int32), copy.view(torch.int32))


def test_tree_clipped_mean_nothing_clipped_and_generator(cuda):
    """A clip norm above every norm: every factor is 1, clipped_norms are the norms' bits, and
    the mean is tree_mean's. The pairs may be a one-shot iterable."""
    K = 5
    x = deltas(K, LEAF_P, seed=4)
    trees = client_trees(x, cuda)
    weights = weight_sets(K, 9)["int"]
    got = tu.tree_clipped_mean(((t, w) for t, w in zip(trees, weights)), 1e30)
    assert not got.clipped.cpu().numpy().any()
    assert torch.equal(got.norms.view(torch.int32), got.clipped_norms.view(torch.int32))
    mean = tu.tree_mean(list(zip(trees, weights)))
    for n in LEAF_NAMES:
        assert torch.equal(got.mean[n].view(torch.int32), mean[n].view(torch.int32)), n


# ------------------------------------------- 6. agreement with the per-client route
def test_agrees_with_per_client_clipping(cuda):
    K = 9
    x = deltas(K, LEAF_P, seed=3)
    trees = client_trees(x, cuda)
    weights = weight_sets(K, 109)["int"]
    C = float(np.median(ref.f64_norms(x)))
    got = tu.tree_clipped_mean(list(zip(trees, weights)), C)
    loop = tu.tree_mean([(tu.tree_clip_by_global_norm(t, C), w) for t, w in zip(trees, weights)])
    c = ref.clip_factors_ref(got.norms.cpu().numpy(), C).astype(np.float64)
    w = np.array(weights, dtype=np.float64)
    bound = 5e-6 * (np.abs(x.astype(np.float64)) * (c * w)[:, None]).sum(axis=0) / w.sum()
    a = torch.cat([got.mean[n].reshape(-1) for n in LEAF_NAMES]).cpu().numpy().astype(np.float64)
    b = torch.cat([loop[n].reshape(-1) for n in LEAF_NAMES]).cpu().numpy().astype(np.float64)
    assert (np.abs(a - b) <= bound).all(), float((np.abs(a - b) / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------ 7. aggregator
def test_clipped_mean_aggregator(cuda):
    K = 5
    x = deltas(K, LEAF_P, seed=6)
    trees = client_trees(x, cuda)
    weights = weight_sets(K, 11)["int"]
    C = float(np.median(ref.f64_norms(x)))
    agg = fedjax_amd.aggregators.clipped_mean_aggregator(C)
    state = agg.init()
    ids = [f"client{k}".encode() for k in range(K)]
    mean, state = agg.apply(zip(ids, trees, weights), state)
    want = tu.tree_clipped_mean(list(zip(trees, weights)), C)
    for n in LEAF_NAMES:
        assert torch.equal(mean[n].view(torch.int32), want.mean[n].view(torch.int32)), n
    assert list(state.norms) == ids and list(state.clipped_norms) == ids and list(state.clipped) == ids
    for k, cid in enumerate(ids):
        assert state.norms[cid].shape == () and state.clipped[cid].dtype == torch.bool
        assert torch.equal(state.norms[cid], want.norms[k])
        assert torch.equal(state.clipped_norms[cid], want.clipped_norms[k])
        assert torch.equal(state.clipped[cid], want.clipped[k])
    assert any(bool(v) for v in state.clipped.values()) and not all(bool(v) for v in state.clipped.values())


# -------------------------------------------------------------------- 8. refusals
def test_refusals(cuda):
    with pytest.raises(TypeError):
        slab_mod.ClientDeltaSlab({"a": np.zeros(8, F32)}, 3, dtype=torch.bfloat16, device=cuda).clipped_mean(
            [1, 2, 3], 1.0)
    mixed = [{"a": torch.ones(8, device=cuda), "b": torch.ones(8, dtype=torch.bfloat16, device=cuda)}
             for _ in range(3)]
    with pytest.raises(TypeError):
        tu.tree_clipped_mean([(t, 1) for t in mixed], 1.0)
    ints = [{"a": torch.ones(8, dtype=torch.int32, device=cuda)} for _ in range(3)]
    with pytest.raises(TypeError):
        tu.tree_clipped_mean([(t, 1) for t in ints], 1.0)
    with pytest.raises(TypeError):
        kernels.clipped_sum_dense(torch.ones(3, 8, dtype=torch.bfloat16, device=cuda),
                                  torch.ones(3, device=cuda), torch.ones(3, device=cuda))
    # raw entry points: refused flags launch nothing (the sentinel output stays)
    K, P = 3, 64
    x = torch.ones(K, P, device=cuda)
    w, c = torch.ones(K, device=cuda), torch.full((K,), 0.5, device=cuda)
    out = torch.full((P,), -7.0, device=cuda)
    l2 = torch.full((K,), -7.0, device=cuda)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    image = torch.tensor([x[k].data_ptr() for k in range(K)] + [out.data_ptr(), P, 0, P // 4], dtype=torch.int64,
                         device=cuda)
    lib = _lib.load()
    stream = torch.cuda.current_stream(cuda).cuda_stream
    for fl in (_lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.ZEROED_WS | _lib.SCALE, 12 << 8):
        rc = lib.fjagg_wsum_clip_dense(_lib.F32, x.data_ptr(), P, K, P, w.data_ptr(), c.data_ptr(), 1.0,
                                       out.data_ptr(), l2.data_ptr(), fl, ws.data_ptr(), ws.numel(), stream)
        assert rc == -3, fl
        rc = lib.fjagg_wsum_clip_ptrs(_lib.F32, image.data_ptr(), 1, K, 1, w.data_ptr(), c.data_ptr(), 1.0,
                                      l2.data_ptr(), fl, ws.data_ptr(), ws.numel(), stream)
        assert rc == -3, fl
    rc = lib.fjagg_wsum_clip_dense(_lib.BF16, x.data_ptr(), P, K, P, w.data_ptr(), c.data_ptr(), 1.0,
                                   out.data_ptr(), l2.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream)
    assert rc == -3
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (l2 == -7.0).all()
    # the same image and buffers are a valid call without those flags
    _lib.call("fjagg_wsum_clip_ptrs", _lib.F32, image.data_ptr(), 1, K, 1, w.data_ptr(), c.data_ptr(), 1.0,
              l2.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream)
    assert (out == 1.5).all() and (l2 == 16.0).all()


# -------------------------------------------------------- 9. no host round trip
def test_no_host_synchronisation(cuda):
    K, P = 9, 1027
    x = deltas(K, P, seed=2)
    sl = slab_mod.ClientDeltaSlab({"a": np.zeros(P, F32)}, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    weights = weight_sets(K, K)["int"]
    C = float(np.median(ref.f64_norms(x)))
    sl.clipped_mean(weights, C)  # first call: library load, kernel attributes
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = sl.clipped_mean(weights, C)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_clipped_mean(got, x, weights, C, "under sync debug mode")
