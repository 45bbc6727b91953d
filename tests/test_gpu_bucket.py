"""Bucketing on the GPU (fjagg_trim_bucket_dense / fjagg_trim_bucket_ptrs and the Python surface
over them) against the numpy restatement in tests/bucket_ref.py, bit for bit with
every NaN mapped to one pattern; fedjax_amd.random.permutation; the bucketed aggregators; and
the bucketed Krum and geometric median against a float64 brute force."""
import functools

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, pytree, random as fj_random, robust, slab as slab_mod, tree_util as tu
from tests import bucket_ref as ref
from tests import robust_mean_ref as trim_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
PS = [1, 63, 64, 65, 257, 600]
P_ALL = sum(PS)


def assert_bits(got, want, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    g, w = trim_ref.canon(got).reshape(-1), trim_ref.canon(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


def scale_of(B, t):
    return float(F32(tu._inverse(B - 2 * t)))


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def data(K):
    """float32 [K, sum(PS)] mixed data, shared by the tests of one K and never written."""
    x = trim_ref.mixed_data(np.random.RandomState(31 * K + 1), K, P_ALL)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def wanted(K, s, table, t):
    """The restatement over all of data(K), once per (shape, table, t)."""
    perm = ref.tables(K, K + s)[table]
    want = ref.trimmed_mean(data(K), s, t, perm)
    want.setflags(write=False)
    return want


def device_table(K, s, table, dev):
    perm = ref.tables(K, K + s)[table]
    return None if perm is None else torch.from_numpy(perm).to(dev)


# ---------------------------------------------------------------------- 1. the dense entry, swept
@pytest.mark.parametrize("K,s", ref.GPU_SHAPES)
def test_dense_sweep_bitwise(cuda, K, s):
    B = ref.bucket_count(K, s)
    x = data(K)
    offs = np.concatenate([[0], np.cumsum(PS)])
    for i, P in enumerate(PS):
        cols = slice(offs[i], offs[i + 1])
        ld = P + (i % 3)  # rows need float32's alignment only
        store = torch.full((1 + K * ld,), float("nan"), dtype=torch.float32, device=cuda)
        xd = store[1:].view(K, ld)[:, :P]
        xd.copy_(torch.from_numpy(np.array(x[:, cols])))
        before = xd.clone()
        for table in ("identity", "shuffle", "reversal"):
            perm = device_table(K, s, table, cuda)
            for t in ref.trims(B):
                want = wanted(K, s, table, t)[cols]
                got = kernels.trim_bucket_dense(xd, s, t, perm=perm, scale=scale_of(B, t))
                assert_bits(got, want, f"K={K} s={s} P={P} {table} t={t}")
                got = kernels.trim_bucket_dense(xd, s, t, perm=perm, scale=scale_of(B, t), nontemporal=True)
                assert_bits(got, want, f"nontemporal K={K} s={s} P={P} {table} t={t}")
        assert torch.equal(xd.view(torch.int32), before.view(torch.int32))  # the inputs are not written


def test_must_fail_without_the_feature(cuda):
    """slab.median(bucket_size=8) at K = 1024, the tree route at K = 130, and the C entry."""
    K, s = 1024, 8
    x = data(K)[:, :257]
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(257)}, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    assert_bits(sl.median(bucket_size=8)["w"], ref.median(x, 8), "slab median, 1024 clients in 128 buckets")
    x = data(130)[:, :70]
    clients = [{"a": torch.from_numpy(np.array(r[:7])).to(cuda), "b": torch.from_numpy(np.array(r[7:])).to(cuda)}
               for r in x]
    assert_bits(flat_of(tu.tree_median(clients, bucket_size=2)), ref.median(x, 2), "tree median, 130 clients")
    lib = _lib.load()
    xd = torch.from_numpy(np.array(data(5)[:, :64])).to(cuda)
    out = torch.empty(64, device=cuda)
    rc = lib.fjagg_trim_bucket_dense(_lib.F32, xd.data_ptr(), 64, 5, 64, None, 2, 1, 1.0, out.data_ptr(), _lib.SCALE,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert_bits(out, ref.trimmed_mean(data(5)[:, :64], 2, 1), "the C entry")


# ------------------------------------------------------------------- 2. slab and tree routes agree
def leaf_lists():
    """Distinct leaf lists of the trimmed mean's sweep, those with empty and odd leaves first."""
    seen, out = set(), []
    for _, _, leaves, _ in trim_ref.sweep_cases():
        if tuple(leaves) not in seen and 0 < sum(leaves) <= P_ALL:
            seen.add(tuple(leaves))
            out.append(leaves)
    out.sort(key=lambda l: (0 not in l, all(n % 4 == 0 for n in l)))
    return out


@pytest.mark.parametrize("i,shape", list(enumerate(ref.GPU_SHAPES)))
def test_tree_route_is_the_slab_route(cuda, i, shape):
    K, s = shape
    B = ref.bucket_count(K, s)
    leaves = leaf_lists()[i]
    offs = np.concatenate([[0], np.cumsum(leaves)])
    P = int(offs[-1])
    x = data(K)[:, :P]
    template = {f"l{j}": torch.zeros(n) for j, n in enumerate(leaves)}
    sl = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    rows = torch.from_numpy(np.array(x)).to(cuda)
    units = set()
    for views in (True, False):  # leaves as views at any element offset (unit 1), or own allocations (unit 4)
        clients = [{f"l{j}": (rows[k, offs[j]:offs[j + 1]] if views else rows[k, offs[j]:offs[j + 1]].clone())
                    for j in range(len(leaves))} for k in range(K)]
        units.add(all(c[f"l{j}"].data_ptr() % 16 == 0 for c in clients[:4] for j in range(len(leaves)) if leaves[j]))
        for table in ("identity", "shuffle", "reversal"):
            perm = ref.tables(K, K + s)[table]
            for t in ref.trims(B):
                want = wanted(K, s, table, t)[:P]
                tree = tu.tree_trimmed_mean(iter(clients), t, bucket_size=s, perm=perm)
                got_tree = torch.cat([tree[f"l{j}"].reshape(-1) for j in range(len(leaves))])
                assert_bits(got_tree, want, f"tree K={K} s={s} {table} t={t} leaves={leaves}")
                if views:
                    got_slab = sl.trimmed_mean(t, bucket_size=s, perm=perm)
                    got_slab = torch.cat([got_slab[f"l{j}"].reshape(-1) for j in range(len(leaves))])
                    assert_bits(got_slab, want, f"slab K={K} s={s} {table} t={t}")
                    assert torch.equal(got_slab.view(torch.int32), got_tree.view(torch.int32))
        med = tu.tree_median(clients, bucket_size=s)
        assert_bits(torch.cat([med[f"l{j}"].reshape(-1) for j in range(len(leaves))]),
                    wanted(K, s, "identity", (B - 1) // 2)[:P], "tree_median")
    assert True in units  # own allocations are 16-byte aligned: the plan's unit of 4 was taken
    assert torch.equal(sl.rows.cpu().view(torch.int32), torch.from_numpy(np.array(x)).view(torch.int32))  # not written


@pytest.mark.parametrize("K", [1, 5, 16, 17, 33, 65, 128])
def test_bucket_of_one_is_todays_entry(cuda, K):
    x = data(max(K, 5))[:K, :321]
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(321)}, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    for t in ref.trims(K):
        a, b = sl.trimmed_mean(t, bucket_size=1)["w"], sl.trimmed_mean(t)["w"]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (K, t)
    assert torch.equal(sl.median(bucket_size=1)["w"].view(torch.int32), sl.median()["w"].view(torch.int32))
    shuffle = np.random.RandomState(K).permutation(K)
    assert_bits(sl.trimmed_mean(0, bucket_size=1, perm=shuffle)["w"], trim_ref.trimmed_mean(x[shuffle], 0), "permuted")


def test_out_views_and_another_stream(cuda):
    K, s, P = 100, 3, 133
    x = data(K)[:, :P]
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(130), "b": torch.zeros(3)}, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    store = torch.full((P + 8,), -7.0, device=cuda)
    out = store[3:3 + P]
    got = sl.trimmed_mean(0.2, bucket_size=s, out=out)  # a fraction counts buckets: floor(0.2 * 34) = 6
    assert got["b"].data_ptr() == out.data_ptr()
    assert_bits(out, ref.trimmed_mean(x, s, 6), "out view")
    assert (store[:3] == -7).all() and (store[3 + P:] == -7).all()
    side = torch.cuda.Stream(cuda)
    perm_host = ref.tables(K, 5)["shuffle"]
    with torch.cuda.stream(side):
        s2 = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
        s2.rows.copy_(torch.from_numpy(np.array(x)), non_blocking=True)
        perm = torch.from_numpy(perm_host).to(cuda, non_blocking=True)
        got = s2.median(bucket_size=s, perm=perm)["w"]
    side.synchronize()
    assert_bits(got, ref.median(x, s, perm_host), "result and inputs on a side stream")
    e = slab_mod.ClientDeltaSlab({"w": torch.zeros(0)}, 300, device=cuda)
    assert e.median(bucket_size=4)["w"].numel() == 0


def test_refusals_launch_nothing(cuda):
    x = torch.zeros(129, 8, device=cuda)
    with pytest.raises(ValueError) as e:
        slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 129, device=cuda).median()
    assert str(e.value) == "the trimmed mean and median support K <= 128 clients, got K = 129"
    with pytest.raises(ValueError, match="128 buckets"):
        kernels.trim_bucket_dense(x, 1, 0)
    with pytest.raises(ValueError, match="different devices|perm"):
        kernels.trim_bucket_dense(x, 2, 0, perm=torch.zeros(128, dtype=torch.int32, device=cuda))
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.fjagg_trim_bucket_dense(_lib.F32, x.data_ptr(), 8, 129, 8, None, 1, 0, 1.0, x.data_ptr(), 0, st) == -3
    assert b"128 buckets" in lib.fjagg_last_error()
    assert lib.fjagg_trim_bucket_dense(_lib.F32, x.data_ptr(), 8, 129, 8, None, 2, 33, 1.0, x.data_ptr(), 0, st) == -1
    torch.cuda.synchronize()  # no pending HIP error, and a following valid call passes
    y = data(5)[:, :64]
    got = kernels.trim_bucket_dense(torch.from_numpy(np.array(y)).to(cuda), 2, 1, scale=1.0)
    assert_bits(got, ref.trimmed_mean(y, 2, 1), "after the refusals")


def test_stale_table_is_clamped(cuda):
    K, s, P = 9, 2, 65
    x = data(K)[:, :P]
    stale = np.array([-1, 9, 2**31 - 1, -2**31, 3, 0, 8, 100, 4], np.int32)
    store = torch.full((3 * K * P,), float("nan"), device=cuda)  # NaN around the slab: a stray read would show
    xd = store[K * P:2 * K * P].view(K, P)
    xd.copy_(torch.from_numpy(np.array(x)))
    got = kernels.trim_bucket_dense(xd, s, 0, perm=torch.from_numpy(stale).to(cuda), scale=scale_of(5, 0))
    clamped = np.array([ref.clamp(int(i), K) for i in stale])
    assert_bits(got, ref.trimmed_mean(x, s, 0, clamped), "clamped table")


# ------------------------------------------------------------------------------------ 3. capture
def test_capture_replays_over_rewritten_deltas_and_table(cuda):
    K, s, t, P = 130, 2, 5, 1029
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    x0 = trim_ref.mixed_data(np.random.RandomState(1), K, P)
    sl.rows.copy_(torch.from_numpy(x0))
    perm = torch.arange(K, dtype=torch.int32, device=cuda)
    out = torch.zeros(P, device=cuda)
    sl.trimmed_mean(t, bucket_size=s, perm=perm, out=out)  # eager once: the kernel is loaded before the capture
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = sl.trimmed_mean(t, bucket_size=s, perm=perm, out=out)
    for seed in (2, 3):
        x = trim_ref.mixed_data(np.random.RandomState(seed), K, P)
        table = np.random.RandomState(10 + seed).permutation(K).astype(np.int32)
        sl.rows.copy_(torch.from_numpy(x))
        perm.copy_(torch.from_numpy(table))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        replayed = res["w"].clone()
        eager = sl.trimmed_mean(t, bucket_size=s, perm=perm)["w"]
        assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32)), seed
        assert_bits(replayed, ref.trimmed_mean(x, s, t, table), f"replay {seed}")
    g1, st1 = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st1):
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g1, stream=st1):
                sl.trimmed_mean(t, bucket_size=s, perm=list(range(K)), out=out)  # a host table is an upload
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. the shuffle and the aggregators
@pytest.mark.parametrize("n", [1, 2, 129, 4096])
def test_permutation(cuda, n):
    key, other = fj_random.PRNGKey(n), fj_random.PRNGKey(n + 1)
    p = fj_random.permutation(key, n, device=cuda)
    assert p.dtype == torch.int32 and p.shape == (n,) and p.device == cuda
    host = p.cpu().numpy()
    assert np.array_equal(np.sort(host), np.arange(n))
    words = fj_random.random_bits(key, (n,), device=cuda).cpu().numpy().view(np.uint32)
    assert np.array_equal(host, np.argsort(words, kind="stable"))
    assert torch.equal(p, fj_random.permutation(key, n, device=cuda))
    if n > 2:
        assert not torch.equal(p, fj_random.permutation(other, n, device=cuda))


def test_aggregators_shuffle_with_a_fresh_key_each_round(cuda):
    K, s, P = 130, 2, 70
    x = data(K)[:, :P]
    clients = [{"a": torch.from_numpy(np.array(r[:7])).to(cuda), "b": torch.from_numpy(np.array(r[7:])).to(cuda)}
               for r in x]
    triples = [(f"c{k}", c, 1 + k % 3) for k, c in enumerate(clients)]
    key = fj_random.PRNGKey(77)
    first, second = fj_random.PRNGSequence(key).take(2)
    t1, t2 = fj_random.permutation(first, K, device=cuda), fj_random.permutation(second, K, device=cuda)
    assert not torch.equal(t1, t2)
    agg = fedjax_amd.aggregators.median_aggregator(bucket_size=s, rng=key)
    state = agg.init()
    got1, state = agg.apply(triples, state)
    got2, state = agg.apply(triples, state)
    for got, table in ((got1, t1), (got2, t2)):  # two rounds, two tables
        want = tu.tree_median(clients, bucket_size=s, perm=table)
        assert torch.equal(torch.from_numpy(flat_of(got)).view(torch.int32), torch.from_numpy(flat_of(want)).view(torch.int32))
        assert_bits(flat_of(got), ref.median(x, s, table.cpu().numpy()), "against the restatement")
    agg = fedjax_amd.aggregators.trimmed_mean_aggregator(0.1, bucket_size=s, rng=fj_random.PRNGSequence(key))
    got, _ = agg.apply(iter(triples), agg.init())
    assert_bits(flat_of(got), ref.trimmed_mean(x, s, 6, t1.cpu().numpy()), "trimmed mean, floor(0.1 * 65) buckets")
    agg = fedjax_amd.aggregators.median_aggregator(bucket_size=s)  # rng=None: consecutive clients
    assert_bits(flat_of(agg.apply(triples, agg.init())[0]), ref.median(x, s), "unshuffled")


# ------------------------------------------------------------- 5. Krum and the geometric median
def clustered(K, P, outliers, seed, nan_client=None):
    """Honest clients within 0.1 a coordinate of the origin; the outliers 100 a coordinate away, so a
    bucket mean holding one stays far more than 10 times the honest spread away at these sizes."""
    rng = np.random.RandomState(seed)
    x = (0.1 * rng.standard_normal((K, P))).astype(F32)
    for k in outliers:
        x[k] += F32(100.0)
    if nan_client is not None:
        x[nan_client] = np.nan
    return x


def brute_bucket_gram(x, s, perm):
    groups = robust.bucket_members(x.shape[0], s, perm)
    means = np.stack([x[g].astype(np.float64).mean(0) for g in groups])
    return means @ means.T, groups


def krum_weights(K, groups, selected, s):
    ids, w = np.full(K, -1, np.int64), [1] * K
    sizes = {len(groups[j]) for j in selected}
    for j in selected:
        ids[groups[j]] = 0
        if len(sizes) > 1:
            for k in groups[j]:
                w[int(k)] = min(sizes) if len(groups[j]) == s else s
    return w, ids


@pytest.mark.parametrize("perm_kind", ["identity", "shuffle"])
def test_bucketed_krum(cuda, perm_kind):
    K, s, P, f = 23, 3, 300, 1  # B = 8, the last bucket holds 2
    perm = ref.tables(K, 3)[perm_kind]
    x = clustered(K, P, outliers=[4], seed=12)
    template = {"w": torch.zeros(P - 5), "b": torch.zeros(5)}
    sl = slab_mod.ClientDeltaSlab(template, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(x))
    clients = [{k: v.clone() for k, v in sl.client(c).items()} for c in range(K)]
    Gb, groups = brute_bucket_gram(x, s, perm)
    for m in (1, 7):  # m = B - f selects every honest bucket, the short one among them
        want = robust.krum_select(Gb, f, m)
        got = sl.krum(f, m, bucket_size=s, perm=perm)
        assert isinstance(got, tu.BucketedKrumResult) and got.scores.shape == (8,)
        assert (got.selected.tolist() == want.tolist()) if m == 1 else (set(got.selected.tolist()) == set(want.tolist()))
        bad_bucket = [j for j, g in enumerate(groups) if 4 in g][0]
        assert bad_bucket not in got.selected
        assert [g.tolist() for g in got.members] == [groups[j].tolist() for j in got.selected]
        w, ids = krum_weights(K, groups, got.selected.tolist(), s)
        if m == 7 and bad_bucket != 7:
            assert 7 in got.selected and sorted(set(w)) == [1, 2, 3]  # the short bucket beside full ones
        assert perm_kind != "identity" or bad_bucket == 1
        want_mean = sl.grouped_mean(w, ids, 1)[0]
        assert torch.equal(torch.from_numpy(flat_of(got.mean)).view(torch.int32),
                           torch.from_numpy(flat_of(want_mean)).view(torch.int32))
        means = np.stack([x[groups[j]].astype(np.float64).mean(0) for j in got.selected]).mean(0)
        np.testing.assert_allclose(flat_of(got.mean), means, rtol=0, atol=1e-5)  # it IS the mean of the bucket means
        tree = tu.tree_krum(clients, f, m, bucket_size=s, perm=perm)
        assert tree.selected.tolist() == got.selected.tolist()
        assert np.array_equal(flat_of(tree.mean).view(np.uint32), flat_of(got.mean).view(np.uint32))


def test_bucketed_rules_never_load_a_nan_client(cuda):
    K, s, P, f = 23, 3, 200, 1
    x = clustered(K, P, outliers=[], seed=13, nan_client=10)  # bucket 3 of the identity table
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(x))
    got = sl.krum(f, 7, bucket_size=s)
    assert 3 not in got.selected and len(got.selected) == 7 and np.isinf(got.scores[3])
    assert torch.isfinite(got.mean["w"]).all()
    assert 10 not in np.concatenate(got.members)
    gm = sl.geometric_median(bucket_size=s)
    assert torch.isfinite(gm.median["w"]).all() and (gm.weights[9:12] == 0).all() and np.isinf(gm.distances[3])


def test_bucketed_geometric_median(cuda):
    K, s, P = 23, 3, 300
    perm = ref.tables(K, 4)["shuffle"]
    x = clustered(K, P, outliers=[4, 17], seed=14)
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    sl.rows.copy_(torch.from_numpy(x))
    got = sl.geometric_median(bucket_size=s, perm=perm, iterations=4)
    groups = robust.bucket_members(K, s, perm)
    a, d = robust.weiszfeld_weights(robust.bucket_gram(got.gram.cpu().numpy(), s, perm), None, 1e-6, 4)
    w32 = np.zeros(K, F32)
    for j, g in enumerate(groups):
        w32[g] = F32(a[j] / len(g))
    assert got.weights.tobytes() == w32.tobytes() and got.distances.shape == (8,)
    want = sl.grouped_mean(w32, np.zeros(K, np.int64), 1)[0]["w"]
    assert torch.equal(got.median["w"].view(torch.int32), want.view(torch.int32))
    Gb, _ = brute_bucket_gram(x, s, perm)
    a64, _ = robust.weiszfeld_weights(Gb, None, 1e-6, 4)
    np.testing.assert_allclose(a, a64, rtol=1e-3)
    means = np.stack([x[g].astype(np.float64).mean(0) for g in groups])
    np.testing.assert_allclose(got.median["w"].cpu().numpy(), a64 @ means, rtol=0, atol=1e-3)
    clients = [{"w": sl.rows[k].clone()} for k in range(K)]
    tree = tu.tree_geometric_median(clients, bucket_size=s, perm=perm)
    np.testing.assert_allclose(tree.weights, got.weights, rtol=1e-4)
    with pytest.raises(ValueError, match="client weights"):
        sl.geometric_median([1.0] * K, bucket_size=s)
    with pytest.raises(ValueError, match="host-only"):
        sl.krum(1, bucket_size=s, select="device")
