"""Differentially private clipped mean on the GPU: the device standard normal
(fjcomp_normal / fjcomp_normal_from_bits) against the restatement in tests/normal_restated.py,
and the noise epilogue of the clipped folds (fjagg_wsum_clip_noise_dense / _ptrs and the Python
surface over them) against the composed route — clipped_mean, then random.normal per leaf, then a
float32 multiply and a float32 add in torch — bit for bit."""
import functools

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import pytree, random as fjr, slab as slab_mod, tree_util as tu
from oracle import jax_random_ref as jr
from tests import normal_restated as nr

pytestmark = pytest.mark.gpu
F32 = np.float32
KEY = jr.prng_key(20240613)
LEAF_SETS = [[1], [3, 5], [1023, 4097, 2], [4096, 4096], [6, 1, 0, 9]]
KS = [1, 2, 5, 64]
STDDEVS = [0.0, 1e-3, 2.5]


def nbits(t):
    """uint32 bit patterns of a float32 tensor / array with every NaN mapped to one pattern."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a, dtype=F32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b.reshape(-1)


def assert_same_bits(got, want, what):
    g, w = nbits(got), nbits(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


def assert_equal_raw(got, want, what):
    assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                       want.view(torch.int32) if want.dtype == torch.float32 else want), what


@functools.lru_cache(maxsize=None)
def deltas(K, P, seed=0):
    """Seeded CPU normal deltas, client k scaled by 2**((k % 5) - 2): float32 [K, P], read-only."""
    g = torch.Generator().manual_seed(977 * seed + 13 * K + P)
    x = torch.randn(K, P, generator=g, dtype=torch.float32)
    x *= torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], dtype=torch.float32)[:, None]
    return x


def weights_of(K):
    return [float(1 + (7 * k) % 11) for k in range(K)]


def template(sizes):
    return {f"l{i:02d}": np.zeros(n, F32) for i, n in enumerate(sizes)}


def make_slab(x, sizes, dev):
    s = slab_mod.ClientDeltaSlab(template(sizes), x.shape[0], device=dev)
    s.rows.copy_(x.to(dev))
    return s


def median_norm(x):
    return float(np.median(np.linalg.norm(x.numpy().astype(np.float64), axis=1)))


def composed(clean, stddev, key, sizes):
    """clipped mean leaves + f32(stddev) * normal(keys[l]): separate torch mul and add (no FMA)."""
    leaves, td = pytree.flatten(clean.mean)
    keys = fjr.split(key, len(sizes))
    sd = torch.tensor(F32(stddev), dtype=torch.float32, device=leaves[0].device)
    out = []
    for l, leaf in enumerate(leaves):
        z = fjr.normal(keys[l], tuple(leaf.shape), device=leaf.device)
        out.append(torch.add(leaf, torch.mul(z, sd)))
    return out


def check_result(got, clean, stddev, key, sizes, what):
    for l, (g, w) in enumerate(zip(pytree.leaves_of(got.mean), composed(clean, stddev, key, sizes))):
        assert g.shape == w.shape
        assert_same_bits(g, w, f"{what}: leaf {l}")
    assert_same_bits(got.norms, clean.norms, what + ": norms")
    assert_same_bits(got.clipped_norms, clean.clipped_norms, what + ": clipped_norms")
    assert torch.equal(got.clipped, clean.clipped), what + ": clipped"


# ------------------------------------------------------------------ 1. the device normal
def test_normal_from_bits_all_mantissas(cuda):
    """All 2^23 mantissa patterns (bits = m << 9): within 1 float32 ulp of the restated value.
    Derived, not measured: both sides evaluate sqrt(2) * erfinv(u) in float64 from the same u and
    round once, so they can differ only where the two float64 values straddle a rounding point."""
    m = np.arange(1 << 23, dtype=np.uint32)
    bits = m << np.uint32(9)
    want = nr.normal_from_bits(bits)
    got = fjr.normal_from_bits(torch.from_numpy(bits.view(np.int32)).to(cuda)).cpu().numpy()
    assert np.isfinite(got).all() and got.dtype == F32
    d = nr.ulp_distance(got, want)
    exact = float((d == 0).mean())
    print(f"normal_from_bits over 2^23 mantissas: {exact:.6%} exact, max {int(d.max())} ulp, "
          f"{int((d > 0).sum())} differ")
    assert d.max() <= 1
    # the low 9 bits of a word do not enter the draw
    lo = fjr.normal_from_bits(torch.from_numpy((bits[:4096] | np.uint32(0x1FF)).view(np.int32)).to(cuda))
    assert_same_bits(lo, got[:4096], "low bits ignored")


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 255, 256, 257, 65537])
def test_normal_is_bits_then_map(cuda, n):
    got = fjr.normal(KEY, (n,), device=cuda)
    assert got.shape == (n,) and got.dtype == torch.float32
    bits = fjr.random_bits(KEY, (n,), device=cuda)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), jr.random_bits(KEY, n))
    assert_same_bits(got, fjr.normal_from_bits(bits), f"n={n}")
    assert nr.ulp_distance(got.cpu().numpy(), nr.normal(KEY, (n,))).max(initial=0) <= 1


def test_normal_shapes(cuda):
    flat = fjr.normal(KEY, (35,), device=cuda)
    assert_same_bits(fjr.normal(KEY, (5, 7), device=cuda), flat, "2-d")
    assert fjr.normal(KEY, (5, 7), device=cuda).shape == (5, 7)
    assert_same_bits(fjr.normal(KEY, 35, device=cuda), flat, "int shape")
    assert fjr.normal(KEY, (), device=cuda).shape == ()
    assert_same_bits(fjr.normal(KEY, (), device=cuda), fjr.normal(KEY, (1,), device=cuda), "scalar")
    with pytest.raises(TypeError):
        fjr.normal_from_bits(flat)


def test_keys_same_and_different(cuda):
    a = fjr.normal(KEY, (4096,), device=cuda)
    assert_same_bits(fjr.normal(KEY, (4096,), device=cuda), a, "same key")
    b = fjr.normal(jr.prng_key(1), (4096,), device=cuda)
    assert float((a.view(torch.int32) != b.view(torch.int32)).float().mean()) > 0.99


# ------------------------------------------------------------------ 2. fused equals composed
@pytest.mark.parametrize("sizes", LEAF_SETS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("K", KS)
def test_fused_equals_composed_both_routes(cuda, K, sizes):
    P = sum(sizes)
    x = deltas(K, P)
    w = weights_of(K)
    C = median_norm(x)
    s = make_slab(x, sizes, cuda)
    clean_slab = s.clipped_mean(w, C)
    clients = [s.client(k) for k in range(K)]
    clean_tree = tu.tree_clipped_mean(list(zip(clients, w)), C)
    if K > 1:
        assert 0 < int(clean_slab.clipped.sum()) < K
    for stddev in STDDEVS:
        tag = f"K={K} sizes={sizes} stddev={stddev}"
        got_slab = s.dp_clipped_mean(w, C, stddev, KEY)
        check_result(got_slab, clean_slab, stddev, KEY, sizes, "slab " + tag)
        got_tree = tu.tree_dp_clipped_mean(list(zip(clients, w)), C, stddev, KEY)
        check_result(got_tree, clean_tree, stddev, KEY, sizes, "pytree " + tag)
        # the two routes agree bit for bit over the same deltas
        for l, (a, b) in enumerate(zip(pytree.leaves_of(got_slab.mean), pytree.leaves_of(got_tree.mean))):
            assert_same_bits(a, b, f"routes {tag}: leaf {l}")
    # the noise is there: another key gives other values
    other = s.dp_clipped_mean(w, C, 2.5, jr.prng_key(5))
    assert any(not torch.equal(a, b) for a, b in zip(pytree.leaves_of(other.mean), pytree.leaves_of(got_slab.mean)))


def test_misaligned_leaves_on_the_pytree_route(cuda):
    """Leaves that are views offset by one element (element units) beside aligned ones."""
    K, sizes = 5, [1023, 4097, 2]
    x = deltas(K, sum(sizes) + 3, seed=2)
    w = weights_of(K)
    store = x.to(cuda)
    clients = []
    for k in range(K):
        o, tree = 0, {}
        for i, n in enumerate(sizes):
            o += 1  # every leaf starts one element after the previous one's end: 4-byte aligned only
            tree[f"l{i:02d}"] = store[k, o:o + n]
            o += n
        clients.append(tree)
    assert any(t.data_ptr() % 16 for t in clients[0].values())
    C = float(np.median([float(torch.sqrt(sum((t.double() ** 2).sum() for t in c.values()))) for c in clients]))
    clean = tu.tree_clipped_mean(list(zip(clients, w)), C)
    for stddev in STDDEVS:
        got = tu.tree_dp_clipped_mean(list(zip(clients, w)), C, stddev, KEY)
        check_result(got, clean, stddev, KEY, sizes, f"misaligned stddev={stddev}")


def test_more_leaves_than_the_kernel_arguments_hold(cuda):
    """The pytree route reads a device table past FJAGG_NOISE_MAX_LEAVES; the slab route refuses."""
    K, sizes = 2, [3] * 70
    x = deltas(K, sum(sizes), seed=3)
    w = weights_of(K)
    s = make_slab(x, sizes, cuda)
    clients = [s.client(k) for k in range(K)]
    C = median_norm(x)
    clean = tu.tree_clipped_mean(list(zip(clients, w)), C)
    got = tu.tree_dp_clipped_mean(list(zip(clients, w)), C, 1e-3, KEY)
    check_result(got, clean, 1e-3, KEY, sizes, "70 leaves")
    with pytest.raises(ValueError, match="leaves"):
        s.dp_clipped_mean(w, C, 1e-3, KEY)


def test_many_workgroups_per_leaf(cuda):
    """64 x 1.2 M: several workgroups per leaf, the 8-unit walk, a tail and an odd leaf length."""
    K, sizes = 64, [700001, 500002]
    x = deltas(K, sum(sizes), seed=1)
    w = weights_of(K)
    C = median_norm(x)
    s = make_slab(x, sizes, cuda)
    clients = [s.client(k) for k in range(K)]
    clean = s.clipped_mean(w, C)
    got_slab = s.dp_clipped_mean(w, C, 1e-3, KEY)
    check_result(got_slab, clean, 1e-3, KEY, sizes, "slab 64 x 1.2M")
    got_tree = tu.tree_dp_clipped_mean(list(zip(clients, w)), C, 1e-3, KEY)
    check_result(got_tree, tu.tree_clipped_mean(list(zip(clients, w)), C), 1e-3, KEY, sizes, "pytree 64 x 1.2M")
    for a, b in zip(pytree.leaves_of(got_slab.mean), pytree.leaves_of(got_tree.mean)):
        assert_same_bits(a, b, "routes 64 x 1.2M")


def test_same_key_same_bits(cuda):
    K, sizes = 5, [3, 5]
    x = deltas(K, 8)
    s = make_slab(x, sizes, cuda)
    a = s.dp_clipped_mean(weights_of(K), 1.0, 2.5, KEY)
    b = s.dp_clipped_mean(weights_of(K), 1.0, 2.5, KEY)
    for u, v in zip(pytree.leaves_of(a.mean), pytree.leaves_of(b.mean)):
        assert_same_bits(u, v, "same key twice")


# ------------------------------------------------------------------ 3. padding, out, non-finite
def test_padding_and_out_are_untouched(cuda):
    K, sizes = 5, [3, 6]  # P = 9, row stride 12
    x = deltas(K, 9)
    w = weights_of(K)
    s = make_slab(x, sizes, cuda)
    assert s.row_stride == 12
    s.storage[:, 9:] = -7.0
    buf = torch.full((16,), -7.0, device=cuda)
    clean = s.clipped_mean(w, 1.0, out=buf[:9])
    assert_same_bits(buf[9:], np.full(7, -7.0, F32), "clipped_mean leaves out's tail alone")
    buf2 = torch.full((16,), -7.0, device=cuda)
    got = s.dp_clipped_mean(w, 1.0, 2.5, KEY, out=buf2[:9])
    assert_same_bits(buf2[9:], np.full(7, -7.0, F32), "beyond P of out")
    assert_same_bits(s.storage[:, 9:], np.full((K, 3), -7.0, F32), "row padding")
    assert pytree.leaves_of(got.mean)[0].data_ptr() == buf2.data_ptr()
    check_result(got, clean, 2.5, KEY, sizes, "with out")


def test_gaps_between_leaves_get_no_noise(cuda):
    """fjagg_wsum_clip_noise_dense with a leaf table that leaves gaps: those elements receive the
    clipped mean as fjagg_wsum_clip_dense writes it."""
    from fedjax_amd import kernels
    K, P = 5, 40
    x = deltas(K, P).to(cuda)
    w = torch.tensor(weights_of(K), device=cuda)
    c = torch.tensor([1.0, 0.5, 0.25, 1.0, 0.75], device=cuda)
    begins, sizes = [2, 9, 30], [5, 7, 10]  # gaps: [0,2) [7,9) [16,30); units straddle every edge
    keys = fjr.split(KEY, 3)
    clean = kernels.clipped_sum_dense(x, w, c, scale=0.125)
    got = kernels.dp_clipped_sum_dense(x, w, c, kernels.NoiseTable(2.5, begins, sizes, keys), scale=0.125)
    want = clean.clone()
    for b, n, k in zip(begins, sizes, keys):
        want[b:b + n] += fjr.normal(k, (n,), device=cuda) * torch.tensor(F32(2.5), device=cuda)
    assert_same_bits(got, want, "gaps")
    covered = torch.zeros(P, dtype=torch.bool, device=cuda)
    for b, n in zip(begins, sizes):
        covered[b:b + n] = True
    assert torch.equal(got[~covered], clean[~covered]) and not torch.equal(got[covered], clean[covered])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_deltas_match_the_composed_route(cuda, bad):
    K, sizes = 5, [1023, 4097, 2]
    x = deltas(K, sum(sizes)).clone()
    x[1, 7] = bad
    x[3, 2000] = bad
    w = weights_of(K)
    s = make_slab(x, sizes, cuda)
    clients = [s.client(k) for k in range(K)]
    clean = s.clipped_mean(w, 30.0)
    check_result(s.dp_clipped_mean(w, 30.0, 1e-3, KEY), clean, 1e-3, KEY, sizes, f"slab {bad}")
    check_result(tu.tree_dp_clipped_mean(list(zip(clients, w)), 30.0, 1e-3, KEY),
                 tu.tree_clipped_mean(list(zip(clients, w)), 30.0), 1e-3, KEY, sizes, f"pytree {bad}")


def test_empty_cases(cuda):
    s = make_slab(torch.zeros(3, 0), [0, 0], cuda)
    got = s.dp_clipped_mean([1.0, 2.0, 3.0], 1.0, 0.5, KEY)
    want = s.clipped_mean([1.0, 2.0, 3.0], 1.0)
    assert [t.numel() for t in pytree.leaves_of(got.mean)] == [0, 0]
    assert_same_bits(got.norms, want.norms, "empty norms")
    assert torch.equal(got.clipped, want.clipped)
    clients = [{"a": torch.zeros(0, device=cuda)} for _ in range(3)]
    got = tu.tree_dp_clipped_mean([(c, 1.0) for c in clients], 1.0, 0.5, KEY)
    want = tu.tree_clipped_mean([(c, 1.0) for c in clients], 1.0)
    assert pytree.leaves_of(got.mean)[0].numel() == 0
    assert_same_bits(got.norms, want.norms, "empty tree norms")
    got = tu.tree_dp_clipped_mean([({}, 1.0), ({}, 2.0)], 1.0, 0.5, KEY)
    assert got.mean == {} and got.norms.tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ 4. aggregator, capture
def test_aggregator_two_rounds(cuda):
    K, sizes = 5, [3, 5]
    x = deltas(K, 8)
    w = [1, 2, 5, 3, 4]
    s = make_slab(x, sizes, cuda)
    clients = [(f"c{k}".encode(), s.client(k), w[k]) for k in range(K)]
    max_norm, mult = median_norm(x), 1.1
    agg = fedjax_amd.aggregators.dp_clipped_mean_aggregator(max_norm, mult, fjr.PRNGSequence(42))
    state = agg.init()
    ref_seq = jr.PRNGSequence(jr.prng_key(42))
    stddev = float(F32(mult * max_norm * 5.0 / 15.0))
    clean = tu.tree_clipped_mean([(p, wt) for _, p, wt in clients], max_norm)
    noises = []
    for rnd in range(2):
        mean, state = agg.apply(clients, state)
        key = next(ref_seq)
        assert state.noise_stddev == stddev
        want = composed(clean, stddev, key, sizes)
        for l, (g, wv) in enumerate(zip(pytree.leaves_of(mean), want)):
            assert_same_bits(g, wv, f"round {rnd} leaf {l}")
        assert_same_bits(torch.stack([state.norms[c] for c, _, _ in clients]), clean.norms, "state norms")
        assert torch.equal(torch.stack([state.clipped[c] for c, _, _ in clients]), clean.clipped)
        noises.append(torch.cat([g - cl for g, cl in zip(pytree.leaves_of(mean), pytree.leaves_of(clean.mean))]))
    assert not torch.equal(noises[0], noises[1])


def test_capture_raises_and_records_nothing(cuda):
    K, sizes = 5, [1023, 4097, 2]
    x = deltas(K, sum(sizes))
    w = weights_of(K)
    s = make_slab(x, sizes, cuda)
    clients = [s.client(k) for k in range(K)]
    eager = s.dp_clipped_mean(w, 30.0, 1e-3, KEY)
    out = torch.full((sum(sizes),), -7.0, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    seen = []
    with torch.cuda.graph(graph):
        for call in (lambda: s.dp_clipped_mean(w, 30.0, 1e-3, KEY, out=out),
                     lambda: tu.tree_dp_clipped_mean(list(zip(clients, w)), 30.0, 1e-3, KEY),
                     lambda: fedjax_amd.aggregators.dp_clipped_mean_aggregator(30.0, 1.0, KEY).apply(
                         [(b"a", clients[0], 1.0)], None)):
            with pytest.raises(RuntimeError, match="privacy"):
                call()
            seen.append(True)
    assert len(seen) == 3
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(out, np.full(sum(sizes), -7.0, F32), "nothing was recorded")
    again = s.dp_clipped_mean(w, 30.0, 1e-3, KEY)
    for a, b in zip(pytree.leaves_of(again.mean), pytree.leaves_of(eager.mean)):
        assert_same_bits(a, b, "eager after the refused capture")
