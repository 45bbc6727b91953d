"""The top-k sparsified mean on the GPU against the numpy restatement of tests/topk_ref.py:
thresholds and sent counts bit for bit over every data family, the mean against the reference and
against ClientDeltaSlab.mean over the masked values, the tree route against the slab route, a
captured round replayed over rewritten deltas, and the aggregator's bit count.

Shapes: K in {1, 3, 17}; P in {1, 2, 255, 256, 257}, one below, at and above one histogram chunk
(kernels.TOPK_CHUNK) and one spanning several; keep counts {1, 2, P // 10, P - 1, P}. Means are
compared bit for bit with every NaN taken as one pattern (which NaN a sum of two NaNs returns is
the hardware's choice, not the contract's)."""
import numpy as np
import pytest
import torch

from fedjax_amd import aggregators, kernels, tree_util as tu
from fedjax_amd.slab import ClientDeltaSlab
from tests import topk_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
CH = kernels.TOPK_CHUNK
KS = (1, 3, 17)
PS = (1, 2, 255, 256, 257, CH - 1, CH, CH + 1, 3 * CH + 5)
SELECT_FAMILIES = ("gauss", "five", "zeros", "equal", "nan_inf", "subnormal", "signed_zero", "hot_bin", "last_digit")


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def ubits(a):
    a = np.ascontiguousarray(host(a))
    u = a.view(np.uint32).copy() if a.dtype != np.uint32 else a.copy()
    if a.dtype == np.float32:
        u[np.isnan(a)] = 0x7FC00000
    return u.ravel()


def assert_bits(got, want, what):
    g, w = ubits(got), ubits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:5].tolist(), [hex(v) for v in g[bad[:5]]], [hex(v) for v in w[bad[:5]]])


def assert_select(thr, sent, want, what):
    """Thresholds as raw bits (a threshold may itself be a NaN pattern: no canonicalisation) and sent."""
    g = np.ascontiguousarray(host(thr)).view(np.uint32)
    assert g.tolist() == want[0].tolist(), (what, "thresholds", [hex(v) for v in g], [hex(v) for v in want[0]])
    assert host(sent).dtype == np.int32 and host(sent).tolist() == want[1].tolist(), (what, "sent")


def weights_for(K):
    return ([3, -1.5, 0, 2.25, 1, 7, 0.5] * 3)[:K] if K > 1 else [2]


def slab_of(x, dev, sizes=None):
    K, P = x.shape
    s = ClientDeltaSlab([np.zeros(n, F32) for n in (sizes or [P])], K, device=dev)
    s.rows.copy_(torch.from_numpy(x))
    return s


# ------------------------------------------------------------------ 1. thresholds and sent
@pytest.mark.parametrize("name", SELECT_FAMILIES)
def test_thresholds_and_sent(cuda, name):
    rng = np.random.RandomState(11 + SELECT_FAMILIES.index(name))
    compared = 0
    for K in KS:
        for P in PS:
            x = ref.family(name, K, P, rng)
            s = slab_of(x, cuda)
            want = ref.select_many(list(x), ref.keep_counts(P))
            for c, w in want.items():
                thr, sent = s.topk_thresholds(c)
                assert_select(thr, sent, w, f"{name} K={K} P={P} c={c}")
                compared += 1
            assert_bits(s.rows, x, f"{name} K={K} P={P}: the slab was written")
    assert compared == sum(len(ref.keep_counts(P)) for P in PS) * len(KS)
    if name == "zeros":
        assert int(host(sent).sum()) == 0 and int(np.ascontiguousarray(host(thr)).view(np.uint32).sum()) == 0


def test_dense_select_on_an_unaligned_padded_slab(cuda):
    """Rows at an odd element offset with a stride that is no multiple of four: the element path."""
    rng = np.random.RandomState(5)
    K, P, ld = 3, CH + 7, CH + 10
    x = ref.family("five", K, P, rng)
    store = torch.full((1 + K * ld,), float("nan"), dtype=torch.float32, device=cuda)
    xd = store[1:].view(K, ld)[:, :P]
    xd.copy_(torch.from_numpy(x))
    for c, w in ref.select_many(list(x), ref.keep_counts(P)).items():
        thr, sent = kernels.topk_select_dense(xd, c)
        assert_select(thr, sent, w, f"unaligned c={c}")
    wv = torch.tensor([1.0, -2.0, 0.5], device=cuda)
    out, thr, sent = kernels.topk_mean_dense(xd, wv, P // 10, scale=0.25)
    mean, T, n = ref.topk_mean_rows(list(x), [1.0, -2.0, 0.5], P // 10)
    assert_select(thr, sent, (T, n), "unaligned mean")
    masked = [ref.mask_row(r, t) for r, t in zip(x, T)]
    s = masked[0] * F32(1.0)
    for m, wk in zip(masked[1:], (-2.0, 0.5)):
        s = (s + m * F32(wk)).astype(F32)
    assert_bits(out, (s * F32(0.25)).astype(F32), "unaligned mean")


# ------------------------------------------------------------------ 2. the mean
@pytest.mark.parametrize("name", ("gauss", "five", "signed_zero", "nan_inf", "subnormal"))
def test_mean_against_the_reference_and_the_exact_fold(cuda, name):
    rng = np.random.RandomState(23)
    for K in KS:
        for P in (2, 257, CH + 1, 3 * CH + 5):
            x = ref.family(name, K, P, rng)
            w = weights_for(K)
            s = slab_of(x, cuda)
            for c in ref.keep_counts(P):
                what = f"{name} K={K} P={P} c={c}"
                got = s.topk_mean(w, c)
                mean, T, sent = ref.topk_mean_rows(list(x), w, c)
                assert_select(got.thresholds, got.sent, (T, sent), what)
                assert_bits(got.mean[0], mean, what + ": mean")
                masked = slab_of(np.stack([ref.mask_row(r, t) for r, t in zip(x, T)]), cuda)
                assert_bits(got.mean[0], masked.mean(w)[0], what + ": slab.mean over the masked values")
            full = s.topk_mean(w, P)
            assert_bits(full.mean[0], s.mean(w)[0], f"{name} K={K} P={P}: c = P against slab.mean")
            frac = s.topk_mean(w, 1.0)
            assert_bits(frac.mean[0], full.mean[0], "fraction 1.0")
            assert_bits(s.rows, x, "the slab was written")


def test_mean_into_out_and_empty_template(cuda):
    rng = np.random.RandomState(2)
    x = ref.family("gauss", 3, 300, rng)
    s = slab_of(x, cuda)
    out = torch.full((300,), float("nan"), device=cuda)
    got = s.topk_mean([1, 2, 3], 30, out=out)
    assert got.mean[0].data_ptr() == out.data_ptr()
    assert_bits(out, ref.topk_mean_rows(list(x), [1, 2, 3], 30)[0], "out")
    empty = ClientDeltaSlab({"a": np.zeros(0, F32)}, 3, device=cuda)
    r = empty.topk_mean([1, 2, 3], 5)
    assert r.mean["a"].numel() == 0 and host(r.sent).tolist() == [0, 0, 0] and host(r.thresholds).tolist() == [0, 0, 0]
    t, n = empty.topk_thresholds(0.5)
    assert host(t).tolist() == [0, 0, 0] and host(n).tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 3. the tree route
def placed(a, dev, offset):
    """A device copy of the float32 array `a`, `offset` elements into a NaN-filled allocation."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    store = torch.full((offset + a.numel() + 3,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:offset + a.numel()].view(a.shape)
    view.copy_(a)
    return view


def tree_case(K, shapes, rng, name="gauss", loud=None):
    """K client dicts over `shapes` (name -> shape); `loud`: a leaf whose values dwarf all others."""
    trees = []
    for k in range(K):
        t = {}
        for n, shp in shapes.items():
            v = ref.family(name, 1, int(np.prod(shp)), rng)[0].reshape(shp)
            if n == loud:
                v = (np.abs(v) + F32(1.0)) * F32(1e6)
            t[n] = v
        trees.append(t)
    return trees


def run_tree_and_slab(trees, w, c, dev, offsets=(0, 0), what=""):
    K = len(trees)
    names = sorted(trees[0])
    dev_trees = [{n: placed(t[n], dev, offsets[(k + i) % len(offsets)]) for i, n in enumerate(names)}
                 for k, t in enumerate(trees)]
    a = tu.tree_topk_mean(list(zip(dev_trees, w)), c)
    s = ClientDeltaSlab(trees[0], K, device=dev)
    for k, t in enumerate(trees):
        s.set_client(k, t)
    b = s.topk_mean(w, c)
    P = sum(int(np.prod(trees[0][n].shape)) for n in names)
    mean, T, sent = ref.topk_mean_trees(trees, w, kernels.topk_count(c, P))
    assert_select(a.thresholds, a.sent, (T, sent), what + " tree")
    assert_select(b.thresholds, b.sent, (T, sent), what + " slab")
    for n in names:
        assert tuple(a.mean[n].shape) == tuple(trees[0][n].shape)
        assert_bits(a.mean[n], mean[n], what + f" tree leaf {n}")
        assert_bits(a.mean[n], b.mean[n], what + f" tree against slab, leaf {n}")
    for k in (0, K - 1):
        for n in names:
            assert_bits(dev_trees[k][n], trees[k][n], what + ": a client leaf was written")
    return a, s


def test_tree_route_equals_the_slab_route(cuda):
    rng = np.random.RandomState(7)
    shapes = {"a": (3, 5), "b": (1,), "c": (CH + 3,), "d": (7, 11), "e": (257,)}
    P = sum(int(np.prod(s)) for s in shapes.values())
    for K in (1, 3, 17):
        w = weights_for(K)
        trees = tree_case(K, shapes, rng)
        for c in (1, P // 10, P - 1, P):
            _, s = run_tree_and_slab(trees, w, c, cuda, what=f"K={K} c={c}")
        assert s.row_stride > s.num_params  # rows with a padded stride
        run_tree_and_slab(trees, w, 0.05, cuda, offsets=(1, 0, 2), what=f"K={K} unaligned leaves")


def test_one_leaf_takes_every_slot(cuda):
    rng = np.random.RandomState(8)
    shapes = {"quiet": (33,), "loud": (41,), "one": (1,)}
    trees = tree_case(3, shapes, rng, loud="loud")
    a, _ = run_tree_and_slab(trees, [1, 2, 3], 41, cuda, what="loud leaf")
    assert not host(a.mean["quiet"]).any() and not host(a.mean["one"]).any()  # masked entirely: +0 terms only
    assert host(a.mean["loud"]).all() and host(a.sent).tolist() == [41, 41, 41]


def test_tree_route_refuses(cuda):
    x = torch.zeros(4, device=cuda)
    with pytest.raises(TypeError, match="float32 leaves"):
        tu.tree_topk_mean([({"a": x.to(torch.bfloat16)}, 1)], 1)
    with pytest.raises(TypeError, match="float32 leaves"):
        tu.tree_topk_mean([({"a": x.to(torch.int32)}, 1)], 1)
    with pytest.raises(ValueError, match="1 <= k <= P = 4"):
        tu.tree_topk_mean([({"a": x}, 1)], 5)
    with pytest.raises(TypeError):
        tu.tree_topk_mean([({"a": x}, 1)], True)
    with pytest.raises(ValueError, match="K <= 4096"):
        tu.tree_topk_mean([({"a": x}, 1)] * 4097, 1)


# ------------------------------------------------------------------ 4. capture
def test_capture_and_replay(cuda):
    rng = np.random.RandomState(9)
    K, P = 5, CH + 9
    w = weights_for(K)
    s = slab_of(ref.family("gauss", K, P, rng), cuda)
    out = torch.empty(P, device=cuda)
    s.topk_mean(w, 0.1, out=out)  # the eager call: the weights are on the device
    torch.cuda.synchronize()
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            res = s.topk_mean(w, 0.1, out=out)
            thr_only = s.topk_thresholds(0.1)
    c = kernels.topk_count(0.1, P)
    for name in ("five", "signed_zero"):
        x2 = ref.family(name, K, P, rng)
        s.rows.copy_(torch.from_numpy(x2))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        mean, T, sent = ref.topk_mean_rows(list(x2), w, c)
        assert_select(res.thresholds, res.sent, (T, sent), f"replay {name}")
        assert_select(thr_only[0], thr_only[1], (T, sent), f"replay {name}, select alone")
        assert_bits(out, mean, f"replay {name}: mean")
    fresh = slab_of(ref.family("gauss", K, P, rng), cuda)
    torch.cuda.synchronize()
    g1, st1 = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st1):  # a first call under capture would upload the weights: refused
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g1, stream=st1):
                fresh.topk_mean(w, 0.1)
    torch.cuda.synchronize()
    assert_bits(fresh.topk_mean(w, 3).mean[0], ref.topk_mean_rows(list(host(fresh.rows)), w, 3)[0], "eager afterwards")


# ------------------------------------------------------------------ 5. the aggregator
def test_aggregator_two_rounds_and_an_empty_one(cuda):
    rng = np.random.RandomState(10)
    shapes = {"w": (20, 13), "b": (13,)}
    P = 273
    agg = aggregators.top_k_sparsifier(0.1)
    state = agg.init()
    assert state.num_bits == 0.0
    sent_rounds = []
    for rnd, name in enumerate(("gauss", "five")):
        trees = tree_case(4, shapes, rng, name=name)
        w = [5, 1, 3, 2]
        clients = [(f"c{k}", {n: torch.from_numpy(v).to(cuda) for n, v in t.items()}, wk)
                   for k, (t, wk) in enumerate(zip(trees, w))]
        mean, state = agg.apply(clients, state)
        want, _, sent = ref.topk_mean_trees(trees, w, kernels.topk_count(0.1, P))
        sent_rounds.append(sent)
        for n in shapes:
            assert_bits(mean[n], want[n], f"round {rnd} leaf {n}")
        assert isinstance(state.num_bits, torch.Tensor) and state.num_bits.dtype == torch.float64
        assert state.num_bits.dim() == 0 and state.num_bits.is_cuda
        assert float(state.num_bits) == ref.num_bits(sent_rounds, P)
    assert ref.num_bits([[27], [27]], P) == 2 * 27 * (32 + 9)
    mean, after = agg.apply([], state)
    assert mean is None and float(after.num_bits) == float(state.num_bits)


# ------------------------------------------------------------------ 6. seeded fuzz
SIZES = (1, 2, 3, 4, 5, 63, 64, 255, 256, 257, 1023, 1024, 1025, CH - 1, CH, CH + 1, 2 * CH + 3)
FUZZ_CASES, FUZZ_GROUPS = 100, 4


def fuzz_case(seed, dev):
    rng = np.random.RandomState(1000 + seed)
    K = int(rng.choice([1, 2, 3, 5, 8, 17, 20]))
    L = int(rng.randint(1, 6))
    sizes = [int(rng.choice(SIZES[:13] if rng.rand() < 0.8 else SIZES)) for _ in range(L)]
    shapes = {f"l{i}": (n,) for i, n in enumerate(sizes)}
    P = sum(sizes)
    name = ref.FAMILIES[int(rng.randint(len(ref.FAMILIES)))]
    trees = tree_case(K, shapes, rng, name=name)
    if rng.rand() < 0.3:  # one client of another family
        trees[int(rng.randint(K))] = tree_case(1, shapes, rng, name="nan_inf" if P > 1 else "zeros")[0]
    w = [float(F32(v)) for v in rng.choice([0.0, 1.0, -1.0, 2.5, 0.125, 100.0], K)]
    if not any(w):
        w[0] = 1.0
    cs = ref.keep_counts(P) + [int(rng.randint(1, P + 1))]
    c = cs[int(rng.randint(len(cs)))]
    offsets = (0, 0) if rng.rand() < 0.5 else (1, 0, 3)
    run_tree_and_slab(trees, w, c, dev, offsets=offsets, what=f"fuzz {seed} {name} K={K} sizes={sizes} c={c}")


@pytest.mark.parametrize("group", range(FUZZ_GROUPS))
def test_fuzz(cuda, group):
    per = FUZZ_CASES // FUZZ_GROUPS
    compared = 0
    for seed in range(group * per, (group + 1) * per):
        fuzz_case(seed, cuda)
        compared += 1
    assert compared == per
