"""Top-k's transmitted form: the mean folded from sorted (index, value) lists against
a numpy restatement, the encoder against np.flatnonzero, the encode -> fold round trip against
top_k_sparsifier, and SparseSlab against ClientDeltaSlab.topk_mean. Bar: bit for bit on int32 views
(Gaussian values and positive weights: no coordinate's terms are all zeros)."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import kernels
from fedjax_amd.aggregators import compression as comp

pytestmark = pytest.mark.gpu
F32 = np.float32
TW, TG = kernels.SPARSE_WAVE_TILE, kernels.SPARSE_GROUP_TILE


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).reshape(-1).view(np.int32)


def make_lists(shape, K, P, rs):
    last = (P - 1) // TW * TW  # the first coordinate of the last wave tile
    pick = lambda lo, n: np.sort(rs.choice(np.arange(lo, P), size=n, replace=False))
    idx = {"one": lambda k: np.array([k * 7919 % P]),
           "all": lambda k: np.arange(P),
           "same": lambda k: np.array([P // 2]),
           "mix": lambda k: pick(0, 0 if k % 3 == 1 else rs.randint(1, min(P, 40) + 1)),
           "last": lambda k: pick(last, rs.randint(1, min(P - last, 40) + 1))}[shape]
    return [(i.astype(np.int32), rs.normal(size=i.size).astype(F32)) for i in map(idx, range(K))]


def numpy_fold(lists, P, w, scale):
    s = np.zeros(P, F32)
    for (i, v), wk in zip(lists, w):
        keep = (i >= 0) & (i < P)
        t = np.zeros(P, F32)
        t[i[keep]] = v[keep] * wk
        s = s + t
    return s * F32(scale)


def gpu_fold(lists, P, w, scale, cuda):
    n = np.array([i.size for i, _ in lists], np.int64)
    off = np.concatenate([[0], np.cumsum(n)])[:-1]
    idx = torch.from_numpy(np.concatenate([i for i, _ in lists] + [np.zeros(1, np.int32)])).to(cuda)
    val = torch.from_numpy(np.concatenate([v for _, v in lists] + [np.zeros(1, F32)])).to(cuda)
    tables = kernels.SparseTables(idx.data_ptr() + 4 * off, val.data_ptr() + 4 * off, n, P, w).upload(cuda)
    out = torch.full((P,), np.nan, dtype=torch.float32, device=cuda)
    return kernels.sparse_fold(tables, scale=scale, out=out)


@pytest.mark.parametrize("shape", ["one", "all", "same", "mix", "last"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("P", [1, TW - 1, TW, TW + 1, TG + 1, 3 * TG + 5])
def test_fold_equals_numpy(P, K, shape, cuda):
    rs = np.random.RandomState(P * 131 + K)
    lists = make_lists(shape, K, P, rs)
    w = rs.uniform(0.5, 2.0, K).astype(F32)
    scale = F32(1.0 / w.sum(dtype=np.float64))
    assert np.array_equal(bits(gpu_fold(lists, P, w, scale, cuda)), bits(numpy_fold(lists, P, w, scale)))


def test_fold_ignores_indices_outside_the_row(cuda):
    P, K = TG + 1, 65
    rs = np.random.RandomState(7)
    lists = make_lists("mix", K, P, rs)
    stray = [(np.concatenate([[-1], i, [P]]).astype(np.int32), np.concatenate([[F32(3)], v, [F32(5)]])) for i, v in lists]
    w = rs.uniform(0.5, 2.0, K).astype(F32)
    assert np.array_equal(bits(gpu_fold(stray, P, w, 0.25, cuda)), bits(numpy_fold(lists, P, w, 0.25)))


def expected_lists(flat, c):
    key = flat.view(np.uint32) & np.uint32(0x7FFFFFFF)
    T = max(int(np.sort(key)[-c]), 1)
    idx = np.flatnonzero(key >= T)
    return idx.astype(np.int32), flat[idx]


ENCODER_CASES = [((16383,), "gauss", 0.1), ((16384,), "gauss", 0.1), ((16385,), "gauss", 0.1),
                 ((5, 16390, 33), "gauss", 0.05), ((5, 16390, 33), "ties", 0.3), ((5, 16390, 33), "nan", 0.01),
                 ((5, 16390, 33), "zero", 0.5), ((16385,), "gauss", 1), ((5, 16390, 33), "gauss", 16428)]


@pytest.mark.parametrize("sizes,kind,k", ENCODER_CASES)
def test_encoder_equals_flatnonzero(sizes, kind, k, cuda):
    rs = np.random.RandomState(sum(sizes))
    P = sum(sizes)
    flat = {"gauss": lambda: rs.normal(size=P), "ties": lambda: rs.randint(-3, 4, P),
            "nan": lambda: rs.normal(size=P), "zero": lambda: np.zeros(P)}[kind]().astype(F32)
    if kind == "nan":
        flat[sizes[0] + 7] = np.nan
    leaves = np.split(flat, np.cumsum(sizes)[:-1])
    got = comp.topk_encode_pytree({f"l{i}": torch.from_numpy(x).to(cuda) for i, x in enumerate(leaves)}, k)
    want_idx, want_val = expected_lists(flat, kernels.topk_count(k, P))
    assert got.shapes == tuple((n,) for n in sizes) and got.indices.dtype == torch.int32
    assert np.array_equal(got.indices.cpu().numpy(), want_idx)
    assert np.array_equal(bits(got.values), bits(want_val))
    if kind == "zero":
        assert got.indices.numel() == 0


@pytest.mark.parametrize("K", [5, 70])
def test_round_trip_equals_top_k_sparsifier(K, cuda):
    rs = np.random.RandomState(K)
    shapes = {"a": (33,), "b": (70, 61), "c": (4099,)}
    deltas = [{n: torch.from_numpy(rs.normal(size=s).astype(F32)).to(cuda) for n, s in shapes.items()} for _ in range(K)]
    weights = [float(x) for x in rs.uniform(0.5, 2.0, K)]
    dense = comp.top_k_sparsifier(0.05)
    want, want_state = dense.apply([(k, d, w) for k, (d, w) in enumerate(zip(deltas, weights))], dense.init())
    sparse = comp.sparse_mean_aggregator(template=deltas[0])
    sent = [(k, comp.topk_encode_pytree(d, 0.05), w) for k, (d, w) in enumerate(zip(deltas, weights))]
    got, got_state = sparse.apply(sent, sparse.init())
    for n in shapes:
        assert got[n].shape == want[n].shape and np.array_equal(bits(got[n]), bits(want[n])), n
    assert float(got_state.num_bits) == float(want_state.num_bits) > 0


def test_sparse_slab_equals_topk_mean_and_replays(cuda):
    K, k = 9, 0.03
    template = {"a": np.zeros(17, F32), "b": np.zeros((130, 129), F32), "c": np.zeros(5, F32)}
    slab = fedjax_amd.ClientDeltaSlab(template, K, device=cuda)
    g = torch.Generator(device=cuda).manual_seed(3)
    slab.rows.copy_(torch.randn(slab.rows.shape, generator=g, device=cuda))
    weights = [1.0 + 0.25 * i for i in range(K)]
    want = slab.topk_mean(weights, k)
    sparse = slab.topk_encode(k)
    out = torch.empty(slab.num_params, dtype=torch.float32, device=cuda)
    got = sparse.mean(weights, out)
    for n in template:
        assert np.array_equal(bits(got[n]), bits(want.mean[n])), n
    assert torch.equal(sparse.sent, want.sent) and sparse.nnz == int(want.sent.sum())
    for c in (0, K - 1):
        mine, ref = sparse.client(c), comp.topk_encode_pytree(slab.client(c), k)
        assert torch.equal(mine.indices, ref.indices) and torch.equal(mine.values, ref.values) and mine.shapes == ref.shapes
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sparse.mean(weights, out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(eager))
