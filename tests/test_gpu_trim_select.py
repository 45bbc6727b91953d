"""The trimmed mean and median by rank selection on the GPU (method="select") against
tests/robust_mean_ref.py, bit for bit with every NaN mapped to one pattern, and the sorting kernels' raw bits."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import kernels, pytree, slab as slab_mod, tree_util as tu
from tests import robust_mean_ref as ref
from tests.trim_select_cases import families, trims

pytestmark = pytest.mark.gpu
C = 32  # the tile's columns (fjtrimsel.hip kCols)


def slab_of(x, dev, template=None):
    s = slab_mod.ClientDeltaSlab(template or {"w": torch.zeros(x.shape[1])}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return s


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def assert_bits(got, want, what):
    assert np.array_equal(ref.canon(got).reshape(-1), ref.canon(want).reshape(-1)), what


@pytest.mark.parametrize("K", [1, 2, 129, 255, 256, 257, 1000, 1024])
def test_bitwise_against_the_restatement(cuda, K):
    rng = np.random.RandomState(K)
    inputs = {f"mixed P={P}": ref.mixed_data(rng, K, P) for P in (1, 31, 33, 2 * C + 5)}
    if K in (257, 1024):
        inputs.update(families(K, 2 * C + 5))
    for name, x in inputs.items():
        s = slab_of(x, cuda)
        for t in trims(K):
            assert_bits(flat_of(s.trimmed_mean(t, method="select")), ref.trimmed_mean(x, t), f"K={K} {name} t={t}")
        if K in (256, 257):
            assert_bits(flat_of(s.median(method="select")), ref.median(x), f"K={K} {name} median")
        got = kernels.trim_select_dense(s.rows, t, scale=float(ref.inverse(K - 2 * t)), nontemporal=True)
        assert_bits(got.cpu().numpy(), ref.trimmed_mean(x, t), f"K={K} {name} t={t} nontemporal")


@pytest.mark.parametrize("K", [1, 16, 17, 100, 128])
def test_same_bits_as_the_sort_path(cuda, K):
    s = slab_of(ref.mixed_data(np.random.RandomState(40 + K), K, 2 * C + 5), cuda)
    for t in trims(K):
        a, b = flat_of(s.trimmed_mean(t, method="select")), flat_of(s.trimmed_mean(t, method="sort"))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (K, t)  # NaN payloads included
        a, b = kernels.trim_select_dense(s.rows, t, nontemporal=True), kernels.trim_dense(s.rows, t)  # no scale
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (K, t)


def test_pytree_route_is_the_slab_route(cuda):
    K, sizes = 257, (1, 33, 100, 4099)
    x = ref.mixed_data(np.random.RandomState(5), K, sum(sizes))
    store = torch.zeros(K, 1 + sum(sizes), device=cuda)
    store[:, 1:].copy_(torch.from_numpy(x))
    offs = np.concatenate([[1], 1 + np.cumsum(sizes)])
    clients = [{f"l{i}": store[k, offs[i]:offs[i + 1]] for i in range(len(sizes))} for k in range(K)]
    assert clients[0]["l1"].data_ptr() % 16 != 0
    s = slab_of(x, cuda, {f"l{i}": torch.zeros(n) for i, n in enumerate(sizes)})
    want = flat_of(s.trimmed_mean(0.1, method="select")).view(np.uint32)
    assert_bits(want.view(np.float32), ref.trimmed_mean(x, kernels.trim_count(0.1, K, select=True)), "slab")
    assert np.array_equal(flat_of(tu.tree_trimmed_mean(clients, 0.1, method="select")).view(np.uint32), want)
    agg = fedjax_amd.aggregators.trimmed_mean_aggregator(0.1, method="select")
    got, _ = agg.apply([(k, c, 1.0 + k) for k, c in enumerate(clients)], agg.init())
    assert np.array_equal(flat_of(got).view(np.uint32), want)


def test_slab_capture_replays(cuda):
    K, P = 257, 2 * C + 5
    s = slab_of(ref.mixed_data(np.random.RandomState(1), K, P), cuda)
    out = torch.zeros(P, device=cuda)
    s.trimmed_mean(25, out=out, method="select")  # eager once: the kernel is loaded before the capture
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = s.trimmed_mean(25, out=out, method="select")
    for seed in (2, 3):
        x = ref.mixed_data(np.random.RandomState(seed), K, P)
        s.rows.copy_(torch.from_numpy(x))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        eager = flat_of(s.trimmed_mean(25, method="select"))
        assert np.array_equal(flat_of(res).view(np.uint32), eager.view(np.uint32)), seed
        assert_bits(flat_of(res), ref.trimmed_mean(x, 25), f"replay {seed}")
