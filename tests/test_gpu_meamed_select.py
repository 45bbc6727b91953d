"""The mean around the median and Bulyan's second stage by rank selection on the GPU (method="select")
against tests/around_median_ref.py, bit for bit with every NaN mapped to one pattern, and the sorting kernels' raw bits."""
import numpy as np
import pytest
import torch

from fedjax_amd import pytree, robust, slab as slab_mod, tree_util as tu
from tests import around_median_ref as ref
from tests import bulyan_ref

pytestmark = pytest.mark.gpu
P = 70  # two full tiles of 32 columns and one of 6


def slab_of(x, dev, leaves=None):
    leaves = [x.shape[1]] if leaves is None else leaves
    s = slab_mod.ClientDeltaSlab({f"l{j}": torch.zeros(n) for j, n in enumerate(leaves)}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return s


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def assert_bits(got, want, what):
    assert np.array_equal(ref.canon(got).reshape(-1), ref.canon(want).reshape(-1)), what


def keeps(K):
    return sorted({1, (K + 1) // 2, K} | ({K - 1} if K > 2 else set()))


@pytest.mark.parametrize("kind", ["ties", "specials", "poisoned"])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 128, 129, 257, 1024])
def test_slab_bits_are_the_restatement(cuda, K, kind):
    x = ref.DATA[kind](np.random.RandomState(7 * K + len(kind)), K, P)
    s = slab_of(x, cuda)
    for beta in keeps(K):
        got = flat_of(s.mean_around_median(beta, method="select"))
        assert_bits(got, ref.mean_around_median(x, beta), f"K={K} {kind} beta={beta}")
        if K <= 128:  # the sorting kernel's raw bits, NaN payloads included
            sort = flat_of(s.mean_around_median(beta, method="sort"))
            assert np.array_equal(got.view(np.uint32), sort.view(np.uint32)), f"K={K} {kind} beta={beta} sort"


@pytest.mark.parametrize("on_device", [False, True])
def test_row_table_reads_only_its_rows(cuda, on_device):
    K, M = 300, 150
    rng = np.random.RandomState(11)
    rows = np.sort(rng.choice(K, size=M, replace=False))
    x = np.full((K, P), np.nan, np.float32)
    x[rows] = ref.specials(rng, M, P)
    s = slab_of(x, cuda)
    table = torch.from_numpy(rows.astype(np.int32)).to(cuda) if on_device else rows.tolist()
    for beta in (1, 75, 149):
        got = flat_of(s.mean_around_median(beta, rows=table, method="select"))
        assert_bits(got, ref.mean_around_median(x[rows], beta), f"beta={beta}")


@pytest.mark.parametrize("K", [129, 1024])
def test_pytree_route_is_the_slab_route(cuda, K):
    sizes = (0, 1, 3, 65, 257)
    x = ref.specials(np.random.RandomState(K), K, sum(sizes))
    store = torch.zeros(K, 1 + sum(sizes), device=cuda)
    store[:, 1:].copy_(torch.from_numpy(x))
    offs = np.concatenate([[1], 1 + np.cumsum(sizes)])
    clients = [{f"l{i}": store[k, offs[i]:offs[i + 1]] for i in range(len(sizes))} for k in range(K)]
    assert clients[0]["l3"].data_ptr() % 8 == 4  # a view at an odd element offset
    s = slab_of(x, cuda, sizes)
    for beta in (1, K // 2, K):
        want = flat_of(s.mean_around_median(beta, method="select"))
        assert_bits(want, ref.mean_around_median(x, beta), f"slab beta={beta}")
        got = tu.tree_mean_around_median(clients, beta, method="select")
        assert [got[f"l{i}"].numel() for i in range(len(sizes))] == list(sizes)
        assert np.array_equal(flat_of(got).view(np.uint32), want.view(np.uint32)), f"tree beta={beta}"


def test_bulyan_past_128_selected(cuda):
    K, f, sizes = 200, 10, (3, 65, 2)
    x = bulyan_ref.small_ints(np.random.RandomState(5), K, sum(sizes))
    x64 = x.astype(np.float64)
    selected = robust.bulyan_select(x64 @ x64.T, f)  # small integers: this Gram is exact
    assert len(selected) == K - 2 * f == 180
    want = ref.mean_around_median(x[np.sort(selected)], 160)
    s = slab_of(x, cuda, sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    clients = [{f"l{i}": s.rows[k, offs[i]:offs[i + 1]] for i in range(len(sizes))} for k in range(K)]
    for got in (s.bulyan(f, method="select"), tu.tree_bulyan(clients, f, method="select")):
        assert got.selected.tolist() == selected.tolist() and got.keep == 160
        assert_bits(flat_of(got.mean), want, "mean")
    for call in (lambda: s.bulyan(f), lambda: tu.tree_bulyan(clients, f)):
        with pytest.raises(ValueError, match="K - 2f <= 128"):
            call()


def test_slab_capture_replays(cuda):
    K, beta = 257, 100
    s = slab_of(ref.specials(np.random.RandomState(1), K, P), cuda)
    out = torch.zeros(P, device=cuda)
    s.mean_around_median(beta, out=out, method="select")  # eager once: the kernel is loaded before the capture
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = s.mean_around_median(beta, out=out, method="select")
    for seed in (2, 3):
        x = ref.specials(np.random.RandomState(seed), K, P)
        s.rows.copy_(torch.from_numpy(x))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        eager = flat_of(s.mean_around_median(beta, method="select"))
        assert np.array_equal(flat_of(res).view(np.uint32), eager.view(np.uint32)), seed
        assert_bits(flat_of(res), ref.mean_around_median(x, beta), f"replay {seed}")
