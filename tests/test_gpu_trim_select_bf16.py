"""The trimmed mean and median of bfloat16 deltas by 16-bit rank selection on the GPU (method="select"):
bit for bit tests/robust_mean_ref.py and the float32 selection kernel on the same values upcast exactly."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import kernels, pytree, slab as slab_mod, tree_util as tu
from tests import robust_mean_ref as ref
from tests.trim_select_cases import trims

pytestmark = pytest.mark.gpu
C = 64  # the tile's columns (fjtrimsel16.hip kCols)


def bits16_of(rng, K, P):
    """bfloat16 bits by truncation: keeps the NaN, inf and zero patterns of both signs and makes many ties."""
    return (ref.mixed_data(rng, K, P).view(np.uint32) >> 16).astype(np.uint16)


def twin_of(bits16):
    return (bits16.astype(np.uint32) << 16).view(np.float32)


def fill(s, bits):
    """Raw bits into a slab's rows: uint16 into a bfloat16 slab, uint32 (of a float32 array) into a float32 one."""
    raw, np_raw = (torch.int16, np.int16) if s.dtype == torch.bfloat16 else (torch.int32, np.int32)
    s.rows.view(raw).copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np_raw)))
    return s


def slab_of(bits, dev, dtype, template=None):
    K, P = bits.shape
    return fill(slab_mod.ClientDeltaSlab(template or {"w": torch.zeros(P)}, K, dtype=dtype, device=dev), bits)


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def assert_canon(got, want, what):
    assert got.dtype == np.float32
    assert np.array_equal(ref.canon(got).reshape(-1), ref.canon(want).reshape(-1)), what


@pytest.mark.parametrize("K", [1, 2, 65, 129, 256, 257, 1000, 1024])
def test_bitwise_against_the_restatement_and_the_float32_kernel(cuda, K):
    rng = np.random.RandomState(1600 + K)
    for P in (1, 63, 65, 2 * C + 5):
        b = bits16_of(rng, K, P)
        x = twin_of(b)
        s, s32 = slab_of(b, cuda, torch.bfloat16), slab_of(x, cuda, torch.float32)
        for t in trims(K):
            got = flat_of(s.trimmed_mean(t, method="select"))
            assert_canon(got, ref.trimmed_mean(x, t), f"K={K} P={P} t={t}")
            want = flat_of(s32.trimmed_mean(t, method="select"))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (K, P, t)  # NaN payloads included
        if K in (256, 257):
            got = flat_of(s.median(method="select"))
            assert_canon(got, ref.median(x), f"K={K} P={P} median")
            assert np.array_equal(got.view(np.uint32), flat_of(s32.median(method="select")).view(np.uint32)), (K, P)
    got = kernels.trim_select_dense(s.rows, t, scale=float(ref.inverse(K - 2 * t)), nontemporal=True)
    assert_canon(got.cpu().numpy(), ref.trimmed_mean(x, t), f"K={K} t={t} nontemporal")


def test_pytree_route_is_the_slab_route(cuda):
    K, sizes = 257, (1, 65, 100, 4099)
    b = bits16_of(np.random.RandomState(5), K, sum(sizes))
    store = torch.zeros(K, 1 + sum(sizes), dtype=torch.bfloat16, device=cuda)
    store[:, 1:].view(torch.int16).copy_(torch.from_numpy(b.view(np.int16)))
    offs = np.concatenate([[1], 1 + np.cumsum(sizes)])
    clients = [{f"l{i}": store[k, offs[i]:offs[i + 1]] for i in range(len(sizes))} for k in range(K)]
    assert clients[0]["l1"].data_ptr() % 16 != 0
    s = slab_of(b, cuda, torch.bfloat16, {f"l{i}": torch.zeros(n) for i, n in enumerate(sizes)})
    want = flat_of(s.trimmed_mean(0.1, method="select"))
    assert_canon(want, ref.trimmed_mean(twin_of(b), kernels.trim_count(0.1, K, select=True)), "slab")
    got = tu.tree_trimmed_mean(clients, 0.1, method="select")
    assert all(x.dtype == torch.float32 for x in pytree.leaves_of(got))
    assert np.array_equal(flat_of(got).view(np.uint32), want.view(np.uint32))
    agg = fedjax_amd.aggregators.trimmed_mean_aggregator(0.1, method="select")
    got, _ = agg.apply([(k, c, 1.0 + k) for k, c in enumerate(clients)], agg.init())
    assert np.array_equal(flat_of(got).view(np.uint32), want.view(np.uint32))


def test_slab_capture_replays(cuda):
    K, P = 257, 2 * C + 5
    s = slab_of(bits16_of(np.random.RandomState(1), K, P), cuda, torch.bfloat16)
    out = torch.zeros(P, device=cuda)
    s.trimmed_mean(25, out=out, method="select")  # eager once: the kernel is loaded before the capture
    torch.cuda.synchronize()
    g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            res = s.trimmed_mean(25, out=out, method="select")
    for seed in (2, 3):
        b = bits16_of(np.random.RandomState(seed), K, P)
        fill(s, b)
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        eager = flat_of(s.trimmed_mean(25, method="select"))
        assert np.array_equal(flat_of(res).view(np.uint32), eager.view(np.uint32)), seed
        assert_canon(flat_of(res), ref.trimmed_mean(twin_of(b), 25), f"replay {seed}")
