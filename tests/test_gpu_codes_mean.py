"""The uniform quantizer's transmitted form: the mean folded straight from 8-bit
level codes against a numpy decode-and-fold, the encode -> fold round trip against the fused
uniform_stochastic_quantizer round, graph capture of CodeSlab.mean, and the refusals.

Bar: bit for bit on int32 views, with every NaN taken as one NaN (payload and sign of a NaN are
not part of the contract anywhere in the compression suite: numpy's 0 * inf is -NaN, the GPU's
+NaN)."""
import math

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _compress, random
from fedjax_amd.aggregators import compression as comp

pytestmark = pytest.mark.gpu
F32 = np.float32
LEVELS = [2, 3, 16, 255, 256]
SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097]


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F32).reshape(-1)
    return np.where(np.isnan(a), F32(np.nan), a).view(np.int32)


def decode_fold(codes, minmax, weights, num_levels):
    """codes[k][l] uint8 arrays, minmax [K, L, 2]: the sequential float32 fold of the decoded values."""
    lev = np.arange(num_levels, dtype=F32) / F32(num_levels - 1)
    inv = F32(1.0 / sum(weights))
    out = []
    with np.errstate(all="ignore"):
        for l in range(len(codes[0])):
            for k, w in enumerate(weights):
                vmin, vmax = minmax[k, l]
                val = vmin + lev[np.minimum(codes[k][l], num_levels - 1)] * F32(vmax - vmin)
                s = val * F32(w) if k == 0 else s + val * F32(w)
            out.append(s * inv)
    return out


@pytest.mark.parametrize("share", ["small", "large"])  # 4 or 16 codes a lane (chosen by the grid's size)
@pytest.mark.parametrize("K", [1, 2, 5, 33, 300])  # 300: a second staged chunk of clients
@pytest.mark.parametrize("num_levels", LEVELS)
def test_fold_from_codes_equals_numpy(num_levels, K, share, cuda, monkeypatch):
    monkeypatch.setattr(_compress, "CODES_MIN_BLOCKS", 0 if share == "large" else _compress.CODES_MIN_BLOCKS)
    rs = np.random.RandomState(1000 * num_levels + K)
    names = [f"l{i}" for i in range(len(SIZES))]
    codes = [[rs.randint(0, num_levels, n).astype(np.uint8) for n in SIZES] for _ in range(K)]
    for r in codes:
        r[7][:num_levels] = np.arange(num_levels)  # every level occurs
        r[5][-3:] = 255                            # >= num_levels unless it is 256: clamped to the top
    minmax = np.empty((K, len(SIZES), 2), F32)
    minmax[..., 0] = rs.normal(size=minmax.shape[:2])
    minmax[..., 1] = minmax[..., 0] + np.abs(rs.normal(size=minmax.shape[:2]))
    minmax[:, 1, 1] = minmax[:, 1, 0]  # vmax == vmin
    minmax[:, 3, 1] = np.inf
    minmax[:, 4, 0] = np.nan
    weights = [float(x) for x in rs.uniform(0.5, 2.0, K)]
    want = decode_fold(codes, minmax, weights, num_levels)

    slab = fedjax_amd.CodeSlab({n: np.zeros(s, F32) for n, s in zip(names, SIZES)}, K, num_levels, device=cuda)
    clients = []
    for k in range(K):
        leaves = {}
        for n, c in zip(names, codes[k]):
            buf = torch.zeros(c.size + 1, dtype=torch.uint8, device=cuda)
            leaves[n] = buf[1:] if n == "l6" else buf[:-1]  # l6: one byte into its buffer
            leaves[n].copy_(torch.from_numpy(c))
        enc = comp.EncodedDelta(leaves, torch.from_numpy(minmax[k]).to(cuda), num_levels)
        assert leaves["l6"].data_ptr() % 16 == 1
        slab.set_client(k, enc)
        clients.append((k, enc, weights[k]))
    got_slab = slab.mean(weights)
    agg = comp.encoded_mean_aggregator(num_levels)
    got_agg, state = agg.apply(clients, agg.init())
    P, L = sum(SIZES), len(SIZES)
    assert state.num_bits == comp._bits_per_param(math.log2(num_levels), P, L)
    for n, w in zip(names, want):
        np.testing.assert_array_equal(bits(got_slab[n]), bits(w), err_msg=f"slab {n}")
        np.testing.assert_array_equal(bits(got_agg[n]), bits(w), err_msg=f"aggregator {n}")


@pytest.mark.parametrize("K", [1, 5, 33])
@pytest.mark.parametrize("num_levels", LEVELS)
def test_encode_then_fold_equals_the_fused_round(num_levels, K, cuda):
    rs = np.random.RandomState(77 * num_levels + K)
    shapes = {"a": (17,), "b": (5,), "c": (4097,), "d": (2, 4100)}  # d: two encoder workgroups
    deltas = []
    for k in range(K):
        t = {n: rs.normal(size=s).astype(F32) for n, s in shapes.items()}
        t["b"][:] = F32(0.25 * k)  # a constant leaf: range = 0
        deltas.append(t)
    deltas[0]["c"][100] = np.nan
    deltas[0]["a"][3] = np.inf
    weights = [float(x) for x in rs.randint(1, 50, K)]
    dev = [{n: torch.from_numpy(v).to(cuda) for n, v in t.items()} for t in deltas]
    rng = random.PRNGKey(num_levels + K)
    fused = comp.uniform_stochastic_quantizer(num_levels, rng)
    want, want_state = fused.apply([(k, d, w) for k, (d, w) in enumerate(zip(dev, weights))], fused.init())

    use_rng = random.split(rng)[1]
    client_keys = random.PRNGSequence(use_rng).take(K)
    enc = [comp.uniform_stochastic_encode_pytree(d, num_levels, ck) for d, ck in zip(dev, client_keys)]
    agg = comp.encoded_mean_aggregator(num_levels)
    got, state = agg.apply([(k, e, w) for k, (e, w) in enumerate(zip(enc, weights))], agg.init())
    assert state.num_bits == want_state.num_bits

    dslab = fedjax_amd.ClientDeltaSlab(deltas[0], K, device=cuda)
    for k, d in enumerate(dev):
        dslab.set_client(k, d)
    got_slab = fedjax_amd.CodeSlab(deltas[0], K, num_levels, device=cuda).encode_from(dslab, use_rng).mean(weights)
    for n in shapes:
        np.testing.assert_array_equal(bits(got[n]), bits(want[n]), err_msg=f"aggregator {n}")
        np.testing.assert_array_equal(bits(got_slab[n]), bits(want[n]), err_msg=f"slab {n}")


def test_captured_mean_reads_codes_afresh(cuda):
    K, num_levels = 5, 16
    slab = fedjax_amd.CodeSlab({"a": np.zeros(17, F32), "b": np.zeros(4097, F32)}, K, num_levels, device=cuda)
    weights = [1.0, 2.0, 3.0, 4.0, 5.0]
    out, eager = (torch.empty(slab.num_params, device=cuda) for _ in range(2))
    gen = torch.Generator(device=cuda).manual_seed(3)

    def rewrite():
        slab.storage.copy_(torch.randint(0, 256, slab.storage.shape, generator=gen, device=cuda, dtype=torch.uint8))
        slab.minmax.copy_(torch.rand(slab.minmax.shape, generator=gen, device=cuda).cumsum(-1))

    rewrite()
    slab.mean(weights, out=out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slab.mean(weights, out=out)
    for _ in range(3):
        rewrite()
        graph.replay()
        got = out.clone()
        slab.mean(weights, out=eager)
        np.testing.assert_array_equal(bits(got), bits(eager))


def _float_codes(e):
    return comp.EncodedDelta({n: v.float() for n, v in e.codes.items()}, e.minmax, e.num_levels)


REFUSALS = [
    (TypeError, lambda s, e, o: fedjax_amd.CodeSlab({"a": np.zeros(3, F32)}, 2, True)),
    (TypeError, lambda s, e, o: comp.encoded_mean_aggregator(4.0)),
    (ValueError, lambda s, e, o: fedjax_amd.CodeSlab({"a": np.zeros(3, F32)}, 2, 1)),
    (ValueError, lambda s, e, o: comp.encoded_mean_aggregator(257)),
    (TypeError, lambda s, e, o: s.set_client(0, _float_codes(e))),
    (TypeError, lambda s, e, o: comp.encoded_mean_aggregator(16).apply([(0, _float_codes(e), 1.0)], None)),
    (ValueError, lambda s, e, o: s.set_client(0, comp.EncodedDelta({"a": e.codes["a"]}, e.minmax[:1], 16))),
    (ValueError, lambda s, e, o: s.set_client(0, comp.EncodedDelta({"a": e.codes["a"], "b": e.codes["a"]}, e.minmax, 16))),
    (ValueError, lambda s, e, o: comp.encoded_mean_aggregator(16).apply(
        [(0, e, 1.0), (1, comp.EncodedDelta(e.codes, e.minmax, 8), 1.0)], None)),
    (ValueError, lambda s, e, o: s.set_client(1, comp.EncodedDelta(e.codes, e.minmax, 8))),
    (ValueError, lambda s, e, o: s.mean([1.0], out=o)),
    (ValueError, lambda s, e, o: s.mean([1.0, 2.0, 3.0], out=o)),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_come_before_any_launch(case, cuda):
    slab = fedjax_amd.CodeSlab({"a": np.zeros(17, F32), "b": np.zeros((3, 5), F32)}, 2, 16, device=cuda)
    out = torch.full((slab.num_params,), 7.0, device=cuda)
    exc, call = REFUSALS[case]
    with pytest.raises(exc):
        call(slab, slab.client(0), out)
    assert bool((out == 7.0).all()) and not bool(slab.storage.any()) and not bool(slab.minmax.any())
