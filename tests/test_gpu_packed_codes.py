"""1-, 2- and 4-bit packed level codes: the mean folded from packed codes against a
numpy decode-and-fold of the unpacked codes, the packed encoder against the packing of the 8-bit
encoder's codes and the fused uniform_stochastic_quantizer round, capture, and the refusals.

Bar: bit for bit on int32 views, with every NaN taken as one NaN (as tests/test_gpu_codes_mean.py)."""
import math

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _compress, _lib, random
from fedjax_amd.aggregators import compression as comp

pytestmark = pytest.mark.gpu
F32 = np.float32
FORMS = [(2, 1), (2, 2), (3, 2), (4, 2), (5, 4), (16, 4)]  # (num_levels, bits)
# 4097 = _lib.PACKED_BLOCK + 1: a second workgroup of the large share for every bits; 8193: a third
SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 127, 129, 4095, _lib.PACKED_BLOCK + 1, 8193]


def bits_of(a):
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


@pytest.mark.parametrize("share", ["small", "large"])  # 8 or 16 elements a lane (chosen by the grid's size)
@pytest.mark.parametrize("K", [1, 5, 300])  # 300: a second staged chunk of clients
@pytest.mark.parametrize("num_levels,bits", FORMS)
def test_fold_from_packed_codes_equals_numpy(num_levels, bits, K, share, cuda, monkeypatch):
    monkeypatch.setattr(_compress, "CODES_MIN_BLOCKS", 0 if share == "large" else _compress.CODES_MIN_BLOCKS)
    rs = np.random.RandomState(1000 * num_levels + 10 * bits + K)
    names = [f"l{i:02d}" for i in range(len(SIZES))]
    per = 8 // bits
    # fields over the whole 2**bits range: those >= num_levels must clamp to the top level
    codes = [[rs.randint(0, 1 << bits, n).astype(np.uint8) for n in SIZES] for _ in range(K)]
    for r in codes:
        r[11][:num_levels] = np.arange(num_levels)  # every level occurs
    minmax = np.empty((K, len(SIZES), 2), F32)
    minmax[..., 0] = rs.normal(size=minmax.shape[:2])
    minmax[..., 1] = minmax[..., 0] + np.abs(rs.normal(size=minmax.shape[:2]))
    minmax[:, 1, 1] = minmax[:, 1, 0]  # vmax == vmin
    minmax[:, 3, 1] = np.inf
    minmax[:, 4, 0] = np.nan
    weights = [float(x) for x in rs.uniform(0.5, 2.0, K)]
    want = decode_fold(codes, minmax, weights, num_levels)

    template = {n: np.zeros(s, F32) for n, s in zip(names, SIZES)}
    shapes = tuple((s,) for s in SIZES)
    slab = fedjax_amd.CodeSlab(template, K, num_levels, bits, device=cuda)
    clients = []
    for k in range(K):
        leaves = {}
        for n, c in zip(names, codes[k]):
            packed = comp.pack_codes(torch.from_numpy(c), bits)
            if c.size % per:  # the padding bits of the last byte must not matter: all ones
                packed[-1] |= (0xFF << (bits * (c.size % per))) & 0xFF
            buf = torch.zeros(packed.numel() + 1, dtype=torch.uint8, device=cuda)
            leaves[n] = buf[1:] if n == "l10" else buf[:-1]  # l10: one byte into its buffer
            leaves[n].copy_(packed)
        assert leaves["l10"].data_ptr() % 16 == 1
        enc = comp.EncodedDelta(leaves, torch.from_numpy(minmax[k]).to(cuda), num_levels, bits, shapes)
        slab.set_client(k, enc)
        clients.append((k, enc, weights[k]))
    got_slab = slab.mean(weights)
    agg = comp.encoded_mean_aggregator(num_levels, bits, template)
    got_agg, state = agg.apply(clients, agg.init())
    assert state.num_bits == comp._bits_per_param(math.log2(num_levels), sum(SIZES), len(SIZES))
    for n, w in zip(names, want):
        np.testing.assert_array_equal(bits_of(got_slab[n]), bits_of(w), err_msg=f"slab {n}")
        np.testing.assert_array_equal(bits_of(got_agg[n]), bits_of(w), err_msg=f"aggregator {n}")


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("num_levels,bits", FORMS)
def test_packed_encode_is_the_packed_8_bit_encode_and_the_fused_round(num_levels, bits, K, cuda):
    rs = np.random.RandomState(77 * num_levels + 7 * bits + K)
    # d: h = 4103 is odd, 3 mod 4 and 7 mod 8 (misaligned for every bits), two encoder workgroups
    shapes = {"a": (17,), "b": (5,), "c": (4097,), "d": (8205,)}
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
    enc = [comp.uniform_stochastic_encode_pytree(d, num_levels, ck, bits=bits) for d, ck in zip(dev, client_keys)]
    for d, ck, e in zip(dev, client_keys, enc):
        e8 = comp.uniform_stochastic_encode_pytree(d, num_levels, ck)
        for n in shapes:
            np.testing.assert_array_equal(e.codes[n].cpu().numpy(), comp.pack_codes(e8.codes[n], bits).cpu().numpy(),
                                          err_msg=f"codes {n}")
        np.testing.assert_array_equal(bits_of(e.minmax), bits_of(e8.minmax))
    agg = comp.encoded_mean_aggregator(num_levels, bits=bits)
    got, state = agg.apply([(k, e, w) for k, (e, w) in enumerate(zip(enc, weights))], agg.init())
    assert state.num_bits == want_state.num_bits

    dslab = fedjax_amd.ClientDeltaSlab(deltas[0], K, device=cuda)
    for k, d in enumerate(dev):
        dslab.set_client(k, d)
    got_slab = fedjax_amd.CodeSlab(deltas[0], K, num_levels, bits=bits, device=cuda).encode_from(dslab, use_rng).mean(weights)
    for n in shapes:
        np.testing.assert_array_equal(bits_of(got[n]), bits_of(want[n]), err_msg=f"aggregator {n}")
        np.testing.assert_array_equal(bits_of(got_slab[n]), bits_of(want[n]), err_msg=f"slab {n}")


def test_captured_packed_mean_reads_codes_afresh(cuda):
    K, num_levels = 5, 16
    slab = fedjax_amd.CodeSlab({"a": np.zeros(17, F32), "b": np.zeros(4097, F32)}, K, num_levels, bits=4, device=cuda)
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
        np.testing.assert_array_equal(bits_of(got), bits_of(eager))


def _with(e, **kw):  # e with some leaves or fields replaced
    f = dict(codes=e.codes, minmax=e.minmax, num_levels=e.num_levels, bits=e.bits, shapes=e.shapes)
    return comp.EncodedDelta(**dict(f, **kw))


def _as_bytes(e):  # the same client as 8-bit codes
    return _with(e, codes={"a": torch.zeros(17, dtype=torch.uint8), "b": torch.zeros(3, 5, dtype=torch.uint8)},
                 bits=8, shapes=None)


TEMPLATE = {"a": np.zeros(17, F32), "b": np.zeros((3, 5), F32)}
REFUSALS = [
    (ValueError, lambda s, e, o: fedjax_amd.CodeSlab(TEMPLATE, 2, 16, bits=3)),
    (TypeError, lambda s, e, o: comp.encoded_mean_aggregator(2, bits=True)),
    (TypeError, lambda s, e, o: comp.uniform_stochastic_encode_pytree(TEMPLATE, 4, random.PRNGKey(0), bits=2.0)),
    (ValueError, lambda s, e, o: fedjax_amd.CodeSlab(TEMPLATE, 2, 16, bits=2)),
    (ValueError, lambda s, e, o: comp.encoded_mean_aggregator(3, bits=1)),
    (ValueError, lambda s, e, o: comp.uniform_stochastic_encode_pytree(TEMPLATE, 5, random.PRNGKey(0), bits=2)),
    (ValueError, lambda s, e, o: s.set_client(0, _with(e, codes={"a": e.codes["a"], "b": e.codes["b"][:-1]}))),
    (ValueError, lambda s, e, o: comp.encoded_mean_aggregator(16, 4).apply(
        [(0, _with(e, codes={"a": torch.zeros(17, dtype=torch.uint8), "b": e.codes["b"]}), 1.0)], None)),
    (TypeError, lambda s, e, o: s.set_client(0, _with(e, codes={"a": e.codes["a"].to(torch.int8), "b": e.codes["b"]}))),
    (ValueError, lambda s, e, o: s.set_client(0, _with(e, shapes=None))),
    (ValueError, lambda s, e, o: comp.encoded_mean_aggregator(16, 4, {"a": np.zeros(18, F32), "b": np.zeros((3, 5), F32)}
                                                              ).apply([(0, e, 1.0)], None)),
    (ValueError, lambda s, e, o: comp.encoded_mean_aggregator(16, 4).apply([(0, e, 1.0), (1, _as_bytes(e), 1.0)], None)),
    (ValueError, lambda s, e, o: s.set_client(1, _as_bytes(e))),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_packed_refusals_come_before_any_launch(case, cuda):
    slab = fedjax_amd.CodeSlab(TEMPLATE, 2, 16, bits=4, device=cuda)
    out = torch.full((slab.num_params,), 7.0, device=cuda)
    exc, call = REFUSALS[case]
    with pytest.raises(exc):
        call(slab, slab.client(0), out)
    assert bool((out == 7.0).all()) and not bool(slab.storage.any()) and not bool(slab.minmax.any())
