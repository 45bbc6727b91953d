"""signSGD with majority vote: k_sign_vote against a numpy column count of the
unpacked bits, k_sign_pack against pack_codes of (x < 0), and majority_vote_aggregator end to end.

Bar: exact. Every comparison is array_equal on the float32 values, plus a sign-bit check that a
tie is +0. The reference is ``np.unpackbits(..., bitorder="little")``, a column sum and the two
output formulas."""
import numpy as np
import pytest
import torch

from fedjax_amd import _compress as C
from fedjax_amd import _lib
from fedjax_amd.aggregators import compression as comp

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = _lib.VOTE_TILE
SMALL = [1, 7, 8, 9, 31, 33, 127, 129]
SIZES = SMALL + [4097, TILE - 1, TILE, TILE + 1]
MODES = {"sign": _lib.VOTE_SIGN, "mean": _lib.VOTE_MEAN}


def want(bits, n, output):
    """bits [K, ceil(n / 8)] uint8: c = clients whose bit is 1, per coordinate; the two formulas."""
    K = bits.shape[0]
    c = np.unpackbits(bits, axis=1, bitorder="little")[:, :n].sum(axis=0, dtype=np.int64)
    if output == "sign":
        return np.where(2 * c > K, F32(-1), np.where(2 * c < K, F32(1), F32(0))).astype(F32)
    return (K - 2 * c).astype(F32) * F32(1.0 / K)


def random_bits(rs, K, n):
    """[K, ceil(n / 8)] packed rows; a coordinate's probability of a 1 is 0, 1, 0.5 or uniform."""
    kind = rs.randint(0, 4, n)
    prob = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, np.where(kind == 2, 0.5, rs.rand(n))))
    return np.packbits(rs.rand(K, n) < prob, axis=1, bitorder="little")


def device_rows(leaves, dev, shift=0):
    """leaves [L] of [K, nbytes] arrays as [K][L] views of one device buffer: leaf l of every client
    starts `shift` bytes past a 16-byte boundary."""
    K = leaves[0].shape[0]
    offs = np.concatenate([[0], np.cumsum([(b.shape[1] + shift + 31) // 16 * 16 for b in leaves])])
    host = np.zeros((K, int(offs[-1])), np.uint8)
    for b, o in zip(leaves, offs):
        host[:, o + shift:o + shift + b.shape[1]] = b
    buf = torch.from_numpy(host).to(dev)
    return [[buf[k, o + shift:o + shift + b.shape[1]] for b, o in zip(leaves, offs)] for k in range(K)]


def vote(leaves, sizes, output, dev, shift=0):
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for n in sizes]
    C.sign_vote(device_rows(leaves, dev, shift), MODES[output], outs)
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("output", ["sign", "mean"])
@pytest.mark.parametrize("K", [1, 2, 3, 7, 8, 9, 31, 32, 33, 255, 256, 257, 4095, 4096])
def test_vote_equals_numpy(K, output, cuda):
    """Every remainder of the group of 8 and of the 4-wave split, every plane; the sizes end
    mid-byte, mid-word and one past a workgroup tile (the big K with the small leaves only)."""
    rs = np.random.RandomState(K)
    sizes = SIZES if K <= 257 else SMALL
    leaves = [random_bits(rs, K, n) for n in sizes]
    for got, b, n in zip(vote(leaves, sizes, output, cuda), leaves, sizes):
        assert np.array_equal(got, want(b, n, output)), (K, n)


@pytest.mark.parametrize("output", ["sign", "mean"])
@pytest.mark.parametrize("K", [2, 8, 4095, 4096])
def test_carries_and_ties(K, output, cuda):
    """Coordinate i: all K set (i % 4 == 0), K // 2 set (1), K - 1 set (2), one set (3)."""
    n = 129
    c = np.array([K, K // 2, K - 1, 1])[np.arange(n) % 4]
    b = np.packbits(np.arange(K)[:, None] < c[None, :], axis=1, bitorder="little")
    got = vote([b], [n], output, cuda)[0]
    assert np.array_equal(got, want(b, n, output))
    assert (got[0::4] == (-1 if output == "sign" else F32(-K) * F32(1.0 / K))).all()
    if K % 2 == 0:  # exactly half: +0.0 in both modes
        assert (got[1::4] == 0).all() and not np.signbit(got[1::4]).any()


@pytest.mark.parametrize("output", ["sign", "mean"])
def test_memory_edges(output, cuda):
    """Bit rows one byte past a 16-byte boundary, padding bits set by hand, outputs at 4-byte
    aligned, not 16-byte aligned offsets of a sentinel-filled buffer, three leaves ending mid-byte
    and mid-word."""
    K, sizes = 9, [13, TILE + 45, 70]
    rs = np.random.RandomState(5)
    leaves = [random_bits(rs, K, n) for n in sizes]
    ref = [want(b, n, output) for b, n in zip(leaves, sizes)]
    for b, n in zip(leaves, sizes):
        b[:, -1] |= (0xFF << (n % 8)) & 0xFF  # the padding bits: must change nothing
    buf = torch.full((sum(sizes) + 40,), 7.0, dtype=torch.float32, device=cuda)
    starts = [1, 1 + 13 + 4, 1 + 13 + 4 + TILE + 45 + 8]  # elements: 1, 18, 8263 (none a multiple of 4)
    outs = [buf[s:s + n] for s, n in zip(starts, sizes)]
    assert all(o.data_ptr() % 16 for o in outs)
    C.sign_vote(device_rows(leaves, cuda, shift=1), MODES[output], outs)
    host = buf.cpu().numpy()
    keep = np.ones(host.size, bool)
    for s, n, r in zip(starts, sizes, ref):
        assert np.array_equal(host[s:s + n], r), n
        keep[s:s + n] = False
    assert (host[keep] == 7.0).all()


def test_encoder_equals_pack_codes(cuda):
    """x < 0 bit by bit, special values included; pack_codes writes the padding bits as zero."""
    rs = np.random.RandomState(2)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0], F32)
    tree = {}
    for n in (1, 8, 9, (16 << 10) + 3):
        x = rs.standard_normal(n).astype(F32)
        x[:min(n, special.size)] = rs.permutation(special)[:min(n, special.size)]
        tree[f"l{n:05d}"] = torch.from_numpy(x).to(cuda)
    tree["l00001"] = torch.tensor([-0.5], device=cuda)
    d = comp.sign_encode_pytree(tree)
    assert d.shapes == tuple((v.numel(),) for _, v in sorted(tree.items()))
    for name, x in tree.items():
        assert torch.equal(d.signs[name], comp.pack_codes((x < 0).to(torch.uint8), 1)), name
    with pytest.raises(TypeError, match="bfloat16"):
        comp.sign_encode_pytree({"a": torch.zeros(4, dtype=torch.bfloat16, device=cuda)})


def test_aggregator_end_to_end(cuda):
    K = 9
    rs = np.random.RandomState(11)
    shapes = {"b": (5,), "w": (3, 37), "z": (TILE + 3,)}
    clients = [{n: rs.standard_normal(s).astype(F32) for n, s in shapes.items()} for _ in range(K)]
    for t in clients[:5]:
        t["b"][0] = 0.0  # a zero is sent as 0: it counts as a plus
    P = sum(int(np.prod(s)) for s in shapes.values())
    deltas = [comp.sign_encode_pytree({n: torch.from_numpy(v).to(cuda) for n, v in t.items()}) for t in clients]
    for output in ("sign", "mean"):
        agg = comp.majority_vote_aggregator(output, template=clients[0])
        state = agg.init()
        got, state = agg.apply([(k, d, 1.0) for k, d in enumerate(deltas)], state)
        again, state = agg.apply([(k, d, 100.0 * k) for k, d in enumerate(deltas)], state)  # weights are ignored
        for n, s in shapes.items():
            c = sum((t[n] < 0).astype(np.int64) for t in clients)  # reference on the floats: zero counts as plus
            ref = (np.where(2 * c > K, F32(-1), F32(1)) if output == "sign" else (K - 2 * c).astype(F32) * F32(1.0 / K))
            assert got[n].shape == s and np.array_equal(got[n].cpu().numpy(), ref.astype(F32)), (output, n)
            assert torch.equal(got[n], again[n])
        assert state.rng is None and state.num_bits == F32(F32(P) + F32(P))
        assert agg.apply([], state) == (None, state)
    agg = comp.majority_vote_aggregator()
    d0 = deltas[0]
    bad_dtype = comp.SignDelta({n: v.to(torch.int8) for n, v in d0.signs.items()}, d0.shapes)
    bad_bytes = comp.SignDelta({n: v[:-1] for n, v in d0.signs.items()}, d0.shapes)
    bad_shape = comp.SignDelta(d0.signs, ((5,), (37, 3), (TILE + 3,)))
    for bad, err in ((clients[0], TypeError), (bad_dtype, TypeError), (bad_bytes, ValueError)):
        with pytest.raises(err):
            agg.apply([(0, bad, 1.0)], agg.init())
    with pytest.raises(ValueError, match="leaf shapes"):
        agg.apply([(0, d0, 1.0), (1, bad_shape, 1.0)], agg.init())
    with pytest.raises(ValueError, match="4096"):
        agg.apply([(k, d0, 1.0) for k in range(4097)], agg.init())
