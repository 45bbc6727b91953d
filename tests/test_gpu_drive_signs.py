"""DRIVE's transmitted form: the mean folded from sign bits against a float64 numpy
inverse rotation and fold; clients encoded by drive_encode_pytree against the fused
structured_drive_quantizer round, bit for bit on int32 views with every NaN taken as one NaN (as
tests/test_gpu_packed_codes.py); the encoder against the packing of structured_rotation_pytree's
signs; zeros; and the refusals.

Leaf sizes: d = 1; 3 pads to 4, under a byte; 8, 9, 31, 33 byte and word edges; 4097 a full
single-pass tile half padding; 8193 two passes, the last of one stage; 2**16 + 1; 2**21 + 1 three
passes (K = 2 only). K = 300 crosses the kernel's staged chunk of 256 clients: the small leaves in both
tests, 4097 and 8193 (a full single-pass tile, a workspace tile) against float64 only.
Batches of 1 client, 2 clients (K = 5: 2 + 2 + 1) and all clients."""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _compress as C
from fedjax_amd import random
from fedjax_amd.aggregators import compression as comp
from fedjax_amd.aggregators import walsh_hadamard as wh

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = (1, 3, 8, 9, 31, 33)
ALL = SMALL + (4097, 8193, 2 ** 16 + 1)
BIG = (2 ** 21 + 1,)
MID = (4097, 8193)  # with K = 300: the staged chunk crossed at a full single-pass tile and at a workspace tile
CASES = [(ALL, 1, "all"), (ALL, 5, 1), (ALL, 5, 2), (ALL, 5, "all"), (SMALL, 300, 1), (SMALL, 300, 2),
         (SMALL, 300, "all"), (MID, 300, "all"), (BIG, 2, 1), (BIG, 2, "all")]


def bits_of(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F32).reshape(-1)
    return np.where(np.isnan(a), F32(np.nan), a).view(np.int32)


def budget(sizes, batch):
    return 1 << 40 if batch == "all" else batch * C.DriveSignsLayout(sizes).client_bytes


def names(sizes):
    return [f"l{i:02d}" for i in range(len(sizes))]


def hadamard64(x):
    x = x.astype(np.float64)
    h = 1
    while h < x.size:
        y = x.reshape(-1, 2, h)
        x = np.concatenate([y[:, :1] + y[:, 1:], y[:, :1] - y[:, 1:]], axis=1).reshape(-1)
        h *= 2
    return x


def rademacher(keys, ds, device):
    """+-1 float64 rotation signs of jobs (keys [J, 2], lengths ds) from random.rademacher (uniform < 0.5), not
    from the packed sign words the kernels under test read."""
    return [random.rademacher(k, int(d), device).cpu().numpy().astype(np.float64) for k, d in zip(keys, ds)]


@functools.lru_cache(maxsize=None)
def hand_made(sizes, K):
    """Random payloads, weights, and the float64 mean with its bound, per leaf."""
    cuda = torch.device("cuda:0")
    rs = np.random.RandomState(len(sizes) * 1000 + K)
    lay = C.DriveSignsLayout(sizes)
    signs = [[rs.randint(0, 256, int(b)).astype(np.uint8) for b in lay.nbytes] for _ in range(K)]
    for r in signs:
        for x, d in zip(r, lay.d):
            if d < 8:
                x |= (0xFF << int(d)) & 0xFF  # padding bits must not matter: all ones
    scales = rs.uniform(0.5, 2.0, (K, len(sizes), 2)).astype(F32)
    weights = [float(x) for x in rs.uniform(0.5, 2.0, K)]
    new_rng, client_keys = comp.drive_round_keys(random.PRNGKey(K), K)
    D = rademacher(random.split_many(client_keys, len(sizes)).reshape(-1, 2), np.tile(lay.d, K), cuda)
    want, bound = [], []
    for l, (n, d) in enumerate(zip(sizes, lay.d)):
        s = 0.0
        for k in range(K):
            sg = 1.0 - 2.0 * np.unpackbits(signs[k][l], bitorder="little")[:d]
            ab = float(scales[k, l, 0]) / float(scales[k, l, 1])
            s = s + weights[k] * (D[k * len(sizes) + l] * hadamard64(ab * sg) / np.sqrt(float(d)))[:n]
        want.append(s / sum(weights))
        ratio = (scales[:, l, 0].astype(np.float64) / scales[:, l, 1]).max()
        bound.append((np.log2(d) + K + 4) * 2.0 ** -24 * np.sqrt(float(d)) * ratio)
    return signs, scales, weights, new_rng, want, bound


@pytest.mark.parametrize("sizes,K,batch", CASES)
def test_fold_from_sign_bits_against_float64(sizes, K, batch, cuda):
    signs, scales, weights, new_rng, want, bound = hand_made(sizes, K)
    shapes = tuple((n,) for n in sizes)
    clients = []
    for k in range(K):
        leaves = {}
        for i, (nm, x) in enumerate(zip(names(sizes), signs[k])):
            buf = torch.zeros(x.size + 1, dtype=torch.uint8, device=cuda)
            leaves[nm] = buf[1:] if i == len(sizes) - 1 else buf[:-1]  # the last leaf: one byte into its buffer
            leaves[nm].copy_(torch.from_numpy(x))
        assert leaves[names(sizes)[-1]].data_ptr() % 4 == 1
        clients.append((k, comp.DriveDelta(leaves, torch.from_numpy(scales[k]).to(cuda), shapes), weights[k]))
    agg = comp.drive_mean_aggregator(random.PRNGKey(K), {nm: np.zeros(n, F32) for nm, n in zip(names(sizes), sizes)},
                                     workspace_bytes=budget(sizes, batch))
    got, state = agg.apply(clients, agg.init())
    assert state.num_bits == F32(sum(sizes) + 64 * len(sizes)) and np.array_equal(state.rng, new_rng)
    for nm, w, b in zip(names(sizes), want, bound):
        err = np.abs(got[nm].cpu().numpy().astype(np.float64) - w).max()
        print(f"{nm}: max error {err:.3e}, bound {b:.3e}")
        assert err <= b, nm


@functools.lru_cache(maxsize=None)
def fused_rounds(sizes, K):
    """Seeded normal deltas through two consecutive structured_drive_quantizer rounds: per round the
    clients' payloads (checked against the rotation's signs and float64 sums), the fused mean and state."""
    cuda = torch.device("cuda:0")
    gen = torch.Generator(device=cuda).manual_seed(len(sizes) * 100 + K)
    deltas = [{nm: torch.randn(n, generator=gen, device=cuda) for nm, n in zip(names(sizes), sizes)} for _ in range(K)]
    weights = [float(x) for x in np.random.RandomState(K).randint(1, 50, K)]
    fused = comp.structured_drive_quantizer(random.PRNGKey(7 + K))
    state, rounds = fused.init(), []
    for _ in range(2):
        _, client_keys = comp.drive_round_keys(state.rng, K)
        enc = [comp.drive_encode_pytree(d, ck) for d, ck in zip(deltas, client_keys)]
        for d, ck, e in zip(deltas, client_keys, enc):
            rot, _ = wh.structured_rotation_pytree(d, ck)
            y = torch.cat([rot[nm] for nm in names(sizes)])
            # the premise of the bitwise comparison: no rotated coordinate is zero or NaN
            assert bool((y != 0).all()) and not bool(torch.isnan(y).any())
            want = torch.cat([comp.pack_codes((rot[nm] < 0).to(torch.uint8), 1) for nm in names(sizes)])
            assert torch.equal(torch.cat([e.signs[nm] for nm in names(sizes)]), want)
            y64 = [rot[nm].cpu().numpy().astype(np.float64) for nm in names(sizes)]
            np.testing.assert_array_equal(e.scales.cpu().numpy(),
                                          [[F32((v * v).sum()), F32(np.abs(v).sum())] for v in y64])
        mean, state = fused.apply([(k, d, w) for k, (d, w) in enumerate(zip(deltas, weights))], state)
        rounds.append((enc, mean, state))
    return weights, rounds


# (without MID x 300: among its 1.5e7 rotated coordinates an exact zero is likely, and the premise would not hold)
@pytest.mark.parametrize("sizes,K,batch", [c for c in CASES if c[0] is not MID])
def test_round_trip_is_the_fused_round_bit_for_bit(sizes, K, batch, cuda):
    weights, rounds = fused_rounds(sizes, K)
    agg = comp.drive_mean_aggregator(random.PRNGKey(7 + K), workspace_bytes=budget(sizes, batch))
    state = agg.init()
    for enc, want, want_state in rounds:
        got, state = agg.apply([(k, e, w) for k, (e, w) in enumerate(zip(enc, weights))], state)
        assert state.num_bits == want_state.num_bits and np.array_equal(state.rng, want_state.rng)
        for nm in names(sizes):
            np.testing.assert_array_equal(bits_of(got[nm]), bits_of(want[nm]), err_msg=nm)


def test_zero_leaf_and_zero_coordinate(cuda):
    key = random.PRNGKey(3)
    delta = {"a": torch.randn(33, device=cuda), "z": torch.zeros(9, device=cuda), "o": torch.ones(2, device=cuda)}
    _, ck = comp.drive_round_keys(key, 1)
    enc = comp.drive_encode_pytree(delta, ck[0])
    assert not bool(enc.signs["z"].any()) and bits_of(enc.scales[2]).tolist() == [0, 0]  # flatten order: a, o, z
    agg = comp.drive_mean_aggregator(key)
    got, _ = agg.apply([(0, enc, 1.0)], agg.init())
    fused = comp.structured_drive_quantizer(key)
    want, _ = fused.apply([(0, delta, 1.0)], fused.init())
    assert bool(torch.isnan(got["z"]).all()) and bool(torch.isnan(want["z"]).all())
    np.testing.assert_array_equal(bits_of(got["a"]), bits_of(want["a"]))
    # x = (1, 1): one rotated coordinate is exactly zero. It is sent as + and decodes to +A/b (the
    # fused round has sign(0) = 0 there): the one documented difference.
    rot, _ = wh.structured_rotation_pytree(delta, ck[0])
    y = rot["o"].cpu().numpy()
    assert (y == 0).sum() == 1 and int(enc.signs["o"][0]) == int(y[0] < 0) | int(y[1] < 0) << 1
    A, b = (float(v) for v in enc.scales[1].cpu().numpy())
    D = rademacher(random.split(ck[0], 3)[1:2], [2], cuda)[0]
    ref = D * hadamard64(A / b * np.where(y < 0, -1.0, 1.0)) / np.sqrt(2.0)
    assert np.abs(got["o"].cpu().numpy() - ref).max() <= (1 + 1 + 4) * 2.0 ** -24 * np.sqrt(2.0) * A / b
    assert not np.array_equal(bits_of(got["o"]), bits_of(want["o"]))


def _delta(**kw):
    f = dict(signs={"a": torch.zeros(4, dtype=torch.uint8), "b": torch.zeros(2, dtype=torch.uint8)},
             scales=torch.ones(2, 2), shapes=((17,), (3, 5)))
    return comp.DriveDelta(**dict(f, **kw))


REFUSALS = [
    (TypeError, lambda: [{"a": torch.zeros(17)}]),
    (TypeError, lambda: [_delta(signs={"a": torch.zeros(4, dtype=torch.int8), "b": torch.zeros(2, dtype=torch.uint8)})]),
    (ValueError, lambda: [_delta(signs={"a": torch.zeros(3, dtype=torch.uint8), "b": torch.zeros(2, dtype=torch.uint8)})]),
    (ValueError, lambda: [_delta(), _delta(shapes=((17,), (5, 3)))]),
    (ValueError, lambda: [_delta(shapes=((18,), (3, 5)))]),  # against the template
    (TypeError, lambda: [_delta(scales=torch.ones(2, 2, dtype=torch.float64))]),
    (ValueError, lambda: [_delta(scales=torch.ones(2))]),
    (ValueError, lambda: [_delta(), _delta(signs={"a": torch.zeros(4, dtype=torch.uint8)})]),  # another structure
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_drive_refusals(case, cuda):
    exc, clients = REFUSALS[case]
    agg = comp.drive_mean_aggregator(random.PRNGKey(0), {"a": np.zeros(17, F32), "b": np.zeros((3, 5), F32)})
    with pytest.raises(exc):
        agg.apply([(k, d, 1.0) for k, d in enumerate(clients())], agg.init())
