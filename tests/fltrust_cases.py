"""What the two GPU test modules of FLTrust share: the rounds they run, the reference results (computed
once and kept read-only), the device layouts, and the comparison of a result with the reference."""
import functools

import numpy as np
import torch

from fedjax_amd import pytree, slab as slab_mod
from tests import fltrust_host as host
from tests import fltrust_ref as ref

F32, F64 = np.float32, np.float64
# the EMNIST-CNN leaf layout at 1/128 scale (tests/golden/make_golden.py), in flatten order
EMNIST_128 = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 2, 8)},
              "linear": {"b": (128,), "w": (72, 128)}, "linear_1": {"b": (62,), "w": (1, 62)}}
RESULT_FIELDS = ("trust", "cosines", "factors", "norms", "server_norm", "count", "total")
REF_NAMES = {"cosines": "cos"}


def tmap(f, t):
    return {k: tmap(f, v) for k, v in t.items()} if isinstance(t, dict) else f(t)


def leaf_sizes(shapes):
    return [z.size for z in pytree.leaves_of(tmap(lambda s: np.zeros(s, F32), shapes))]


def split(x, sizes):
    """A [K, P] (or [P]) array as the reference's list of leaves."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [x[..., offs[l]:offs[l + 1]] for l in range(len(sizes))]


def np_of(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def assert_same_bits(got, want, what):
    g, w = np.ascontiguousarray(np_of(got)), np.ascontiguousarray(np.asarray(want))
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    g, w = host.bits(g).reshape(-1), host.bits(w).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}: {g[bad[:4]]} {w[bad[:4]]}"


def check_result(got, want, what, mean=None):
    """Every field of an FLTrustResult against the reference's dict, bit for bit."""
    assert_same_bits(flat_of(got.mean) if mean is None else mean, np.concatenate([m.reshape(-1) for m in want["mean"]]),
                     what + " mean")
    for name in RESULT_FIELDS:
        assert_same_bits(getattr(got, name), want[REF_NAMES.get(name, name)], f"{what} {name}")


@functools.lru_cache(maxsize=None)
def mixed_round(K, P, seed=0):
    """(x [K, P], g [P]), read-only: honest clients around multiples of g, one in five pointing away
    from it, one in seven unrelated (a cosine near 0 of either sign)."""
    rng = np.random.RandomState(100 * seed + 3 * K + P)
    g = rng.standard_normal(P).astype(F32)
    scale = rng.uniform(0.2, 5.0, K).astype(F32)
    x = g[None] * scale[:, None] + F32(0.3) * scale[:, None] * rng.standard_normal((K, P)).astype(F32)
    x[::5] = -x[::5]
    x[3::7] = rng.standard_normal((len(x[3::7]), P)).astype(F32)
    x = x.astype(F32)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


@functools.lru_cache(maxsize=None)
def mixed_reference(K, P, sizes, seed=0):
    x, g = mixed_round(K, P, seed)
    return ref.fltrust(split(x, sizes), split(g, sizes))


def attack_round(P, seed=0):
    """(x, g, names): three honest clients, then the attack set: -10 g, all 1e30, one NaN, all zero,
    all inf, 1e-30 g."""
    rng = np.random.RandomState(seed + P)
    g = rng.standard_normal(P).astype(F32)
    honest = [(g * F32(s) + F32(0.05) * rng.standard_normal(P).astype(F32)).astype(F32) for s in (0.5, 1.0, 2.0)]
    nan = honest[1].copy()
    nan[P // 2] = np.nan
    attacks = {"minus": -10 * g, "huge": np.full(P, 1e30, F32), "nan": nan, "zero": np.zeros(P, F32),
               "inf": np.full(P, np.inf, F32), "tiny": F32(1e-30) * g}
    return np.stack(honest + [v.astype(F32) for v in attacks.values()]), g, ["h0", "h1", "h2"] + list(attacks)


def slab_of(x, shapes, dev):
    s = slab_mod.ClientDeltaSlab(tmap(lambda z: torch.zeros(z), shapes), x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x)))
    return s


def separate_clients(x, shapes, dev, misalign_leaf=3):
    """Client pytrees, every (client, leaf) its own allocation; one leaf of every client is a view one
    element into its buffer (4-byte aligned only)."""
    zs, td = pytree.flatten(tmap(lambda s: np.zeros(s, F32), shapes))
    offs = np.concatenate([[0], np.cumsum([z.size for z in zs])])
    clients = []
    for k in range(x.shape[0]):
        leaves = []
        for l, z in enumerate(zs):
            a = torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]]))
            if l == misalign_leaf:
                buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=dev)
                buf[1:].copy_(a)
                leaves.append(buf[1:].view(z.shape))
            else:
                leaves.append(a.to(dev).view(z.shape))
        clients.append(pytree.unflatten(td, leaves))
    return clients


def tree_of(v, shapes, dev):
    zs, td = pytree.flatten(tmap(lambda s: np.zeros(s, F32), shapes))
    offs = np.concatenate([[0], np.cumsum([z.size for z in zs])])
    return pytree.unflatten(td, [torch.from_numpy(np.array(v[offs[l]:offs[l + 1]])).to(dev).view(z.shape)
                                 for l, z in enumerate(zs)])


def on_device(x, dev, ld=None, offset=0):
    """x [K, P] as a device view with row stride ld and a base offset in elements; everything around
    the rows holds NaN (never read)."""
    K, P = x.shape
    ld = P if ld is None else ld
    store = torch.full((offset + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:].view(K, ld)[:, :P]
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def dev_vec(a, dev, offset=0):
    a = np.array(a, dtype=F32)
    store = torch.full((offset + a.size + 3,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    return view
