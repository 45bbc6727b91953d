"""numpy restatement of the coordinate-wise trimmed mean and median (Yin et al.,
"Byzantine-Robust Distributed Learning", ICML 2018). The specification the kernels are held to,
bit for bit; nothing here calls the product.

For one coordinate with values v_k, k = 0..K-1 (float32), and trim count t, 0 <= 2t < K:
  1. key(v) = bits(v) ^ (sign ? 0xFFFFFFFF : 0x80000000), compared as uint32: a total order
     -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; clients are ordered by (key, k).
  2. the kept clients are those of rank t .. K-1-t.
  3. s = the first kept value verbatim, then s = fl(s + v_k) over the kept clients in CLIENT order.
  4. y = fl(s * r), r = f32(1 / (K - 2t)) as tree_util._inverse forms it.
  5. the median is the rule at t = (K-1)//2.
"""
import math

import numpy as np

CANONICAL_NAN = np.uint32(0x7FC00000)
K_MAX = 128


def keys(x: np.ndarray) -> np.ndarray:
    """uint32 keys of float32 ``x`` whose unsigned order is the total order of item 1."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def kept_mask(x: np.ndarray, t: int) -> np.ndarray:
    """bool [K, P]: client k is kept in column p (stable argsort of the keys, ranks t..K-1-t)."""
    K = x.shape[0]
    if not (0 <= 2 * t < K):
        raise ValueError(f"need 0 <= 2t < K (t={t}, K={K})")
    order = np.argsort(keys(x), axis=0, kind="stable")  # ties by client index
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(K)[:, None].repeat(x.shape[1], 1), axis=0)
    return (rank >= t) & (rank <= K - 1 - t)


def kept_mask_by_counts(x: np.ndarray, t: int) -> np.ndarray:
    """The same mask from the sorted KEYS alone (the rule the kernel uses): L, U the keys of rank t
    and K-1-t; nL sorted positions < t hold L, nU positions > K-1-t hold U, cU clients have key U;
    a client is kept iff L <= key <= U, and if key == L its running index among the L-valued
    clients is >= nL, and if key == U its running index among the U-valued is < cU - nU."""
    K, P = x.shape
    k = keys(x)
    srt = np.sort(k, axis=0)
    keep = np.zeros((K, P), dtype=bool)
    for p in range(P):
        L, U = srt[t, p], srt[K - 1 - t, p]
        nL = int((srt[:t, p] == L).sum())
        nU = int((srt[K - t:, p] == U).sum())
        cU = int((k[:, p] == U).sum())
        iL = iU = 0
        for c in range(K):
            key = k[c, p]
            ok = L <= key <= U
            if key == L:
                ok = ok and iL >= nL
                iL += 1
            if key == U:
                ok = ok and iU < cU - nU
                iU += 1
            keep[c, p] = ok
    return keep


def inverse(W) -> np.float32:
    """tree_util._inverse: f32(1/W) from the Python float W."""
    return np.float32(1.0 / float(W))


def trimmed_mean(x: np.ndarray, t: int) -> np.ndarray:
    """float32 [P] of float32 ``x`` [K, P]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K, P = x.shape
    keep = kept_mask(x, t)
    s = np.zeros(P, dtype=np.float32)
    started = np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            nxt = np.where(started, (s + x[k]).astype(np.float32), x[k])
            s = np.where(keep[k], nxt, s)
            started |= keep[k]
        return (s * inverse(K - 2 * t)).astype(np.float32)


def median(x: np.ndarray) -> np.ndarray:
    return trimmed_mean(x, (x.shape[0] - 1) // 2)


def trim_count(trim, K: int) -> int:
    """The documented ``trim`` argument: an int count t, or a float fraction beta in [0, 0.5)
    giving t = floor(beta * K)."""
    if isinstance(trim, bool):
        raise TypeError("trim must be an int count or a float fraction, not a bool")
    if isinstance(trim, (int, np.integer)):
        return int(trim)
    beta = float(trim)
    if not (0.0 <= beta < 0.5):
        raise ValueError("fraction outside [0, 0.5)")
    return int(math.floor(beta * K))


def canon(a: np.ndarray) -> np.ndarray:
    """uint32 bits with every NaN canonicalised to 0x7FC00000."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), CANONICAL_NAN, a.view(np.uint32))


SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0], dtype=np.float32)


def special_bits() -> np.ndarray:
    """+NaN, -NaN, a payload NaN of each sign, +-inf, +-3e38, +-0 as uint32."""
    return np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000,
                     np.float32(3e38).view(np.uint32), np.float32(-3e38).view(np.uint32), 0, 0x80000000],
                    dtype=np.uint32)


def mixed_data(rng: np.random.RandomState, K: int, P: int, special: float = 0.1, ties: float = 0.1) -> np.ndarray:
    """float32 [K, P]: normal values with a ``special`` share of special_bits() and a ``ties``
    share drawn from a 3-value set."""
    x = rng.standard_normal((K, P)).astype(np.float32)
    u = rng.random_sample((K, P))
    three = np.array([-1.0, 0.5, 0.5000001], dtype=np.float32)
    x = np.where(u < ties, three[rng.randint(0, 3, (K, P))], x)
    sp = special_bits()[rng.randint(0, len(special_bits()), (K, P))].view(np.float32)
    return np.where((u >= ties) & (u < ties + special), sp, x).astype(np.float32)


def sweep_cases(n: int = 60, seed: int = 20181):
    """The seeded sweep of the GPU and CPU tests: (K, t, leaf sizes, data seed), valid by
    construction (0 <= 2t < K, 1 <= K <= 128)."""
    rng = np.random.RandomState(seed)
    cases = []
    for i in range(n):
        K = int(rng.choice([1, 2, 3, 5, 8, 15, 16, 17, 31, 33, 64, 65, 100, 128])) if i % 3 else int(rng.randint(1, 129))
        t = int(rng.randint(0, (K - 1) // 2 + 1))
        leaves = [int(rng.choice([0, 1, 3, 4, 63, 64, 65, 130, 257, 600])) for _ in range(int(rng.randint(1, 5)))]
        cases.append((K, t, leaves, int(rng.randint(0, 2**31 - 1))))
    return cases
