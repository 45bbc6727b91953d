"""numpy restatement of the mean around the median ("MeaMed", Xie, Koyejo and Gupta,
"Generalized Byzantine-tolerant SGD", 2018; the coordinate-wise stage of Bulyan). The
specification the kernels are held to, bit for bit; nothing here calls the product.

For one coordinate with float32 values v_k, k = 0..K-1, and keep count beta, 1 <= beta <= K:
  1. key(v) and the total order are the trimmed mean's (tests/robust_mean_ref.py); clients are
     ordered by (key, k); s_0 .. s_{K-1} are the values in that order.
  2. mid = (K-1)//2, med = s_mid: the lower median, a value of the data.
  3. d_j = 0 if key(s_j) == key(med), else |fl(s_j - med)| with a NaN result replaced by +inf.
  4. the kept sorted positions are [a, a + beta). Written two ways:
       greedy: grow from {mid}; take the side with the strictly smaller distance, the lower side
               on a tie, the other side when one is exhausted;
       count:  a_lo = max(0, mid-beta+1), a_hi = min(mid, K-beta),
               a = a_lo + #{ i in [a_lo, a_hi) : d[i+beta] < d[i] }.
  5. s = the first kept value verbatim, then s = fl(s + v_k) over the kept clients in CLIENT order.
  6. y = fl(s * f32(1/beta)).
"""
import numpy as np

from tests import robust_mean_ref as rm

F32 = np.float32
K_MAX = 128
keys = rm.keys
canon = rm.canon
inverse = rm.inverse


def values_of(k: np.ndarray) -> np.ndarray:
    """float32 values of uint32 keys (the inverse of keys())."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(F32)


def distances(srt: np.ndarray) -> np.ndarray:
    """float32 [K, P]: item 3 for sorted keys ``srt`` [K, P]."""
    K = srt.shape[0]
    mk = srt[(K - 1) // 2]
    with np.errstate(all="ignore"):
        d = np.abs((values_of(srt) - values_of(mk)[None, :]).astype(F32))
    d = np.where(np.isnan(d), F32(np.inf), d)
    return np.where(srt == mk[None, :], F32(0), d).astype(F32)


def _check(K, beta):
    if not (1 <= beta <= K):
        raise ValueError(f"need 1 <= beta <= K (beta={beta}, K={K})")


def window_start_by_counts(x: np.ndarray, beta: int) -> np.ndarray:
    """int [P]: the first kept sorted position by the count rule."""
    K = x.shape[0]
    _check(K, beta)
    d = distances(np.sort(keys(x), axis=0))
    mid = (K - 1) // 2
    a_lo, a_hi = max(0, mid - beta + 1), min(mid, K - beta)
    if a_hi <= a_lo:
        return np.full(x.shape[1], a_lo, dtype=np.int64)
    return a_lo + (d[a_lo + beta:a_hi + beta] < d[a_lo:a_hi]).sum(axis=0)


def window_start_greedy(x: np.ndarray, beta: int) -> np.ndarray:
    """int [P]: the first kept sorted position by the two-pointer greedy, column by column."""
    K, P = x.shape
    _check(K, beta)
    d = distances(np.sort(keys(x), axis=0))
    mid = (K - 1) // 2
    out = np.empty(P, dtype=np.int64)
    for p in range(P):
        lo = hi = mid
        while hi - lo + 1 < beta:
            if lo == 0:
                hi += 1
            elif hi == K - 1:
                lo -= 1
            elif d[hi + 1, p] < d[lo - 1, p]:
                hi += 1
            else:
                lo -= 1
        out[p] = lo
    return out


def kept_mask(x: np.ndarray, beta: int) -> np.ndarray:
    """bool [K, P] by the greedy and the stable argsort of the keys (ties by client index)."""
    K, P = x.shape
    a = window_start_greedy(x, beta)
    order = np.argsort(keys(x), axis=0, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(K)[:, None].repeat(P, 1), axis=0)
    return (rank >= a[None, :]) & (rank < a[None, :] + beta)


def kept_mask_by_counts(x: np.ndarray, beta: int) -> np.ndarray:
    """The same mask from the sorted KEYS alone (the rule the kernel uses): the count rule for the
    window, then the trimmed mean's tie cuts with two trim counts t_lo = a, t_hi = K - beta - a."""
    K, P = x.shape
    k = keys(x)
    srt = np.sort(k, axis=0)
    a = window_start_by_counts(x, beta)
    L = np.take_along_axis(srt, a[None, :], axis=0)[0]
    U = np.take_along_axis(srt, (a + beta - 1)[None, :], axis=0)[0]
    below, above, cU = (srt < L).sum(0), (srt > U).sum(0), (srt == U).sum(0)
    nL, keepU = a - below, cU - (K - beta - a - above)
    isL, isU = k == L, k == U
    iL = np.cumsum(isL, axis=0) - isL  # running index among the L-valued, before this client
    iU = np.cumsum(isU, axis=0) - isU
    return (k >= L) & (k <= U) & (~isL | (iL >= nL)) & (~isU | (iU < keepU))


def mean_around_median(x: np.ndarray, beta: int, mask=kept_mask_by_counts) -> np.ndarray:
    """float32 [P] of float32 ``x`` [K, P]."""
    x = np.ascontiguousarray(x, dtype=F32)
    K, P = x.shape
    keep = mask(x, beta)
    s = np.zeros(P, dtype=F32)
    started = np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            nxt = np.where(started, (s + x[k]).astype(F32), x[k])
            s = np.where(keep[k], nxt, s)
            started |= keep[k]
        return (s * inverse(beta)).astype(F32)


def bits(a) -> list:
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32).ravel().tolist()


def integer_ties(rng: np.random.RandomState, K: int, P: int) -> np.ndarray:
    """Small integers: many equal values, equal distances on both sides of the median."""
    return rng.randint(-3, 4, (K, P)).astype(F32)


def specials(rng: np.random.RandomState, K: int, P: int) -> np.ndarray:
    """Normal values, small-integer ties and +-0, +-inf, +-NaN, +-1e30, a third each on average."""
    x = rng.standard_normal((K, P)).astype(F32)
    sp = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                   F32(1e30).view(np.uint32), F32(-1e30).view(np.uint32)], dtype=np.uint32).view(F32)
    u = rng.random_sample((K, P))
    x = np.where(u < 0.33, integer_ties(rng, K, P), x)
    return np.where(u > 0.67, sp[rng.randint(0, len(sp), (K, P))], x).astype(F32)


def poisoned(rng: np.random.RandomState, K: int, P: int) -> np.ndarray:
    """Mostly +-inf and +-NaN: the median itself is non-finite in most columns."""
    sp = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000], dtype=np.uint32).view(F32)
    x = rng.standard_normal((K, P)).astype(F32)
    return np.where(rng.random_sample((K, P)) < 0.7, sp[rng.randint(0, 4, (K, P))], x).astype(F32)


DATA = {"normal": lambda rng, K, P: rng.standard_normal((K, P)).astype(F32), "ties": integer_ties,
        "specials": specials, "poisoned": poisoned}


def edge_ties(x: np.ndarray, beta: int) -> int:
    """Columns whose window edge cuts through equal keys or has equal distances on both sides."""
    K = x.shape[0]
    srt = np.sort(keys(x), axis=0)
    d = distances(srt)
    a = window_start_by_counts(x, beta)
    cols = np.arange(x.shape[1])
    n = np.zeros(x.shape[1], dtype=bool)
    lo_ok, hi_ok = a > 0, a + beta < K
    n |= lo_ok & (srt[np.maximum(a - 1, 0), cols] == srt[a, cols])
    n |= hi_ok & (srt[np.minimum(a + beta, K - 1), cols] == srt[a + beta - 1, cols])
    n |= lo_ok & hi_ok & (d[np.maximum(a - 1, 0), cols] == d[np.minimum(a + beta, K - 1), cols])
    return int(n.sum())


def nonfinite_medians(x: np.ndarray) -> int:
    srt = np.sort(keys(x), axis=0)
    return int((~np.isfinite(values_of(srt[(x.shape[0] - 1) // 2]))).sum())


def width_of(K: int) -> int:
    return 16 if K <= 16 else 32 if K <= 32 else 64 if K <= 64 else 128


def fuzz_cases(n: int = 60, seed: int = 20182):
    """The seeded fuzz of the GPU tests: (aggregate, K, f or beta, leaf sizes, data kind, seed).
    aggregate "meamed": K clients, keep beta; "bulyan": K clients, f Byzantine (K >= 4f + 3,
    K - 2f <= 128)."""
    rng = np.random.RandomState(seed)
    cases = []
    for i in range(n):
        leaves = [int(rng.choice([0, 1, 3, 4, 63, 65, 130, 257, 600])) for _ in range(int(rng.randint(1, 5)))]
        if sum(leaves) == 0:
            leaves.append(5)
        if i % 3 == 2:
            f = int(rng.randint(0, 6))
            K = int(rng.randint(4 * f + 3, 4 * f + 3 + 40))
            cases.append(("bulyan", K, f, leaves, "ints", int(rng.randint(0, 2**31 - 1))))
        else:
            edges = [1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 64, 65, 100, 127, 128]
            K = int(rng.choice(edges)) if i % 2 else int(rng.randint(1, 129))
            beta = int(rng.randint(1, K + 1))
            kind = ["normal", "ties", "specials", "poisoned"][i % 4]
            cases.append(("meamed", K, beta, leaves, kind, int(rng.randint(0, 2**31 - 1))))
    return cases
