"""numpy restatement of bucketing for the coordinate-wise robust means (Karimireddy,
He and Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets via Bucketing", ICLR 2022,
Algorithm 1). The specification the kernels are held to, bit for bit; nothing here calls the
product.

K clients, bucket size s >= 1, a table perm of K client indices (None: the identity):
  1. B = ceil(K / s); bucket j has the members perm[j*s + i], i = 0 .. n_j - 1, n_j = min(s, K - j*s).
  2. per coordinate, in float32: a = the first member's value verbatim, a = fl(a + x) over the
     other members in table order; y_j = a if n_j == 1, else fl(a * f32(1 / n_j)) with a NaN
     result replaced by +NaN 0x7FC00000 (the sign of a computed NaN is not IEEE's to fix, and it
     decides which end of the order the bucket is trimmed from).
  3. the result is robust_mean_ref.trimmed_mean over y [B, P] with t counting buckets.
"""
import numpy as np

from tests import robust_mean_ref as trim_ref

B_MAX = 128
K_MAX = 4096


def bucket_count(K: int, s: int) -> int:
    return -(-K // s)


def bucket_means(x: np.ndarray, s: int, perm=None) -> np.ndarray:
    """float32 [B, P] of float32 ``x`` [K, P]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K, P = x.shape
    perm = np.arange(K) if perm is None else np.asarray(perm, dtype=np.int64)
    B = bucket_count(K, s)
    y = np.empty((B, P), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(B):
            members = perm[j * s:min((j + 1) * s, K)]
            a = x[members[0]].copy()
            for k in members[1:]:
                a = (a + x[k]).astype(np.float32)
            if len(members) == 1:
                y[j] = a
            else:
                m = (a * trim_ref.inverse(len(members))).astype(np.float32)
                y[j] = np.where(np.isnan(m), trim_ref.CANONICAL_NAN.view(np.float32), m)
    return y


def trimmed_mean(x: np.ndarray, s: int, t: int, perm=None) -> np.ndarray:
    return trim_ref.trimmed_mean(bucket_means(x, s, perm), t)


def median(x: np.ndarray, s: int, perm=None) -> np.ndarray:
    return trimmed_mean(x, s, (bucket_count(x.shape[0], s) - 1) // 2, perm)


def clamp(i: int, K: int) -> int:
    """The device tables' rule: an entry as an index into [0, K)."""
    return 0 if i < 0 else (K - 1 if i >= K else i)


def tables(K: int, seed: int):
    """The three tables of the tests: the identity (None), a seeded shuffle, the reversal."""
    return {"identity": None, "shuffle": np.random.RandomState(seed).permutation(K).astype(np.int32),
            "reversal": np.arange(K - 1, -1, -1, dtype=np.int32)}


# (K, s) of the GPU tests: B = 3, 17, 34, 65, 86, 128, 127 (a last bucket of one), 128, 1, 1
GPU_SHAPES = [(5, 2), (33, 2), (100, 3), (130, 2), (257, 3), (1024, 8), (4033, 32), (4096, 32), (129, 129), (40, 64)]


def trims(B: int):
    return sorted({t for t in (0, 1, (B - 1) // 2) if 2 * t < B})
