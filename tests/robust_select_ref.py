"""Restatements for the Gram-matrix aggregates, on the client VECTORS in float64 — no Gram
matrix anywhere: brute-force Krum (Blanchard et al., NeurIPS 2017) and the direct-form smoothed
Weiszfeld iteration (Pillutla et al., IEEE TSP 2022). Plus a numpy emulation of the Gram kernel's
arithmetic (float32 fmaf chains of C columns, added in float64), as a yardstick for accuracy."""
import numpy as np


def krum_scores(x, f):
    """score_i = sum of the K - f - 2 smallest |x_i - x_j|^2, j != i; inf for a non-finite row
    (a row is compared only with finite rows; a non-finite neighbour is infinitely far)."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    finite = [bool(np.isfinite(x[k]).all()) for k in range(K)]
    scores = []
    for i in range(K):
        if not finite[i]:
            scores.append(np.inf)
            continue
        d = []
        for j in range(K):
            if j == i:
                continue
            if not finite[j]:
                d.append(np.inf)
                continue
            diff = x[i] - x[j]
            d.append(float(np.dot(diff, diff)))
        d.sort()
        s = 0.0
        for v in d[: K - f - 2]:
            s += v
        scores.append(s)
    return np.array(scores, dtype=np.float64)


def krum_select(x, f, m):
    """The m finite-score clients of smallest score, ties to the lower index."""
    scores = krum_scores(x, f)
    order = sorted(range(len(scores)), key=lambda k: (scores[k], k))
    return np.array([k for k in order if np.isfinite(scores[k])][:m], dtype=np.int64), scores


def weiszfeld(x, alpha, nu, iterations):
    """Direct form on the vectors: v = sum a_k x_k; d_k = |v - x_k|; beta_k = alpha_k / max(nu, d_k);
    a = beta / sum beta. Returns (a, v) with v the final point sum a_k x_k. Finite rows only."""
    x = np.asarray(x, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    a = alpha / alpha.sum()
    for _ in range(iterations):
        v = a @ x
        d = np.sqrt(((x - v[None, :]) ** 2).sum(axis=1))
        beta = alpha / np.maximum(nu, d)
        a = beta / beta.sum()
    return a, a @ x


def chain_gram(x, chain):
    """The Gram kernel's arithmetic in numpy: per chain of `chain` columns, every pair's products
    accumulated in float32 in column order from +0 (the float64 product is exact, the float64 sum
    is then rounded to float32: an fmaf up to rare double roundings, which a yardstick can
    live with — this is not a bitwise reference); chains added in float64."""
    x = np.asarray(x, dtype=np.float32)
    K, P = x.shape
    G = np.zeros((K, K), dtype=np.float64)
    x64 = x.astype(np.float64)
    for c0 in range(0, P, chain):
        acc = np.zeros((K, K), dtype=np.float32)
        for p in range(c0, min(P, c0 + chain)):
            acc = (acc.astype(np.float64) + np.outer(x64[:, p], x64[:, p])).astype(np.float32)
        G += acc.astype(np.float64)
    return G


def outlier_data(rng, K, P, outliers):
    """0.01 * N(0, 1) honest clients and `outliers` N(0, 1) ones at the end, float32."""
    x = (0.01 * rng.standard_normal((K, P))).astype(np.float32)
    if outliers:
        x[K - outliers:] = rng.standard_normal((outliers, P)).astype(np.float32)
    return x
