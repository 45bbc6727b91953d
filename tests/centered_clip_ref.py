"""Numpy float32 restatement of centered clipping (no product code).

Karimireddy, He and Jaggi (ICML 2021): the mean of the clients, each clipped to l2 distance tau
from a centre v, taken around that centre. One iteration of this project's contract:

    d_k = fl(x_k - v)                             float32, per element
    q_k = sum of fl(d_k^2);  n_k = sqrt(q_k)      float32 (the library's own reduction order)
    c_k = minimum(1, tau / n_k)                   float32, NaN propagates (clip_factors_ref)
    t_k = c_k > 0 ? fl(c_k * d_k) : +0            a client with c NaN, 0 or negative adds nothing
    s   = +0;  s = fl(s + t_k)                    in client order
    v'  = fl(v + fl(s * f32(1/K)))                the divisor is K, whatever was skipped

numpy's float32 ``-``, ``*``, ``+``, ``/`` and ``sqrt`` are correctly rounded IEEE operations, so
every step below is the contract's rounding. The one thing numpy cannot restate is the ORDER in
which the library adds the squares: ``centered_clip_ref`` without ``factors`` takes q from a
float64 sum rounded once — a stand-in, within 2e-6 of any float32 order, and documented as such;
with ``factors`` (the library's own) the folds are exact restatements.
"""
import numpy as np

from tests.clipped_mean_ref import clip_factors_ref

F32 = np.float32


def centered_fold_ref(x, v, c):
    """One fold: v' = v + (1/K) sum_k [c_k > 0] c_k (x_k - v), float32, client by client from +0."""
    x = np.asarray(x, dtype=F32)
    v = np.asarray(v, dtype=F32)
    c = np.asarray(c, dtype=F32)
    K = x.shape[0]
    s = np.zeros(x.shape[1], dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(K):
            if not c[k] > 0:  # NaN, zero or negative: the row's bits are not touched
                continue  # (s is never -0, so adding +0 would leave the same bits)
            d = (x[k] - v).astype(F32)
            s = (s + (c[k] * d).astype(F32)).astype(F32)
        return (v + (s * F32(1.0 / K)).astype(F32)).astype(F32)


def centered_distances_f64(x, v):
    """l2 distance of every row of ``x`` from ``v`` in float64, of the FLOAT32 differences."""
    with np.errstate(all="ignore"):
        d = (np.asarray(x, dtype=F32) - np.asarray(v, dtype=F32)).astype(F32).astype(np.float64)
        return np.sqrt((d * d).sum(axis=1))


def stand_in_norms(x, v):
    """n_k as float32 from a float64 sum of the float32 squares, rounded once: NOT the library's
    order (any float32 order is within 2e-6 of it), only a stand-in for tests of the rule itself."""
    with np.errstate(all="ignore"):
        d = (np.asarray(x, dtype=F32) - np.asarray(v, dtype=F32)).astype(F32)
        q = (d * d).astype(F32).astype(np.float64).sum(axis=1).astype(F32)
        return np.sqrt(q)


def centered_clip_ref(x, v, tau, L, factors=None):
    """``L`` iterations from centre ``v``. Returns (centre, distances [L, K], factors [L, K]).
    ``factors`` [L, K] given: those drive the folds (distances are then the stand-in's, for
    information). Otherwise the factors come from ``stand_in_norms``."""
    x = np.asarray(x, dtype=F32)
    v = np.asarray(v, dtype=F32).copy()
    K = x.shape[0]
    dist, fac = np.empty((L, K), dtype=F32), np.empty((L, K), dtype=F32)
    for l in range(L):
        dist[l] = stand_in_norms(x, v)
        fac[l] = clip_factors_ref(dist[l], tau) if factors is None else np.asarray(factors, dtype=F32)[l]
        v = centered_fold_ref(x, v, fac[l])
    return v, dist, fac


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)
