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
every step below is the contract's rounding. That includes the ORDER in which the library adds the
squares: ``clipped_mean_ref.l2sq_rows_ref`` restates ``fjagg_l2sq_rows``' summation (leaf by leaf,
64 Ki-element blocks, 256 lanes striding the block, the xor shuffle tree, the four wave sums, the
block partials in order), and the centred norm pass is that summation applied to ``fl(x - v)``:
``centered_l2sq_ref`` for one client, ``centered_distances_ref`` for all K rows at once (the same
additions, vectorised over the clients). ``centered_clip_ref(x, v, tau, L, sizes=...)`` is
therefore a closed computation of a whole round, distances, factors and centre, with nothing
taken from the code under test; a row given whole is the one-leaf case ``sizes=[P]``. Without
``sizes`` and ``factors`` q comes from a float64 sum rounded once — a stand-in, within 2e-6 of
any float32 order, kept for the CPU tests of the rule itself; with ``factors`` those drive the
folds.
"""
import numpy as np

from tests.clipped_mean_ref import clip_factors_ref, l2sq_rows_ref

F32 = np.float32
NORM_BLOCK = 65536  # elements per norm block (fjagg_l2sq_rows' partition)


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


def centered_l2sq_ref(leaves_x, leaves_v):
    """q of ONE client: ``l2sq_rows_ref``'s summation applied to fl(x - v), leaf by leaf (a leaf of
    no elements adds +0). ``leaves_x`` / ``leaves_v``: the client's and the centre's leaves."""
    with np.errstate(all="ignore"):
        return l2sq_rows_ref([(np.asarray(a, dtype=F32).reshape(-1) - np.asarray(b, dtype=F32).reshape(-1)).astype(F32)
                              for a, b in zip(leaves_x, leaves_v)])


def centered_l2sq_rows_ref(x, v, sizes, wave_order=(0, 1, 2, 3)):
    """``centered_l2sq_ref`` of every row of ``x`` [K, P] cut into leaves of ``sizes``: float32 [K].
    The same additions in the same order, each made for all K clients at once. ``wave_order``
    other than the library's (0, 1, 2, 3) gives a WRONG sum on purpose: a test uses it to show
    that its data tells the orders apart."""
    x = np.asarray(x, dtype=F32)
    v = np.asarray(v, dtype=F32)
    K, P = x.shape
    assert sum(sizes) == P and v.shape == (P,)
    s = np.zeros(K, dtype=F32)
    o = 0
    with np.errstate(all="ignore"):
        for n in sizes:
            d = (x[:, o:o + n] - v[o:o + n]).astype(F32)
            o += n
            for b0 in range(0, max(n, 1), NORM_BLOCK):
                sq = (d[:, b0:b0 + NORM_BLOCK] * d[:, b0:b0 + NORM_BLOCK]).astype(F32)
                m, full = sq.shape[1], sq.shape[1] // 256
                acc = np.zeros((K, 256), dtype=F32)  # lane t: elements t, t + 256, ... in order from +0
                body = sq[:, :full * 256].reshape(K, full, 256)
                for j in range(full):
                    acc = acc + body[:, j]
                if m % 256:  # (a lane with no element left adds nothing: its sum is never -0)
                    acc[:, :m % 256] = acc[:, :m % 256] + sq[:, full * 256:]
                w = acc.reshape(K, 4, 64)
                for step in (32, 16, 8, 4, 2, 1):  # the xor shuffle tree of a wave: lane i adds lane i ^ step
                    pairs = w.reshape(K, 4, 32 // step, 2, step)
                    w = (pairs + pairs[:, :, :, ::-1, :]).reshape(K, 4, 64)
                t = w[:, wave_order[0], 0]
                for i in wave_order[1:]:  # the four wave sums in order
                    t = t + w[:, i, 0]
                s = s + t  # the block partials in leaf / block order from +0
    return s


def centered_distances_ref(x, v, sizes):
    """n_k = the float32 ``sqrt`` of ``centered_l2sq_rows_ref``: the library's distances, bit for bit."""
    with np.errstate(all="ignore"):
        return np.sqrt(centered_l2sq_rows_ref(x, v, sizes))


def centered_clip_ref(x, v, tau, L, factors=None, sizes=None):
    """``L`` iterations from centre ``v``. Returns (centre, distances [L, K], factors [L, K]).
    ``sizes`` (the row's leaf sizes; ``[P]`` for a row taken whole) given: the closed round, the
    distances ``centered_distances_ref``'s and the factors from them. ``factors`` [L, K] given:
    those drive the folds (distances are then the stand-in's, for information). Neither: the
    factors come from ``stand_in_norms``."""
    x = np.asarray(x, dtype=F32)
    v = np.asarray(v, dtype=F32).copy()
    K = x.shape[0]
    assert factors is None or sizes is None
    dist, fac = np.empty((L, K), dtype=F32), np.empty((L, K), dtype=F32)
    for l in range(L):
        dist[l] = stand_in_norms(x, v) if sizes is None else centered_distances_ref(x, v, sizes)
        fac[l] = clip_factors_ref(dist[l], tau) if factors is None else np.asarray(factors, dtype=F32)[l]
        v = centered_fold_ref(x, v, fac[l])
    return v, dist, fac


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)
