"""Numpy float32 restatement of the clipped weighted mean (no product code).

The reference clips every client's delta before it weights and adds it
(fedjax/algorithms/mime_lite.py:131-149 with tree_clip_by_global_norm,
fedjax/core/tree_util.py:117-133):

    norm  = sqrt(sum of squares)                 float32
    c     = minimum(1, max_norm / norm)          float32, NaN propagates
    t     = (c * x) * w                          two float32 roundings
    sum   = sum + t                              in client order
    mean  = sum * f32(1 / W)

numpy's float32 ``sqrt``, ``/``, ``*`` and ``+`` are correctly rounded IEEE operations,
so every step below is the reference's rounding.
"""
import numpy as np

F32 = np.float32


def clip_factors_ref(n, C):
    """c = minimum(1, C / n) in float32 for norms ``n``; NaN propagates (np.where, not fmin)."""
    n = np.asarray(n, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (F32(C) / n).astype(F32)
    return np.where(np.isnan(r), r, np.where(r < F32(1), r, F32(1))).astype(F32)


def clip_scales_ref(q, C):
    """(norms, c) of squared norms ``q``: c = minimum(1, C / sqrt(q)) in float32."""
    q = np.asarray(q, dtype=F32)
    with np.errstate(invalid="ignore"):
        n = np.sqrt(q)
    return n, clip_factors_ref(n, C)


def clipped_fold_ref(x, w, c, scale, init=None):
    """sum_k (c_k * x_k) * w_k over the rows of ``x`` [K, P], float32, client by client;
    from ``init`` if given; times ``scale`` if not None."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(w, dtype=F32)
    c = np.asarray(c, dtype=F32)
    s = None if init is None else np.asarray(init, dtype=F32).copy()
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            t = (c[k] * x[k]).astype(F32) * w[k]
            s = t if s is None else (s + t).astype(F32)
        if scale is not None:
            s = (s * F32(scale)).astype(F32)
    return s


def merged_fold_ref(x, w, c, scale):
    """The fold with the factor merged into the weight, x * fl(c * w): NOT the reference's
    rounding (the tests show the two differ)."""
    x = np.asarray(x, dtype=F32)
    cw = (np.asarray(c, dtype=F32) * np.asarray(w, dtype=F32)).astype(F32)
    s = None
    for k in range(x.shape[0]):
        t = (x[k] * cw[k]).astype(F32)
        s = t if s is None else (s + t).astype(F32)
    if scale is not None:
        s = (s * F32(scale)).astype(F32)
    return s


def clipped_products(x, c):
    """fl(c_k * x_k) per client, float32 [K, P]."""
    with np.errstate(all="ignore"):
        return (np.asarray(c, dtype=F32)[:, None] * np.asarray(x, dtype=F32)).astype(F32)


def f64_norms(x):
    """l2 norm of every row of ``x`` in float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt((x * x).sum(axis=1))


def l2sq_rows_ref(leaves):
    """fjagg_l2sq_rows's sum of one client's squares, restated in numpy float32: every leaf in
    64 Ki-element blocks; in a block lane t of 256 adds the squares of elements t, t + 256, ... in
    that order from +0; the 64 lanes of a wave are added by an xor butterfly (32, 16, ... 1), the
    four waves in order; then the block partials in leaf / block order from +0."""
    s = F32(0)
    for a in leaves:
        a = np.asarray(a, dtype=F32).reshape(-1)
        for b0 in range(0, max(a.size, 1), 65536):
            sq = a[b0:b0 + 65536] * a[b0:b0 + 65536]
            m = np.zeros((sq.size + 255) // 256 * 256, dtype=F32)  # (+0 where a lane has no element:
            m[:sq.size] = sq                                        # adding it changes nothing)
            acc = np.zeros(256, dtype=F32)
            for row in m.reshape(-1, 256):
                acc = acc + row
            w = acc.reshape(4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                w = w + w[:, np.arange(64) ^ o]
            t = w[0, 0]
            for i in range(1, 4):
                t = t + w[i, 0]
            s = s + t
    return s


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)
