"""FLTrust (Cao, Fang, Liu and Gong, NDSS 2021) restated in numpy from the contract of
include/fjagg.h alone; nothing here comes from the product. The clients are a list of leaves, leaf l
a float32 array ``[K, n_l]`` (row k is client k's leaf), the server delta a list of float32 arrays
``[n_l]``.

Pass 1 (float32, no FMA): ``a_k = sum fl(x_k[p] g[p])`` and ``q_k = sum fl(x_k[p]^2)`` in
``fjagg_l2sq_rows``' order — leaf by leaf, in 64 Ki-element blocks; lane t of 256 adds elements
t, t + 256, ... ascending from +0; the xor butterfly 32 .. 1 over the 64 lanes of a wave; the four
wave sums in order; the block partials in leaf / block order from +0. ``product_order_sums`` is
that order over any element-wise product (``tests/clipped_mean_ref.l2sq_rows_ref`` with ``x g`` in
place of ``x^2``), for all K rows at once.

Selection (float64, one rounding per operation) and pass 2 (the grouped fold) as ``select`` and
``fold`` state them. A NaN cosine or norm is the quiet NaN numpy's ``nan`` is
(0x7ff8000000000000 / 0x7fc00000)."""
import numpy as np

F32, F64 = np.float32, np.float64
BLOCK = 65536


def _block_sums(prod):
    """[K] float32: every row of ``prod`` [K, m <= 64 Ki] added as one workgroup of 256 lanes does."""
    K, m = prod.shape
    pad = (m + 255) // 256 * 256
    buf = np.zeros((K, pad), dtype=F32)  # (+0 where a lane has no element: adding it changes nothing)
    buf[:, :m] = prod
    acc = np.zeros((K, 256), dtype=F32)
    for i in range(pad // 256):
        acc = acc + buf[:, i * 256:(i + 1) * 256]
    w = acc.reshape(K, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, np.arange(64) ^ o]
    t = w[:, 0, 0]
    for i in range(1, 4):
        t = t + w[:, i, 0]
    return t


def product_order_sums(xs, ys):
    """[K] float32 ``sum fl(x y)`` over the leaves ``xs`` ([K, n_l] each) and ``ys`` ([n_l] or [K, n_l])
    in the library's order."""
    K = xs[0].shape[0]
    s = np.zeros(K, dtype=F32)
    with np.errstate(all="ignore"):
        for x, y in zip(xs, ys):
            x = np.asarray(x, dtype=F32).reshape(K, -1)
            y = np.asarray(y, dtype=F32)
            y = y.reshape(1, -1) if y.size == x.shape[1] else y.reshape(K, -1)
            for b0 in range(0, max(x.shape[1], 1), BLOCK):
                s = s + _block_sums(x[:, b0:b0 + BLOCK] * y[:, b0:b0 + BLOCK])
    return s


def sums(xs, gs):
    """(a [K], q [K], q_s) of pass 1."""
    a = product_order_sums(xs, gs)
    q = product_order_sums(xs, xs)
    g_rows = [np.asarray(g, dtype=F32).reshape(1, -1) for g in gs]
    return a, q, product_order_sums(g_rows, g_rows)[0]


def sequential_dot(x, g):
    """``sum fl(x[p] g[p])`` added one element after the other from +0: ANOTHER order, to tell the
    library's apart from."""
    s = F32(0)
    for v in np.asarray(x, dtype=F32) * np.asarray(g, dtype=F32):
        s = s + v
    return s


def select(a, q, qs):
    """The selection rule over float32 ``a[K]``, ``q[K]`` and ``q_s``: a dict of ``cos`` / ``trust``
    (float64 [K]), ``factors`` / ``norms`` (float32 [K]), ``server_norm``, ``total``, ``count``,
    ``order`` (int32 [K], 0 padded), ``seg``, ``wperm`` (float32 [K], 0 padded) and ``gscale``."""
    a, q = np.asarray(a, dtype=F32), np.asarray(q, dtype=F32)
    K = a.size
    with np.errstate(all="ignore"):
        nk = np.sqrt(q.astype(F64))
        ns = np.sqrt(F64(F32(qs)))
        cos = a.astype(F64) / (nk * ns)
        ts = np.where(cos > 0, np.minimum(cos, 1.0), 0.0)
        c = np.where(ts > 0, ((ts * ns) / nk).astype(F32), F32(0)).astype(F32)
        ok = np.isfinite(c) & (c > 0)
        c = np.where(ok, c, F32(0)).astype(F32)
        ts = np.where(ok, ts, 0.0)
        norms = nk.astype(F32)
        server_norm = F32(ns)
    T = F64(0.0)
    for t in ts:
        T = T + t
    members = np.flatnonzero(c > 0).astype(np.int32)
    order = np.zeros(K, dtype=np.int32)
    wperm = np.zeros(K, dtype=F32)
    order[:members.size] = members
    wperm[:members.size] = c[members]
    return dict(cos=np.where(np.isnan(cos), np.nan, cos), trust=ts, factors=c,
                norms=np.where(np.isnan(norms), F32(np.nan), norms).astype(F32),
                server_norm=F32(np.nan) if np.isnan(server_norm) else server_norm, total=T,
                count=np.int32(members.size), order=order, seg=np.array([0, members.size], dtype=np.int32),
                wperm=wperm, gscale=F32(1.0 / T) if T > 0 else F32(0))


def fold(xs, sel):
    """Pass 2: per element ``s = +0; s = fl(s + fl(x_m c_m))`` over the members in order, ``y = fl(s r)``;
    all +0 when the table is empty. A client that is not a member is never touched. (Element-wise,
    so the leaves are folded side by side as one row and cut apart again.)"""
    K = np.asarray(xs[0]).shape[0]
    rows = np.concatenate([np.asarray(x, dtype=F32).reshape(K, -1) for x in xs], axis=1)
    count, r = int(sel["count"]), sel["gscale"]
    s = np.zeros(rows.shape[1], dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(count):
            s = s + rows[sel["order"][j]] * sel["wperm"][j]
        if count:
            s = s * r
    offs = np.concatenate([[0], np.cumsum([np.asarray(x).reshape(K, -1).shape[1] for x in xs])])
    return [s[offs[l]:offs[l + 1]].reshape(np.asarray(x).shape[1:]) for l, x in enumerate(xs)]


def fltrust(xs, gs):
    """The whole round: ``select``'s dict plus ``a``, ``q``, ``qs`` and ``mean`` (a list of leaves)."""
    a, q, qs = sums(xs, gs)
    sel = select(a, q, qs)
    sel.update(a=a, q=q, qs=qs, mean=fold(xs, sel))
    return sel
