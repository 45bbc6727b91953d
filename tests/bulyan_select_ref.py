"""numpy restatement of Bulyan's first stage on the device (include/fjagg.h: fjagg_bulyan_select),
written from the header's semantics block, not from fjselect_dev.h, and the Gram matrices the
tests feed it with. Every step sorts the remaining distances afresh; every score is added one
neighbour at a time, in ascending order, from 0.0."""
import numpy as np

F64 = np.float64
F32 = np.float32
KFS = [(3, 0), (7, 1), (23, 3), (43, 5), (83, 9), (160, 16), (252, 62)]


def sq_distances(G):
    """d2(i,j) = fl(fl(G_ii + G_jj) - fl(2 G_ij)); finite: max(d2, +0), else +inf; +inf when either
    client is unusable. The diagonal is never used."""
    G = np.asarray(G, F64)
    K = G.shape[0]
    ok = np.array([bool(np.isfinite(G[k, k])) for k in range(K)])
    d2 = np.full((K, K), np.inf, F64)
    with np.errstate(all="ignore"):
        for i in range(K):
            if not ok[i]:
                continue
            v = (G[i, i] + np.diagonal(G)) - F64(2.0) * G[i]
            for j in range(K):
                if ok[j] and np.isfinite(v[j]):
                    d2[i, j] = v[j] if v[j] > 0 else 0.0
    return ok, d2


def select(G, f):
    """(selected[theta] -1 padded, count, step_scores[theta] +inf padded, keep, scale, rows[theta])."""
    G = np.asarray(G, F64)
    K = G.shape[0]
    theta = K - 2 * f
    ok, d2 = sq_distances(G)
    R = [k for k in range(K) if ok[k]]
    picked, won = [], []
    for _ in range(theta):
        n = len(R)
        if n == 0:
            break
        c = max(n - f - 2, 1)
        scores = np.zeros(n, F64)
        if n > 1:
            sub = d2[np.ix_(R, R)]
            others = sub[~np.eye(n, dtype=bool)].reshape(n, n - 1)  # row i without d2(i, i)
            nearest = np.sort(others, axis=1)[:, :c]
            for t in range(c):  # ascending, one addition per neighbour
                scores = scores + nearest[:, t]
        best = None
        for r in range(n):  # R is ascending: the first strict minimum is the lower index
            if np.isfinite(scores[r]) and (best is None or scores[r] < scores[best]):
                best = r
        if best is None:
            break
        picked.append(R[best])
        won.append(scores[best])
        del R[best]
    count = len(picked)
    selected = np.full(theta, -1, np.int64)
    selected[:count] = picked
    step_scores = np.full(theta, np.inf, F64)
    step_scores[:count] = won
    keep = count - 2 * f if count - 2 * f >= 1 else 0
    scale = np.array([F32(1.0 / float(keep)) if keep > 0 else F32(0)], F32)
    rows = np.zeros(theta, np.int32)
    if count:
        rows[:count] = sorted(picked)
        rows[count:] = max(picked)
    return selected, count, step_scores, keep, scale, rows


# ------------------------------------------------------------------------------ the inputs
def gram_of(x):
    """float64 Gram of float32 rows (exact products, numpy's sum): symmetric bit for bit."""
    x = np.asarray(x, F32).astype(F64)
    G = x @ x.T
    return np.triu(G) + np.triu(G, 1).T


def rows_of(rng, K, kind, P=24):
    if kind == "integer":  # small integers: every inner product is exact, ties are common
        return rng.randint(-8, 9, (K, P)).astype(F32)
    return rng.standard_normal((K, P)).astype(F32)


def poison(G, bad):
    """G with the clients `bad` unusable: inf and NaN diagonals in turn."""
    G = G.copy()
    for n, k in enumerate(bad):
        G[k, k] = np.inf if n % 2 == 0 else np.nan
    return G


def inputs(rng, K, f, kind):
    """name -> (Gram matrix, expected count): full, all-tie, short, too short and empty selections."""
    x = rows_of(rng, K, kind)
    G = gram_of(x)
    theta = K - 2 * f
    out = {"base": (G, theta)}
    out["duplicated"] = (gram_of(x[np.arange(K) // 2]), theta)  # every client twice: all ties
    spread = rng.permutation(K)
    if f > 0:
        out["unusable_2f"] = (poison(G, spread[: 2 * f]), theta)  # u <= 2f: a full selection
    u = 2 * f + 1  # u > 2f: a short one
    out["short"] = (poison(G, spread[:u]), K - u)
    u = K - 2 * f  # 2f usable: count < 2f + 1, no mean
    out["too_short"] = (poison(G, spread[:u]), 2 * f)
    out["all_unusable"] = (poison(G, np.arange(K)), 0)
    return out


def permuted(G, perm):
    """The Gram of the clients in the order perm (client i is the old perm[i]): the same bits."""
    return np.ascontiguousarray(G[np.ix_(perm, perm)])
