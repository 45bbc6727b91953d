"""numpy restatement of the top-k sparsified mean, written from its contract and not from the
kernels: magnitude keys ``bits & 0x7fffffff`` compared as uint32, the threshold by ``np.sort``,
the mask ``key >= T`` (all ties kept), ``sent = #{key >= max(T, 1)}``, and the mean as the oracle's
``tree_mean`` over the masked arrays. Also the data families the CPU and GPU tests share."""
import numpy as np

from oracle import tree_util_ref as oref

F32 = np.float32
KEY_MASK = np.uint32(0x7FFFFFFF)


def keys(row):
    """Magnitude keys of a float32 array (uint32)."""
    return np.ascontiguousarray(row, dtype=F32).view(np.uint32) & KEY_MASK


def threshold(row, c):
    """The c-th largest key of a flat float32 row: element c - 1 of the keys sorted descending."""
    m = np.sort(keys(np.ravel(row)))[::-1]
    assert 1 <= c <= m.size
    return np.uint32(m[c - 1])


def select(rows, c):
    """(thresholds uint32 [K], sent int32 [K]) of K flat float32 rows."""
    T = np.array([threshold(r, c) for r in rows], dtype=np.uint32)
    sent = np.array([int((keys(np.ravel(r)) >= max(int(t), 1)).sum()) for r, t in zip(rows, T)], dtype=np.int32)
    return T, sent


def select_many(rows, cs):
    """{c: (thresholds, sent)} for several keep counts, each row sorted once (np.sort, ascending:
    the c-th largest is element P - c; the keys >= t are those from searchsorted's left edge)."""
    out = {c: (np.zeros(len(rows), np.uint32), np.zeros(len(rows), np.int32)) for c in cs}
    for k, r in enumerate(rows):
        m = np.sort(keys(np.ravel(r)))
        for c in cs:
            assert 1 <= c <= m.size
            t = m[m.size - c]
            out[c][0][k] = t
            out[c][1][k] = m.size - np.searchsorted(m, max(int(t), 1), side="left")
    return out


def mask_row(row, T):
    """x~ = kept ? x : +0 (a kept -0 passes verbatim)."""
    row = np.ascontiguousarray(row, dtype=F32)
    return np.where(keys(row) >= np.uint32(T), row, F32(0.0)).astype(F32)


def flat_row(leaves):
    """A client's row: its leaves concatenated in leaf order."""
    return np.concatenate([np.ravel(np.asarray(x, dtype=F32)) for x in leaves]) if leaves else np.zeros(0, F32)


def topk_mean_rows(rows, weights, c):
    """(mean float32 [P], thresholds, sent) of K flat rows: the oracle's tree_mean over the masked rows."""
    T, sent = select(rows, c)
    masked = [mask_row(r, t) for r, t in zip(rows, T)]
    with np.errstate(all="ignore"):
        mean = oref.tree_mean([({"x": m}, w) for m, w in zip(masked, weights)])["x"]
    return np.asarray(mean, dtype=F32), T, sent


def topk_mean_trees(trees, weights, c):
    """(mean pytree, thresholds, sent) of K client pytrees (dicts of float32 arrays): one global
    threshold per client over all its leaves (oracle leaf order), then tree_mean over the masked trees."""
    flats = [oref.flatten(t) for t in trees]
    rows = [flat_row(leaves) for leaves, _ in flats]
    T, sent = select(rows, c)
    masked = [oref.unflatten(td, [mask_row(x, t) for x in leaves]) for (leaves, td), t in zip(flats, T)]
    with np.errstate(all="ignore"):
        mean = oref.tree_mean(list(zip(masked, weights)))
    return mean, T, sent


def num_bits(sent_rounds, P):
    """The aggregator's bits over rounds: sum of mean_k(sent_k) * (32 + ceil(log2 P)), in float64."""
    per = 32 + int(np.ceil(np.log2(P))) if P > 1 else 32
    return float(sum(np.mean(np.asarray(s, dtype=np.float64)) * per for s in sent_rounds))


# ------------------------------------------------------------------ data families
FAMILIES = ("gauss", "five", "zeros", "equal", "nan_inf", "subnormal", "signed_zero", "hot_bin", "last_digit",
            "mid_digit", "top_digit")


def family(name, K, P, rng):
    """A float32 [K, P] array of the named family."""
    if name == "gauss":
        x = rng.standard_normal((K, P)).astype(F32) * F32(0.01)
    elif name == "five":  # five distinct magnitudes: ties straddle most ranks
        mags = np.array([0.5, 0.25, 1.0, 2.0, 0.125], F32)
        x = mags[rng.randint(0, 5, (K, P))] * rng.choice(np.array([-1, 1], F32), (K, P))
    elif name == "zeros":
        x = np.zeros((K, P), F32)
    elif name == "equal":
        x = np.full((K, P), F32(-0.375))
    elif name == "nan_inf":
        x = rng.standard_normal((K, P)).astype(F32)
        for k in range(K):
            x[k, rng.randint(0, P)] = np.nan
            x[k, rng.randint(0, P)] = -np.inf if k % 2 else np.inf
    elif name == "subnormal":  # subnormals, zeros and a few normals
        b = rng.randint(0, 1 << 23, (K, P)).astype(np.uint32) | (rng.randint(0, 2, (K, P)).astype(np.uint32) << 31)
        x = b.view(F32).copy()
        x[rng.rand(K, P) < 0.2] = 0.0
        x[rng.rand(K, P) < 0.05] = F32(1e-30)
    elif name == "signed_zero":  # +-0 mixed in: fewer non-zeros than many a keep count
        x = rng.standard_normal((K, P)).astype(F32)
        z = rng.rand(K, P)
        x[z < 0.4] = 0.0
        x[z < 0.2] = -0.0
    elif name == "hot_bin":  # every magnitude in one top-level bin: keys share their top 11 bits
        b = np.uint32(0x3F800000) | rng.randint(0, 1 << 20, (K, P)).astype(np.uint32)
        x = (b | (rng.randint(0, 2, (K, P)).astype(np.uint32) << 31)).view(F32).copy()
    elif name == "last_digit":  # keys differ only in the lowest 10 bits
        x = (np.uint32(0x3F812C00) | rng.randint(0, 1 << 10, (K, P)).astype(np.uint32)).view(F32).copy()
    elif name == "mid_digit":  # keys differ only in the middle digit
        x = (np.uint32(0x3F800155) | (rng.randint(0, 1 << 10, (K, P)).astype(np.uint32) << 10)).view(F32).copy()
    elif name == "top_digit":  # keys differ only in the top digit (NaN and inf patterns included)
        x = (np.uint32(0x000AAAAA & 0xFFFFF) | (rng.randint(0, 1 << 11, (K, P)).astype(np.uint32) << 20)).view(F32).copy()
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, dtype=F32)


def keep_counts(P):
    """The keep counts of the issue for a row of P: {1, 2, P // 10, P - 1, P} within [1, P]."""
    return sorted({c for c in (1, 2, P // 10, P - 1, P) if 1 <= c <= P})
