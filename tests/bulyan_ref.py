"""Restatement of Bulyan (El Mhamdi, Guerraoui and Rouault, ICML 2018) on the client
VECTORS in float64 — no Gram matrix anywhere: the brute-force iterated-Krum selection, then the
mean around the median (tests/around_median_ref.py) over the selected rows. Nothing here calls
the product.

Selection, with f Byzantine clients and theta = K - 2f: R = the usable clients; up to theta
times, with n = |R| and c = max(n - f - 2, 1), score_i = the c smallest |x_i - x_j|^2, j in
R \\ {i}, added in ascending order from 0.0 (0.0 when n = 1); the smallest finite score, ties to
the lower index, is selected and leaves R. The round's mean is the mean around the median of the
rows sorted(S) with keep = |S| - 2f, or None when that is below 1.

A client is usable when its squared norm is finite IN FLOAT32, as the Gram pass forms it: a
row holding NaN, inf or 1e30 is not (1e30^2 overflows float32)."""
import numpy as np

from tests import around_median_ref as am
from tests import robust_select_ref as sel

F32 = np.float32


def usable(x) -> np.ndarray:
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        return np.isfinite((x.astype(np.float64) ** 2).sum(axis=1).astype(F32)) & np.isfinite(x).all(axis=1)


def distances(x) -> np.ndarray:
    """float64 [K, K] squared distances of the rows, from the differences (no inner products)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((x - x[i][None, :]) ** 2).sum(axis=1) for i in range(x.shape[0])])


def select(x, f, with_gaps=False):
    """int64 indices in selection order; with_gaps: also, per pick, the second-best finite score
    minus the best (inf when there is no second)."""
    x = np.asarray(x, dtype=F32)
    K = x.shape[0]
    if K < 4 * f + 3:
        raise ValueError("K >= 4f + 3")
    D = distances(x)
    R = [int(k) for k in np.flatnonzero(usable(x))]
    S, gaps = [], []
    for _ in range(K - 2 * f):
        if not R:
            break
        c = max(len(R) - f - 2, 1)
        scores = []
        for i in R:
            s = 0.0
            for v in np.sort(D[i, [j for j in R if j != i]])[:c].tolist():
                s += v
            scores.append(s)
        finite = sorted((s, i) for s, i in zip(scores, R) if np.isfinite(s))
        if not finite:
            break
        S.append(finite[0][1])
        gaps.append(finite[1][0] - finite[0][0] if len(finite) > 1 else np.inf)
        R.remove(finite[0][1])
    S = np.array(S, dtype=np.int64)
    return (S, np.array(gaps)) if with_gaps else S


def bulyan(x, f):
    """(mean float32 [P] or None, selected, keep)."""
    x = np.asarray(x, dtype=F32)
    S = select(x, f)
    keep = len(S) - 2 * f
    if keep < 1:
        return None, S, 0
    return am.mean_around_median(x[np.sort(S)], keep), S, keep


def small_ints(rng: np.random.RandomState, K: int, P: int) -> np.ndarray:
    """Integers in [-8, 8] as float32: every inner product and every float32 chain of the Gram
    pass is exact, so the Gram routes agree bit for bit and equal the float64 products."""
    return rng.randint(-8, 9, (K, P)).astype(F32)


def poison(rng: np.random.RandomState, x: np.ndarray, count: int):
    """``count`` rows at random filled with NaN, inf or 1e30 (one kind per row). Returns the rows."""
    rows = np.sort(rng.choice(x.shape[0], size=count, replace=False))
    for n, r in enumerate(rows):
        x[r] = [np.nan, np.inf, 1e30][(n + int(rows[0])) % 3]
    return rows


SELECT_CASES = ((3, 0), (7, 1), (11, 2), (23, 5), (64, 15), (160, 16))
ROUND_CASES = ((7, 1, 257), (23, 5, 1000), (64, 15, 515), (160, 16, 2049))  # (K, f, P)
# N(0, 1) rounds: (K, f, P, seed) candidates; the tests keep those whose every pick is separated
# by more than 2 E (robust_select_ref.krum_error_bound) and need at least 6 of them. f >= 3 only:
# with f <= 2 the last steps score a client by its ONE nearest neighbour, the two closest clients
# then tie exactly (d2 is symmetric), and the gap at that pick is 0 whatever the data
NORMAL_CANDIDATES = tuple((K, f, P, seed) for K, f, P in ((15, 3, 515), (19, 4, 300), (23, 5, 130), (31, 7, 257))
                          for seed in (0, 1, 2))


def normal_round(K, f, P, seed) -> np.ndarray:
    return np.random.RandomState(7000 + 100 * K + seed).standard_normal((K, P)).astype(F32)


def separated_normal_cases():
    """The NORMAL_CANDIDATES whose selection cannot depend on the Gram's rounding: at every pick
    the best true score is more than 2 E below the next. E bounds the error of a sum of up to
    K - f - 2 distances from any Gram within the library's bound; Bulyan's steps add at most that
    many, over a subset of the clients, so the same E covers every step."""
    out = []
    for K, f, P, seed in NORMAL_CANDIDATES:
        x = normal_round(K, f, P, seed)
        _, gaps = select(x, f, with_gaps=True)
        if len(gaps) == K - 2 * f and gaps.min() > 2 * sel.krum_error_bound(x, f):
            out.append((K, f, P, seed))
    return out
