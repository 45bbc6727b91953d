"""Host-side selection for the whole-vector Byzantine-robust aggregates, on the K x K Gram
matrix ``G[i][j] = <x_i, x_j>`` of the client deltas (numpy float64; no GPU, no torch).

* Krum / multi-Krum — Blanchard, El Mhamdi, Guerraoui and Stainer, "Machine Learning with
  Adversaries: Byzantine Tolerant Gradient Descent", NeurIPS 2017: the client(s) whose delta is
  closest to its ``K - f - 2`` nearest neighbours. Needs ``d2(i, j) = G_ii + G_jj - 2 G_ij``.
* Bulyan's selection — El Mhamdi, Guerraoui and Rouault, "The Hidden Vulnerability of Distributed
  Learning in Byzantium", ICML 2018: Krum iterated ``K - 2f`` times on the shrinking set of
  clients not yet chosen. The coordinate-wise second stage is the mean around the median
  (``fjagg_meamed_*``) over the chosen clients.
* The geometric median by the smoothed Weiszfeld algorithm ("RFA") — Pillutla, Kakade and
  Harchaoui, "Robust Aggregation for Federated Learning", IEEE Trans. Signal Processing 2022.
  Every iterate is ``v = sum_j a_j x_j``, so ``|v - x_k|^2 = a'Ga - 2 (Ga)_k + G_kk``: all
  iterations run on K x K numbers and only the final weights ``a`` go back to the device.

The Gram matrix comes from :func:`fedjax_amd.kernels.gram_dense` / ``gram_ptrs`` (one pass over
the deltas); the result is one grouped fold over the chosen or re-weighted clients. A client
with a non-finite value anywhere in its delta has a non-finite ``G[k][k]``: it is *unusable*,
never selected, and gets weight 0 — the callers give it group id -1, so the fold never loads it.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np

__all__ = ["usable", "sq_distances", "krum_scores", "krum_select", "check_krum_args", "bulyan_select",
           "weiszfeld_weights", "bucket_gram", "bucket_members"]


def _gram(G) -> np.ndarray:
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1:
        raise ValueError(f"G must be a square [K, K] matrix with K >= 1, got shape {G.shape}")
    return G


def _int(name: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an int, not {type(v).__name__}")
    return int(v)


def usable(G) -> np.ndarray:
    """bool[K]: client k is usable iff ``G[k][k]`` is finite (its delta holds no NaN or inf, and
    its squared norm did not overflow)."""
    return np.isfinite(np.diagonal(_gram(G)))


def sq_distances(G) -> np.ndarray:
    """float64[K, K] squared distances ``max(G_ii + G_jj - 2 G_ij, 0)``, 0 on the diagonal, and
    ``+inf`` wherever either client is unusable or the value is not finite."""
    G = _gram(G)
    ok = usable(G)
    d = np.diagonal(G)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (d[:, None] + d[None, :]) - 2.0 * G
        d2 = np.where(np.isfinite(d2), np.maximum(d2, 0.0), np.inf)
    d2[~ok, :] = np.inf
    d2[:, ~ok] = np.inf
    np.fill_diagonal(d2, 0.0)
    return d2


def _check_krum(K: int, f) -> int:
    f = _int("num_byzantine", f)
    if f < 0:
        raise ValueError(f"num_byzantine must be >= 0, got {f}")
    if K < 2 * f + 3:
        raise ValueError(f"Krum needs K >= 2f + 3 clients: K = {K}, f = {f}")
    return f


def krum_scores(G, f) -> np.ndarray:
    """float64[K] Krum scores: ``score_i`` is the sum of the ``K - f - 2`` smallest ``d2(i, j)``,
    ``j != i``, added in ascending order; ``+inf`` for an unusable client (and for one with too
    few usable neighbours). Needs ``K >= 2f + 3`` and an int ``f >= 0`` (a bool is refused)."""
    G = _gram(G)
    K = G.shape[0]
    f = _check_krum(K, f)
    d2 = sq_distances(G)
    ok = usable(G)
    others = d2[~np.eye(K, dtype=bool)].reshape(K, K - 1)  # row i without d2(i, i)
    nearest = np.sort(others, axis=1)[:, : K - f - 2]
    scores = np.zeros(K, dtype=np.float64)
    for c in range(nearest.shape[1]):  # ascending, one addition per neighbour
        scores = scores + nearest[:, c]
    scores[~ok] = np.inf
    return scores


def krum_select(G, f, m=1) -> np.ndarray:
    """int64 indices of the ``m`` clients of smallest finite Krum score, best first, ties to the
    lower index (``m = 1``: Krum; ``m > 1``: multi-Krum). ``1 <= m <= K - f``. With fewer than
    ``m`` finite scores, those there are; with none, an empty selection."""
    G = _gram(G)
    K = G.shape[0]
    f = _check_krum(K, f)
    m = _int("num_selected", m)
    if not (1 <= m <= K - f):
        raise ValueError(f"num_selected must be in [1, K - f] = [1, {K - f}], got {m}")
    scores = krum_scores(G, f)
    order = np.argsort(scores, kind="stable")
    order = order[np.isfinite(scores[order])]
    return order[:m].astype(np.int64)


def check_krum_args(K: int, f, m) -> Tuple[int, int]:
    """:func:`krum_select`'s conditions on the client count alone, with its exceptions and
    nothing computed: int ``f >= 0`` and ``m`` (a bool is refused), ``K >= 2f + 3``,
    ``1 <= m <= K - f``. Returns ``(f, m)``."""
    f = _check_krum(K, f)
    m = _int("num_selected", m)
    if not (1 <= m <= K - f):
        raise ValueError(f"num_selected must be in [1, K - f] = [1, {K - f}], got {m}")
    return f, m


def check_bulyan(K: int, f) -> int:
    """Bulyan's conditions on the client count alone: an int ``f >= 0`` (a bool is refused) and
    ``K >= 4f + 3``. Returns ``f``."""
    f = _int("num_byzantine", f)
    if f < 0:
        raise ValueError(f"num_byzantine must be >= 0, got {f}")
    if K < 4 * f + 3:
        raise ValueError(f"Bulyan needs K >= 4f + 3 clients: K = {K}, f = {f}")
    return f


def bulyan_select(G, f) -> np.ndarray:
    """int64 indices of Bulyan's first stage, in selection order: ``theta = K - 2f`` times, the
    client of smallest Krum score among the set ``R`` of usable clients not yet chosen, which
    then leaves ``R``. Needs ``K >= 4f + 3`` and an int ``f >= 0`` (a bool is refused).

    With ``n = |R|``, ``score_i`` is the sum of the ``c = max(n - f - 2, 1)`` smallest ``d2(i, j)``,
    ``j`` in ``R`` without ``i``, added in ascending order from 0.0 (0.0 when ``n = 1``); the
    smallest FINITE score wins, ties to the lower index; with no finite score the selection stops
    short. The paper applies Krum to the remaining set unchanged, whose neighbour count ``n - f - 2``
    falls below 1 on the last steps (Krum itself wants ``n >= 2f + 3``, and the set shrinks to
    ``2f + 1``); the clamp at one neighbour is this project's decision. With every client usable
    the first pick is ``krum_select(G, f, 1)[0]``.

    Every row's neighbours are sorted once (by distance, then index); a step takes each
    remaining row's first ``c`` remaining neighbours in that order, so the sums are those of a
    fresh sort per step."""
    G = _gram(G)
    K = G.shape[0]
    f = check_bulyan(K, f)
    d2 = sq_distances(G)
    alive = usable(G).copy()
    order = np.argsort(d2, axis=1, kind="stable")  # row i: its neighbours, nearest first
    near = np.take_along_axis(d2, order, axis=1)
    not_self = order != np.arange(K)[:, None]
    selected = []
    for _ in range(K - 2 * f):
        rows = np.flatnonzero(alive)  # R, ascending
        if rows.size == 0:
            break
        c = max(rows.size - f - 2, 1)
        cand = alive[order[rows]] & not_self[rows]
        take = cand & (np.cumsum(cand, axis=1) <= c)
        # zeros between the taken terms leave a sequential sum of non-negative terms unchanged
        scores = np.cumsum(np.where(take, near[rows], 0.0), axis=1)[:, -1]
        best = int(np.argmin(scores))  # the first minimum: ties to the lower index
        if not np.isfinite(scores[best]):
            break
        selected.append(int(rows[best]))
        alive[rows[best]] = False
    return np.array(selected, dtype=np.int64)


def _bucket_table(K: int, bucket_size, perm) -> Tuple[int, int, np.ndarray]:
    """(s, B, table) of ``K`` clients in buckets of ``bucket_size`` by ``perm`` (None: the identity),
    checked: an int ``bucket_size >= 1`` (a bool is refused; above ``K`` it is ``K``) and a
    permutation of ``range(K)``."""
    s = _int("bucket_size", bucket_size)
    if s < 1:
        raise ValueError(f"bucket_size must be >= 1, got {s}")
    s = min(s, K)
    if perm is None:
        table = np.arange(K, dtype=np.int64)
    else:
        table = np.asarray(perm)
        if table.dtype == np.bool_ or table.dtype.kind not in "iu":
            raise TypeError(f"perm must hold ints, got dtype {table.dtype}")
        table = table.astype(np.int64)
        if table.ndim != 1 or table.size != K or not np.array_equal(np.sort(table), np.arange(K)):
            raise ValueError(f"perm must be a permutation of range({K})")
    return s, -(-K // s), table


def bucket_members(K: int, bucket_size, perm=None) -> list:
    """The member clients of every bucket, in table order: ``B`` int64 arrays, bucket ``j`` holding
    ``perm[j*s : min((j+1)*s, K)]``. Only the last can be short. ``np.concatenate`` of the entries
    a bucketed Krum selected gives the clients whose deltas were averaged."""
    s, B, table = _bucket_table(int(K), bucket_size, perm)
    return [table[j * s:min((j + 1) * s, K)] for j in range(B)]


def bucket_gram(G, bucket_size, perm=None) -> np.ndarray:
    """float64 [B, B] Gram matrix of the bucket means of bucketing (Karimireddy, He and Jaggi, ICLR
    2022) from the clients' ``G`` alone, with no pass over the deltas: with bucket ``a`` holding
    the ``n_a`` clients ``perm[a*s + i]`` (:func:`bucket_members`),

        Gb[a][b] = (sum_{i in a} sum_{j in b} G[i][j]) / (n_a * n_b)

    The ``n_a * n_b`` terms are added sequentially as ONE chain in table order, rows first: the
    first term verbatim, then for each member ``i`` of ``a`` in turn every member ``j`` of ``b``;
    then one division by the float64 ``n_a * n_b``. ``bucket_size = 1`` with the identity table
    returns ``G`` bit for bit. A client holding a NaN or inf has a non-finite row and column in
    ``G`` and makes exactly its bucket's row and column of ``Gb`` non-finite; any client with a
    non-finite ``G[k][k]`` makes its bucket's diagonal entry non-finite, so the bucket is unusable
    (:func:`usable`) and is never selected."""
    G = _gram(G)
    K = G.shape[0]
    s, B, table = _bucket_table(K, bucket_size, perm)
    Gp = G[np.ix_(table, table)]
    full, n_last = (K // s, 0) if K % s == 0 else (K // s, K % s)
    out = np.empty((B, B), dtype=np.float64)

    def block(r0, cnt_r, nr, c0, cnt_c, nc):  # cnt_r x cnt_c buckets of nr x nc clients: each one chain
        blk = Gp[r0:r0 + cnt_r * nr, c0:c0 + cnt_c * nc].reshape(cnt_r, nr, cnt_c, nc)
        chain = np.ascontiguousarray(blk.transpose(0, 2, 1, 3)).reshape(cnt_r, cnt_c, nr * nc)
        return np.cumsum(chain, axis=-1)[..., -1] / float(nr * nc)  # cumsum adds strictly left to right

    with np.errstate(invalid="ignore", over="ignore"):
        out[:full, :full] = block(0, full, s, 0, full, s)
        if n_last:
            e = full * s
            out[:full, full:] = block(0, full, s, e, 1, n_last)
            out[full:, :full] = block(e, 1, n_last, 0, full, s)
            out[full:, full:] = block(e, 1, n_last, e, 1, n_last)
    return out


def weiszfeld_weights(G, alpha=None, nu: float = 1e-6, iterations: int = 4) -> Tuple[np.ndarray, np.ndarray]:
    """The smoothed Weiszfeld iteration on the usable sub-matrix of ``G``. ``alpha``: positive
    finite client weights (default: all 1). With ``a = alpha / sum(alpha)``, ``iterations`` times

        d_k = sqrt(max(a'Ga - 2 (Ga)_k + G_kk, 0));  beta_k = alpha_k / max(nu, d_k);  a = beta / sum(beta)

    Returns ``(a, d)``, both float64[K]: the final weights, summing to 1 over the usable clients
    and 0 for the others, and the last distances (``d`` is zeros with ``iterations = 0`` and
    ``inf`` for unusable clients). No usable client: all-zero weights."""
    G = _gram(G)
    K = G.shape[0]
    iterations = _int("iterations", iterations)
    if iterations < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations}")
    if isinstance(nu, (bool, np.bool_)) or not isinstance(nu, (int, float, np.integer, np.floating)):
        raise TypeError("nu must be a number")
    nu = float(nu)
    if not (nu > 0.0 and np.isfinite(nu)):
        raise ValueError(f"nu must be finite and > 0, got {nu}")
    if alpha is None:
        alpha = np.ones(K, dtype=np.float64)
    alpha = np.asarray(alpha)
    if alpha.dtype == np.bool_:
        raise TypeError("weights must be numbers, not bools")
    alpha = alpha.astype(np.float64)
    if alpha.shape != (K,):
        raise ValueError(f"need {K} weights, got shape {alpha.shape}")
    if not (np.isfinite(alpha).all() and (alpha > 0.0).all()):
        raise ValueError("weights must be finite and > 0")
    ok = usable(G)
    a_full = np.zeros(K, dtype=np.float64)
    d_full = np.where(ok, 0.0, np.inf)
    if not ok.any():
        return a_full, d_full
    idx = np.flatnonzero(ok)
    Gu = G[np.ix_(idx, idx)]
    al = alpha[idx]
    diag = np.diagonal(Gu)
    a = al / al.sum()
    d = np.zeros(len(idx), dtype=np.float64)
    for _ in range(iterations):
        Ga = Gu @ a
        d = np.sqrt(np.maximum(a @ Ga - 2.0 * Ga + diag, 0.0))
        beta = al / np.maximum(nu, d)
        a = beta / beta.sum()
    a_full[idx] = a
    d_full[idx] = d
    return a_full, d_full
