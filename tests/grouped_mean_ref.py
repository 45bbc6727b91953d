"""Numpy float32 restatement of the grouped weighted mean (no product code).

The reference keeps one running sum per cluster (fedjax/algorithms/hyp_cluster.py:268-303,
``expectation_step``)::

    sums   = [tree_zeros_like(params)] * G ; totals = [0] * G          :278-282
    for each client: c = cluster_ids[client]
        sums[c]   = tree_add(sums[c], tree_weight(delta, n))           :289-291
        totals[c] += n                                                 :292
    [tree_inverse_weight(s, W) if W > 0 else None ...]                 :298-302

Per group that is the oracle's exact fold ``wsum_dense`` over the group's members in client
order, started from a row of +0, times f32(1 / W_g); the ``W_g > 0`` rule is plain Python.
A client whose id is -1 is in no group: its row is never indexed.
"""
import numpy as np

from oracle import tree_util_ref as oracle

F32 = np.float32


def group_totals(weights, group_ids, num_groups):
    """W_g summed in client order from the int 0, as hyp_cluster.py:282,292 does."""
    totals = [0] * num_groups
    for w, g in zip(weights, group_ids):
        if g >= 0:
            totals[g] += w
    return totals


def grouped_mean_ref(x, weights, group_ids, num_groups):
    """List of G float32 [P] means (``None`` where W_g > 0 is false) of the rows of ``x`` [K, P]."""
    x = np.asarray(x, dtype=F32)
    ids = [int(g) for g in group_ids]
    assert len(ids) == x.shape[0] == len(weights) and all(-1 <= g < num_groups for g in ids)
    totals = group_totals(weights, ids, num_groups)
    out = []
    for g in range(num_groups):
        m = [k for k, gk in enumerate(ids) if gk == g]
        W = totals[g]
        if not (W > 0):
            out.append(None)
            continue
        scale = F32(1.0 / W)
        with np.errstate(all="ignore"):
            out.append(oracle.wsum_dense(x[m], [F32(weights[k]) for k in m], scale,
                                         init=np.zeros(x.shape[1], dtype=F32)).astype(F32))
    return out


def grouped_sum_ref(x, w, group_ids, num_groups, scales=None):
    """The raw grouped fold: every group with members gets its sum from +0 (times scales[g] if
    given), a group without members ``None``."""
    x = np.asarray(x, dtype=F32)
    out = []
    for g in range(num_groups):
        m = [k for k, gk in enumerate(group_ids) if gk == g]
        if not m:
            out.append(None)
            continue
        with np.errstate(all="ignore"):
            out.append(oracle.wsum_dense(x[m], np.asarray(w, dtype=F32)[m], None if scales is None else scales[g],
                                         init=np.zeros(x.shape[1], dtype=F32)).astype(F32))
    return out


def bits(a):
    """uint32 bit patterns with every NaN mapped to one pattern (IEEE 754 leaves a generated
    NaN's sign and payload to the implementation)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = np.uint32(0x7FC00000)
    return b


def seeded_ids(K, G, seed, force_edges=True):
    """Seeded group ids. With ``force_edges`` and K >= 5: at least two clients in no group (-1)
    and, as far as G allows, one group with exactly one member (G >= 2) and one group with
    none (G >= 3)."""
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, G, size=K)
    if force_edges and K >= 5:
        perm = rng.permutation(K)
        ids[perm[:2]] = -1
        if G >= 2:
            single = G - 1
            ids[ids == single] = 0
            ids[perm[2]] = single
        if G >= 3:
            ids[ids == G - 2] = 0
    return ids.astype(np.int64)
