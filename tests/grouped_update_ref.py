"""Numpy float32 restatement of a HypCluster round's server side (no product code but the
optimizer's hyperparameter descriptor).

The reference (fedjax/algorithms/hyp_cluster.py:107-128) takes the G cluster means of the
expectation step and, for every cluster whose mean is not ``None``, runs
``server_optimizer.apply(delta_params, opt_state, params)`` on that cluster's OWN params and
optimizer state; a cluster without a mean keeps its params and its state, step count included
(:121-123). Composed of existing pieces: the grouped mean of tests/grouped_mean_ref.py, then
per group with a result tests/test_gpu_parity.py's ``_np_server_step`` with the descriptor of
that cluster's incremented count.
"""
import numpy as np

from tests import grouped_mean_ref as gref
from tests.test_gpu_parity import _np_server_step

F32 = np.float32


def grouped_update_ref(x, weights, group_ids, num_groups, opt, params, ms, vs, counts):
    """One round. ``params`` / ``ms`` / ``vs``: lists of G float32 [P] arrays (``ms[g]`` /
    ``vs[g]`` None where the rule keeps no such moment); ``counts``: G ints. Nothing is changed
    in place. Returns a dict of lists: ``params``, ``m``, ``v``, ``counts``, ``means`` (None
    without a result) and ``updated``; a cluster that took no step keeps the very objects it
    came with."""
    means = gref.grouped_mean_ref(x, weights, group_ids, num_groups)
    out = {"params": list(params), "m": list(ms), "v": list(vs), "counts": list(counts), "means": means,
           "updated": [mean is not None for mean in means]}
    for g, mean in enumerate(means):
        if mean is None:
            continue
        d = opt.descriptor(counts[g] + 1)  # each cluster has its own step count
        with np.errstate(all="ignore"):
            p, m, v = _np_server_step(opt, d, mean, np.asarray(params[g], F32), ms[g], vs[g])
        out["params"][g] = np.asarray(p, F32)
        out["m"][g] = None if ms[g] is None else np.asarray(m, F32)
        out["v"][g] = None if vs[g] is None else np.asarray(v, F32)
        out["counts"][g] = counts[g] + 1
    return out
