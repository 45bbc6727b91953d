"""Numpy float32 restatement of a clipped round's server side (no product code but the
optimizer's hyperparameter descriptor).

The reference (fedjax/algorithms/mime_lite.py:131-149) clips every client's delta, weights and
adds it, divides by the unclipped total weight, and then steps the server model on that mean
(:162-167, ``params = p - server_learning_rate * mean``; with another server optimizer,
``server_optimizer.apply(mean, opt_state, params)``). Composed of existing pieces: the clipped
fold of tests/clipped_mean_ref.py, then tests/test_gpu_parity.py's ``_np_server_step`` with the
descriptor of the incremented count.
"""
import numpy as np

from tests import clipped_mean_ref as cref
from tests.test_gpu_parity import _np_server_step

F32 = np.float32


def inverse_total(weights):
    """f32(1 / W) with W summed from 0.0 in client order, 0 when W is not > 0 (tree_util.py:37,60)."""
    W = 0.0
    for v in weights:
        W += v
    return F32((1.0 / W) if W > 0.0 else 0.0)


def clipped_update_ref(x, weights, c, opt, params, m, v, count):
    """One round over deltas ``x`` [K, P] with the per-client factors ``c`` (restated from the
    norms by clipped_mean_ref.clip_factors_ref). ``m`` / ``v`` are None where the rule keeps no
    such moment. Nothing is changed in place. Returns ``(params, m, v, count, mean)``."""
    w32 = np.array([F32(t) for t in weights], dtype=F32)
    mean = cref.clipped_fold_ref(x, w32, c, inverse_total(weights))
    d = opt.descriptor(count + 1)
    with np.errstate(all="ignore"):
        p, m2, v2 = _np_server_step(opt, d, mean, np.asarray(params, F32), m, v)
    return (np.asarray(p, F32), None if m is None else np.asarray(m2, F32),
            None if v is None else np.asarray(v2, F32), count + 1, mean)


def mime_lite_sgd_ref(p, y, lr):
    """Mime Lite's own server update, fl(p - fl(f32(lr) * y)) (mime_lite.py:162-167)."""
    with np.errstate(all="ignore"):
        return (np.asarray(p, F32) - (F32(lr) * np.asarray(y, F32)).astype(F32)).astype(F32)
