"""The restatement of the per-cluster server step (tests/grouped_update_ref.py) pinned on the CPU:
the reference's own numbers (hyp_cluster_test.py:452-472), and the rule that a cluster which sat
out a round keeps its params, state and step count, so that its next step is an EARLIER step than
the other clusters' (hyp_cluster.py:121-123).
"""
import numpy as np

from fedjax_amd import server
from tests import algorithms_restated as ar
from tests import grouped_mean_ref as gref
from tests.grouped_update_ref import grouped_update_ref
from tests.test_gpu_parity import _np_server_step

F32 = np.float32


def test_reference_kat_hyp_cluster_round():
    """hyp_cluster_test.py:452-472 with the setup of algorithms_restated.hyp_cluster_round:
    clusters [1, -1], four clients, sgd(0.25)."""
    params = [F32(1.), F32(-1.)]
    ids = [int(np.argmin([np.mean(np.square((F32(p) - x).astype(F32)), dtype=F32) for p in params]))
           for _, x in ar._HC_CLIENTS]
    assert ids == [0, 0, 1, 1]
    x = np.array([[ar._hc_delta(params[g], xs)] for g, (_, xs) in zip(ids, ar._HC_CLIENTS)], dtype=F32)
    weights = [len(xs) for _, xs in ar._HC_CLIENTS]
    got = grouped_update_ref(x, weights, ids, 2, server.sgd(0.25), [np.array([p], F32) for p in params],
                             [None, None], [None, None], [0, 0])
    assert got["updated"] == [True, True] and got["counts"] == [1, 1]
    np.testing.assert_allclose(got["params"][0], [1 - 0.25 * 0.1 / 3], rtol=1e-7)
    np.testing.assert_allclose(got["params"][1], [-1 + 0.25 * 0.2 / 4], rtol=1e-7)


def test_empty_cluster_keeps_everything_and_steps_later_with_its_own_count():
    rs = np.random.RandomState(5)
    K, G, P = 7, 3, 33
    opt = server.adam(0.01, b1=0.9, b2=0.999, eps=1e-4)
    p0 = [rs.uniform(-1, 1, P).astype(F32) for _ in range(G)]
    m0 = [np.zeros(P, F32) for _ in range(G)]
    v0 = [np.zeros(P, F32) for _ in range(G)]
    x1, x2 = (rs.uniform(-0.02, 0.02, (K, P)).astype(F32) for _ in range(2))
    w = [3, 1, 4, 1, 5, 9, 2]
    r1 = grouped_update_ref(x1, w, [0, 2, 0, -1, 2, 0, 2], G, opt, p0, m0, v0, [0, 0, 0])
    assert r1["updated"] == [True, False, True] and r1["counts"] == [1, 0, 1] and r1["means"][1] is None
    # untouched means the very objects, not equal copies
    assert r1["params"][1] is p0[1] and r1["m"][1] is m0[1] and r1["v"][1] is v0[1]
    assert not np.array_equal(r1["params"][0], p0[0]) and np.array_equal(p0[1], r1["params"][1])
    ids2 = [0, 1, 1, -1, 2, 0, 2]
    r2 = grouped_update_ref(x2, w, ids2, G, opt, r1["params"], r1["m"], r1["v"], r1["counts"])
    assert r2["updated"] == [True, True, True] and r2["counts"] == [2, 1, 2]
    means = gref.grouped_mean_ref(x2, w, ids2, G)
    for g, t in enumerate([2, 1, 2]):
        p, m, v = _np_server_step(opt, opt.descriptor(t), means[g], r1["params"][g], r1["m"][g], r1["v"][g])
        assert np.array_equal(gref.bits(r2["params"][g]), gref.bits(p)), g
        assert np.array_equal(gref.bits(r2["m"][g]), gref.bits(m)) and np.array_equal(gref.bits(r2["v"][g]), gref.bits(v))
    # the count matters: cluster 1's step with the other clusters' count is another step
    p_wrong, _, _ = _np_server_step(opt, opt.descriptor(2), means[1], r1["params"][1], r1["m"][1], r1["v"][1])
    assert not np.array_equal(gref.bits(p_wrong), gref.bits(r2["params"][1]))
    assert opt.descriptor(1).bc1 != opt.descriptor(2).bc1
