"""The numpy restatement of centered clipping (tests/centered_clip_ref.py) against what the rule
must do, on the CPU: (a) a zero centre and one iteration is the clipped mean with unit weights,
(b) clients at the centre leave it where it is, (c) Byzantine rows move the result by at most
|B| tau / K, (d) rows holding NaN, inf or 1e30 are skipped, (e) two iterations are two single
ones chained. No product code runs here; tests/test_gpu_centered_clip.py holds the library to
this restatement.
"""
import numpy as np
import pytest

from tests import centered_clip_ref as ref
from tests import clipped_mean_ref as cm

F32 = np.float32
SHAPES = [(1, 1), (2, 3), (3, 4), (7, 5), (8, 63), (9, 64), (16, 65), (17, 255), (63, 256), (64, 257), (65, 1000),
          (130, 4099)]


def normal(K, P, seed=0):
    return np.random.RandomState(1000 * seed + 7 * K + P).standard_normal((K, P)).astype(F32)


def canon(a):
    """Bit patterns with -0 mapped to +0."""
    a = np.asarray(a, dtype=F32).copy()
    a[a == 0] = 0.0
    return ref.bits(a)


def median_tau(x, v):
    return float(np.median(ref.centered_distances_f64(x, v)))


@pytest.mark.parametrize("K,P", SHAPES)
def test_zero_centre_is_the_clipped_mean(K, P):
    x = normal(K, P)
    tau = median_tau(x, np.zeros(P, F32))
    got, dist, fac = ref.centered_clip_ref(x, np.zeros(P, F32), tau, 1)
    want = cm.clipped_fold_ref(x, np.ones(K, F32), fac[0], F32(1.0 / K))
    assert np.array_equal(canon(got), canon(want))
    assert np.array_equal(ref.bits(fac[0]), ref.bits(cm.clip_factors_ref(dist[0], tau)))
    assert (fac[0] < 1).any() or K == 1


@pytest.mark.parametrize("K,P", SHAPES)
def test_fixed_point(K, P):
    v = normal(1, P, seed=3)[0]
    x = np.tile(v, (K, 1))
    got, dist, fac = ref.centered_clip_ref(x, v, 0.5, 2)
    assert np.array_equal(ref.bits(got), ref.bits(v))
    assert (dist == 0).all() and (fac == 1).all()


def byzantine_bound(x, v, fac, nbyz, tau):
    """|B| tau / K (1 + 1e-5) in l2, plus the float32 fold bound (K + 2) 2^-24 sum_k |t_k| per
    element taken in l2, over the attacked run's own terms."""
    K = x.shape[0]
    with np.errstate(all="ignore"):
        d = (x - v).astype(F32)
        t = np.where((fac > 0)[:, None], (fac[:, None] * d).astype(F32), F32(0)).astype(np.float64)
    fold = (K + 2) * 2.0 ** -24 * np.abs(t).sum(axis=0)
    return nbyz * tau / K * (1 + 1e-5) + float(np.sqrt((fold * fold).sum()))


@pytest.mark.parametrize("K,P", SHAPES)
def test_byzantine_rows_move_the_result_by_at_most_tau_over_k(K, P):
    rng = np.random.RandomState(K * 31 + P)
    v = (0.1 * rng.standard_normal(P)).astype(F32)
    x = (v + normal(K, P, seed=1)).astype(F32)
    tau = median_tau(x, v)
    B = sorted(rng.choice(K, size=max(1, K // 5), replace=False))
    attacked, clean = x.copy(), x.copy()
    attacked[B] = (1e6 * rng.standard_normal((len(B), P))).astype(F32)
    clean[B] = v
    got, _, fac = ref.centered_clip_ref(attacked, v, tau, 1)
    base, _, _ = ref.centered_clip_ref(clean, v, tau, 1)
    moved = float(np.sqrt(((got.astype(np.float64) - base.astype(np.float64)) ** 2).sum()))
    bound = byzantine_bound(attacked, v, fac[0], len(B), tau)
    assert np.isfinite(got).all()
    assert moved <= bound, (moved, bound, moved / bound)
    plain = attacked.astype(np.float64).mean(axis=0) - clean.astype(np.float64).mean(axis=0)
    assert np.sqrt((plain ** 2).sum()) > 100 * bound  # the plain mean is off by ~1e6 / sqrt(K)


@pytest.mark.parametrize("K,P", [(4, 1), (5, 4), (9, 65), (17, 257), (130, 4099)])
def test_unusable_rows_are_skipped(K, P):
    v = normal(1, P, seed=4)[0]
    x = (v + normal(K, P, seed=2)).astype(F32)
    tau = median_tau(x, v)
    x[0, P // 2] = np.nan
    x[1, 0] = np.inf
    x[2, :] = 1e30
    got, dist, fac = ref.centered_clip_ref(x, v, tau, 1)
    assert np.isnan(fac[0, 0]) and fac[0, 1] == 0 and fac[0, 2] == 0
    assert np.isnan(dist[0, 0]) and np.isinf(dist[0, 1]) and np.isinf(dist[0, 2])
    assert np.isfinite(got).all()
    # the run without those rows' terms: their rows sit at the centre (terms +0), the divisor stays K
    without = x.copy()
    without[:3] = v
    want = ref.centered_fold_ref(without, v, np.concatenate([np.ones(3, F32), fac[0, 3:]]))
    assert np.array_equal(ref.bits(got), ref.bits(want))


@pytest.mark.parametrize("K,P", SHAPES)
def test_two_iterations_are_two_calls_chained(K, P):
    v = normal(1, P, seed=5)[0]
    x = (v + 2 * normal(K, P, seed=6)).astype(F32)
    tau = 0.7 * median_tau(x, v)
    got, dist, fac = ref.centered_clip_ref(x, v, tau, 2)
    v1, d1, f1 = ref.centered_clip_ref(x, v, tau, 1)
    v2, d2, f2 = ref.centered_clip_ref(x, v1, tau, 1)
    assert np.array_equal(ref.bits(got), ref.bits(v2))
    assert np.array_equal(ref.bits(dist), ref.bits(np.stack([d1[0], d2[0]])))
    assert np.array_equal(ref.bits(fac), ref.bits(np.stack([f1[0], f2[0]])))
    # driven by given factors, the folds repeat the same bits
    again, _, _ = ref.centered_clip_ref(x, v, tau, 2, factors=fac)
    assert np.array_equal(ref.bits(again), ref.bits(got))
