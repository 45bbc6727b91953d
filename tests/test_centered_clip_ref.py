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


# ------------------------------------------------------------------ the restated norm order
NORM_SIZES = [0, 1, 255, 256, 257, 2049, 65536 + 300]


def literal_l2sq(leaves_x, leaves_v):
    """The centred norm pass written out a second time, with no array arithmetic: per 64 Ki-element
    block a scalar loop per lane (elements t, t + 256, ... from +0), the xor shuffle tree of each
    wave step by step (every lane adds its partner's value of the step before), the four wave sums
    in order, and the block partials in leaf / block order from +0."""
    total = F32(0)
    with np.errstate(all="ignore"):
        for a, b in zip(leaves_x, leaves_v):
            n = len(a)
            for e0 in range(0, max(n, 1), 65536):
                e1 = min(e0 + 65536, n)
                lanes = []
                for t in range(256):
                    s = F32(0)
                    for e in range(e0 + t, e1, 256):
                        d = F32(F32(a[e]) - F32(b[e]))
                        s = F32(s + F32(d * d))
                    lanes.append(s)
                for step in (32, 16, 8, 4, 2, 1):
                    lanes = [F32(lanes[i] + lanes[(i & ~63) | ((i & 63) ^ step)]) for i in range(256)]
                t = lanes[0]
                for wave in (1, 2, 3):
                    t = F32(t + lanes[64 * wave])
                total = F32(total + t)
    return total


def norm_case(seed=0):
    """Two clients and a centre over NORM_SIZES, client 1 four times as far from the centre."""
    rng = np.random.RandomState(77 + seed)
    P = sum(NORM_SIZES)
    v = (0.5 * rng.standard_normal(P)).astype(F32)
    x = (v + rng.standard_normal((2, P)) * np.array([[1.0], [4.0]])).astype(F32)
    return x, v, np.concatenate([[0], np.cumsum(NORM_SIZES)])


def test_vectorised_norm_order_is_the_literal_one():
    x, v, offs = norm_case()
    cut = lambda a: [a[o:o + n] for o, n in zip(offs[:-1], NORM_SIZES)]
    for k in range(2):
        # every size as a row of its own (one leaf), then the whole row cut into all of them
        for o, n in zip(offs[:-1], NORM_SIZES):
            want = literal_l2sq([x[k, o:o + n]], [v[o:o + n]])
            got = ref.centered_l2sq_ref([x[k, o:o + n]], [v[o:o + n]])
            assert ref.bits(got) == ref.bits(want), (k, n)
            rows = ref.centered_l2sq_rows_ref(x[:, o:o + n], v[o:o + n], [n])
            assert ref.bits(rows[k]) == ref.bits(want), (k, n)
            assert n > 0 or ref.bits(want) == 0
        want = literal_l2sq(cut(x[k]), cut(v))
        assert ref.bits(ref.centered_l2sq_ref(cut(x[k]), cut(v))) == ref.bits(want)
        assert ref.bits(ref.centered_l2sq_rows_ref(x, v, NORM_SIZES)[k]) == ref.bits(want)
        d = ref.centered_distances_ref(x, v, NORM_SIZES)
        assert d.dtype == F32 and ref.bits(d[k]) == ref.bits(np.sqrt(want))
    # the order matters: the four wave sums added in reverse give other bits in a good share of rows
    rng = np.random.RandomState(3)
    x48, v0 = rng.standard_normal((48, 1027)).astype(F32), rng.standard_normal(1027).astype(F32)
    fwd, rev = ref.centered_l2sq_rows_ref(x48, v0, [1027]), ref.centered_l2sq_rows_ref(x48, v0, [1027], (3, 2, 1, 0))
    assert (ref.bits(fwd) != ref.bits(rev)).sum() >= 8
    assert all(ref.bits(fwd[k]) == ref.bits(ref.centered_l2sq_ref([x48[k]], [v0])) for k in range(48))
    # and so does the leaf cut: the whole row as ONE leaf is another sum
    one = ref.centered_l2sq_rows_ref(x, v, [x.shape[1]])
    assert (ref.bits(one) != ref.bits(ref.centered_l2sq_rows_ref(x, v, NORM_SIZES))).any()


def test_restated_distances_are_within_the_float64_bound():
    x, v, offs = norm_case(seed=1)
    for o, n in zip(offs[:-1], NORM_SIZES):
        got = ref.centered_distances_ref(x[:, o:o + n], v[o:o + n], [n]).astype(np.float64)
        want = ref.centered_distances_f64(x[:, o:o + n], v[o:o + n])
        assert (np.abs(got - want) <= 2e-6 * want).all(), (n, got, want)
    for sizes in (NORM_SIZES, [x.shape[1]]):
        got = ref.centered_distances_ref(x, v, sizes).astype(np.float64)
        want = ref.centered_distances_f64(x, v)
        assert (np.abs(got - want) <= 2e-6 * want).all(), (sizes, got, want)


def test_restated_norms_of_special_rows():
    """q of an all-zero row is +0, of a row holding a NaN NaN, of one holding an inf inf, and of a
    row of 1e30 inf (the float32 squares overflow): the contract's n = 0, NaN, inf, inf and hence
    c = 1, NaN, 0, 0."""
    sizes = [3, 0, 300, 65536 + 300]
    P = sum(sizes)
    rng = np.random.RandomState(5)
    v = rng.standard_normal(P).astype(F32)
    x = np.tile(v, (5, 1))  # row 0: the centre itself, d = +0 everywhere
    x[1, 66000] = np.nan  # in the last leaf's second block
    x[2, 2] = np.inf
    x[3, :] = 1e30
    x[4] = (v + rng.standard_normal(P)).astype(F32)
    q = ref.centered_l2sq_rows_ref(x, v, sizes)
    assert ref.bits(q[0]) == 0 and np.isnan(q[1]) and q[2] == np.inf and q[3] == np.inf and np.isfinite(q[4])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for k in range(5):
        one = ref.centered_l2sq_ref([x[k, o:o + n] for o, n in zip(offs[:-1], sizes)],
                                    [v[o:o + n] for o, n in zip(offs[:-1], sizes)])
        assert np.array_equal(canon_nan(one), canon_nan(q[k])), k
    d = ref.centered_distances_ref(x, v, sizes)
    assert ref.bits(d[0]) == 0 and np.isnan(d[1]) and d[2] == np.inf and d[3] == np.inf
    got, dist, fac = ref.centered_clip_ref(x, v, 1.0, 2, sizes=sizes)
    assert fac[0, 0] == 1 and np.isnan(fac[0, 1]) and fac[0, 2] == 0 and fac[0, 3] == 0 and 0 < fac[0, 4] < 1
    assert np.isfinite(got).all()
    # the closed round is the fold driven by its own factors, and its distances are its own centre's
    again, _, _ = ref.centered_clip_ref(x, v, 1.0, 2, factors=fac)
    assert np.array_equal(ref.bits(again), ref.bits(got))
    v1 = ref.centered_fold_ref(x, v, fac[0])
    assert np.array_equal(canon_nan(dist[1]), canon_nan(ref.centered_distances_ref(x, v1, sizes)))


def canon_nan(a):
    """Bit patterns with every NaN mapped to one."""
    a = np.atleast_1d(np.asarray(a, dtype=F32))
    b = ref.bits(a).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


# ------------------------------------------------------------------ refusals that need no device
def test_out_overlapping_the_deltas_is_refused_on_the_host():
    """An out anywhere inside [x, x + ((K-1)*ld + P)*4) is refused before anything is launched:
    the wrappers' own check raises ValueError, and the two dense entries return FJAGG_EUNSUPPORTED
    with a message. The entries are met with made-up addresses, so only where no device could be
    handed them (tests/test_gpu_centered_clip_limits.py makes the same calls with real buffers)."""
    import torch

    from fedjax_amd import _lib, kernels

    lib = _lib.load()
    K, P, ld, x0, far = 3, 8, 10, 1 << 20, 1 << 24
    span = ((K - 1) * ld + P) * 4
    for out in () if torch.cuda.is_available() else (x0 - 4 * P + 4, x0, x0 + 4, x0 + 4 * ld, x0 + span - 4):
        rc = lib.fjagg_center_fold_dense(_lib.F32, x0, ld, K, P, far, far + 4096, out, 0, None)
        assert rc == -3 and b"overlaps the deltas" in lib.fjagg_last_error(), out
        rc = lib.fjagg_center_clip_dense(_lib.F32, x0, ld, K, P, None, 1, P, 1.0, 1, far + 4096, out, far, far + 64,
                                         far + 8192, 1 << 16, 0, None)
        assert rc == -3 and b"overlaps the deltas" in lib.fjagg_last_error(), out
    if not torch.cuda.is_available():
        # one client: the extent is the row, whatever ld says
        assert lib.fjagg_center_fold_dense(_lib.F32, x0, 1 << 40, 1, P, far, far + 4096, x0 + 4 * P - 4, 0, None) == -3
        # a centre inside the deltas is not the overlap that is refused: what comes back is the next check's
        rc = lib.fjagg_center_fold_dense(_lib.F32, x0, ld, K, P, None, x0 + 4 * ld, far, 0, None)
        assert rc == -3 and b"null pointer" in lib.fjagg_last_error()
    store = torch.zeros(64)
    x = torch.as_strided(store, (K, P), (ld, 1), 16)
    centre = torch.zeros(P)
    for o in (9, 16, 17, 16 + ld, 16 + (K - 1) * ld + P - 1):
        with pytest.raises(ValueError, match="overlap the deltas"):
            kernels._check_center_vectors(centre, store[o:o + P], x)
    for o in (8, 16 + (K - 1) * ld + P):  # beside the slab
        assert kernels._check_center_vectors(centre, store[o:o + P], x).data_ptr() == store[o:o + P].data_ptr()
    assert kernels._check_center_vectors(x[1], store[:P], x).data_ptr() == store.data_ptr()  # the centre is a row
