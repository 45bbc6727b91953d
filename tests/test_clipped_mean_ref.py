"""The numpy restatement of the clipped weighted mean (tests/clipped_mean_ref.py) against
the reference's own numbers and the IEEE edge cases. No GPU needed; the product is touched
only to show that it exposes the API the GPU tests exercise."""
import numpy as np

from tests import clipped_mean_ref as ref

F32 = np.float32


def test_clip_scales_special_values():
    q = np.array([0.0, np.inf, np.nan, 0.25, 4.0], dtype=F32)
    n, c = ref.clip_scales_ref(q, 1.0)
    assert c.dtype == F32 and n.dtype == F32
    assert c[0] == 1.0 and n[0] == 0.0        # norm 0: 1 / 0 = +inf -> 1
    assert c[1] == 0.0 and np.isinf(n[1])     # norm inf: 1 / inf = 0
    assert np.isnan(c[2]) and np.isnan(n[2])  # NaN propagates through the minimum
    assert c[3] == 1.0 and n[3] == 0.5        # 1 / 0.5 = 2 -> 1
    assert c[4] == 0.5 and n[4] == 2.0


def test_clip_scales_just_below_one():
    # sqrt(1 + 2^-22) rounds to 1 + 2^-23, the float after 1; 1 / that rounds just under 1
    q = F32(1) + F32(2.0 ** -22)
    n, c = ref.clip_scales_ref([q], 1.0)
    assert n[0] == np.nextafter(F32(1), F32(2))
    assert c[0] < 1.0 and F32(1) - c[0] <= F32(2.0 ** -23)
    # and the float between (1 + 2^-23 squared down) still clips nothing
    n1, c1 = ref.clip_scales_ref([np.nextafter(F32(1), F32(2))], 1.0)
    assert n1[0] == 1.0 and c1[0] == 1.0


def test_clip_scales_zero_and_infinite_max_norm():
    q = np.array([0.0, 4.0, np.inf], dtype=F32)
    _, c0 = ref.clip_scales_ref(q, 0.0)
    assert np.isnan(c0[0]) and c0[1] == 0.0 and c0[2] == 0.0  # 0 / 0 = NaN
    _, ci = ref.clip_scales_ref(q, np.inf)
    assert ci[0] == 1.0 and ci[1] == 1.0 and np.isnan(ci[2])  # inf / inf = NaN


def test_restated_fold_differs_from_merged_weight_fold():
    """fl(fl(c x) w) is not fl(x fl(c w)): the restatement can tell the two apart."""
    rng = np.random.RandomState(7)
    K, P = 5, 1027
    x = rng.standard_normal((K, P)).astype(F32)
    w = rng.randint(1, 500, K).astype(F32)
    c = rng.uniform(0.25, 1.0, K).astype(F32)
    scale = F32(1.0 / float(w.astype(np.float64).sum()))
    a = ref.clipped_fold_ref(x, w, c, scale)
    b = ref.merged_fold_ref(x, w, c, scale)
    differ = int((ref.bits(a) != ref.bits(b)).sum())
    assert differ >= 1
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7)  # the same quantity all the same


def test_fold_init_and_scale():
    x = np.array([[1.0, 2.0], [3.0, 4.0]], dtype=F32)
    got = ref.clipped_fold_ref(x, [2.0, 1.0], [0.5, 1.0], 0.5, init=[10.0, 20.0])
    np.testing.assert_array_equal(got, np.array([(10 + 1 + 3) * 0.5, (20 + 2 + 4) * 0.5], dtype=F32))


def test_reference_kat():
    """fedjax/core/tree_util_test.py:64-75: max_norm = 3.640055 = 0.5 * tree_l2_norm(pytree)."""
    x = np.array([4, 5, 1, 1], dtype=F32)
    y = np.array([3, 1], dtype=F32)
    flat = np.concatenate([x, y])[None, :]
    q = (flat * flat).sum(dtype=F32)
    assert q == 53.0
    _, c = ref.clip_scales_ref([q], 3.640055)
    clipped = ref.clipped_products(flat, c)[0]
    np.testing.assert_array_almost_equal(clipped[:4], [2, 2.5, 0.5, 0.5])
    np.testing.assert_array_almost_equal(clipped[4:], [1.5, 0.5])
    # the weighted mean of that one client with weight 3 is the clipped pytree again
    mean = ref.clipped_fold_ref(flat, [3.0], c, F32(1.0 / 3.0))
    np.testing.assert_array_almost_equal(mean, [2, 2.5, 0.5, 0.5, 1.5, 0.5])


def test_product_exposes_the_clipped_mean_api():
    import fedjax_amd
    from fedjax_amd import _lib, kernels, slab, tree_util

    assert tree_util.ClippedMean._fields == ("mean", "norms", "clipped_norms", "clipped")
    for obj, name in ((kernels, "clip_scales"), (kernels, "clipped_sum_dense"), (tree_util, "tree_clipped_mean"),
                      (slab.ClientDeltaSlab, "clipped_mean"), (fedjax_amd.aggregators, "clipped_mean_aggregator")):
        assert callable(getattr(obj, name)), name
    assert _lib.ABI_VERSION == 4
    for sym in ("fjagg_clip_scales", "fjagg_wsum_clip_dense", "fjagg_wsum_clip_ptrs", "fjagg_clip_finish",
                "fjagg_wsum_clip_workspace_bytes", "fjagg_wsum_clip_ptrs_workspace_bytes"):
        assert sym in _lib.SYMBOLS
    # empty input: all-None, as tree_mean_with_l2_norms answers no clients
    assert tree_util.tree_clipped_mean([], 1.0) == tree_util.ClippedMean(None, None, None, None)


def test_raw_entry_points_refuse_unsupported_flags_on_the_host():
    """FJAGG_NARROW / FJAGG_HOST_TABLES / FJAGG_ZEROED_WS, a variant byte and non-f32 dtypes
    return FJAGG_EUNSUPPORTED before any HIP call (dummy pointers are never touched)."""
    from fedjax_amd import _lib

    lib = _lib.load()
    for fl in (_lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, 12 << 8, _lib.UNBALANCED):
        rc = lib.fjagg_wsum_clip_dense(_lib.F32, 16, 8, 2, 8, 16, 16, 1.0, 16, None, fl, None, 0, None)
        assert rc == -3, fl
        rc = lib.fjagg_wsum_clip_ptrs(_lib.F32, 16, 1, 2, 1, 16, 16, 1.0, None, fl, None, 0, None)
        assert rc == -3, fl
    for dt in (_lib.BF16, _lib.I32):
        assert lib.fjagg_wsum_clip_dense(dt, 16, 8, 2, 8, 16, 16, 1.0, 16, None, 0, None, 0, None) == -3
        assert lib.fjagg_wsum_clip_ptrs(dt, 16, 1, 2, 1, 16, 16, 1.0, None, 0, None, 0, None) == -3
    # norms for more than 4096 clients
    assert lib.fjagg_wsum_clip_dense(_lib.F32, 16, 8, 5000, 8, 16, 16, 1.0, 16, 16, 0, 16, 1 << 30, None) == -3
    assert lib.fjagg_wsum_clip_ptrs(_lib.F32, 16, 1, 5000, 1, 16, 16, 1.0, 16, 0, 16, 1 << 30, None) == -3
    assert b"4096" in lib.fjagg_last_error()
    # the pytree entry alone takes FJAGG_UNALIGNED
    assert lib.fjagg_wsum_clip_dense(_lib.F32, 16, 8, 2, 8, 16, 16, 1.0, 16, None, _lib.UNALIGNED, None, 0, None) == -3
