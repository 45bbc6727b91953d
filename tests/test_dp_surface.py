"""The differentially private clipped mean's Python surface without a GPU: validation before
any launch, the aggregator's noise calibration and key consumption, the per-leaf key schedule,
and a sanity check of the numpy restatement of the normal (tests/normal_restated.py) that the
GPU tests hold the device draw to."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, random as fjr, slab as slab_mod, tree_util as tu
from fedjax_amd.aggregators import aggregator as agg_mod
from oracle import jax_random_ref as jr
from tests import normal_restated as nr

KEY = fjr.PRNGKey(3)


def cpu_slab(K=2, dtype=torch.float32):
    return slab_mod.ClientDeltaSlab({"a": np.zeros(3, np.float32), "b": np.zeros((2, 2), np.float32)}, K, dtype=dtype,
                                    device=torch.device("cpu"))


def pairs(K=2, dtype=np.float32):
    return [({"a": np.ones(3, dtype)}, 1.0) for _ in range(K)]


# ------------------------------------------------------------------------- validation
@pytest.mark.parametrize("stddev", [-1.0, -1e-50, float("nan"), float("inf"), -float("inf"), 1e39])
def test_bad_noise_stddev_raises(stddev):
    with pytest.raises(ValueError, match="noise_stddev"):
        tu.tree_dp_clipped_mean(pairs(), 1.0, stddev, KEY)
    with pytest.raises(ValueError, match="noise_stddev"):
        cpu_slab().dp_clipped_mean([1.0, 1.0], 1.0, stddev, KEY)


def test_noise_stddev_type():
    with pytest.raises(TypeError):
        tu.tree_dp_clipped_mean(pairs(), 1.0, "0.1", KEY)
    assert kernels.check_noise_stddev(0) == 0.0
    assert kernels.check_noise_stddev(np.float32(0.25)) == 0.25


@pytest.mark.parametrize("key", [np.zeros(3, np.uint32), np.zeros((1, 2), np.uint32), 7, [1, 2, 3], [-1, 0], [0, 1 << 32]])
def test_bad_key_raises_value_error(key):
    with pytest.raises(ValueError, match="two uint32"):
        tu.tree_dp_clipped_mean(pairs(), 1.0, 0.1, key)
    with pytest.raises(ValueError, match="two uint32"):
        cpu_slab().dp_clipped_mean([1.0, 1.0], 1.0, 0.1, key)


@pytest.mark.parametrize("key", [np.zeros(2, np.float32), [0.5, 1.0], "ab", None])
def test_bad_key_raises_type_error(key):
    with pytest.raises(TypeError, match="two uint32"):
        tu.tree_dp_clipped_mean(pairs(), 1.0, 0.1, key)
    with pytest.raises(TypeError, match="two uint32"):
        cpu_slab().dp_clipped_mean([1.0, 1.0], 1.0, 0.1, key)
    with pytest.raises(TypeError, match="two uint32"):
        fedjax_amd.aggregators.dp_clipped_mean_aggregator(1.0, 1.0, key)


def test_strict_key_accepts_keys():
    for k in (KEY, [1, 2], np.array([1, 2], np.int64), fjr.split(KEY)[1], (0, 0xFFFFFFFF)):
        got = fjr.strict_key(k)
        assert got.dtype == np.uint32 and got.shape == (2,)
        assert [int(v) for v in got] == [int(v) for v in np.asarray(k).reshape(-1)]


def test_non_f32_raises():
    with pytest.raises(TypeError, match="float32 slab"):
        cpu_slab(dtype=torch.bfloat16).dp_clipped_mean([1.0, 1.0], 1.0, 0.1, KEY)
    with pytest.raises(TypeError, match="float32 leaves"):
        tu.tree_dp_clipped_mean([({"a": np.ones(3, np.int32)}, 1.0)], 1.0, 0.1, KEY)
    with pytest.raises(TypeError, match="float32 leaves"):
        tu.tree_dp_clipped_mean([({"a": torch.ones(3, dtype=torch.bfloat16)}, 1.0)], 1.0, 0.1, KEY)


def test_too_many_clients_raises():
    K = tu._L2_MAX_CLIENTS + 1
    with pytest.raises(ValueError, match="clients"):
        tu.tree_dp_clipped_mean(pairs(K), 1.0, 0.1, KEY)
    with pytest.raises(ValueError, match="clients"):
        cpu_slab(K).dp_clipped_mean([1.0] * K, 1.0, 0.1, KEY)


def test_no_clients():
    assert tu.tree_dp_clipped_mean([], 1.0, 0.1, KEY) == tu.ClippedMean(None, None, None, None)
    agg = fedjax_amd.aggregators.dp_clipped_mean_aggregator(1.0, 1.0, KEY)
    mean, state = agg.apply([], agg.init())
    assert mean is None and state.norms == {} and state.noise_stddev is None


def test_entry_points_refuse_bad_descriptors_on_the_host():
    """The C entry points check the noise descriptor before any HIP call."""
    lib = _lib.load()

    def dense(noise, P=8, flags=_lib.SCALE, dtype=_lib.F32):
        return lib.fjagg_wsum_clip_noise_dense(dtype, 16, P, 2, P, 16, 16, 1.0, 16, None,
                                               None if noise is None else noise.ref, flags, None, 0, None)

    ok_keys = np.zeros((2, 2), np.uint32)
    assert dense(None) == -1 and b"noise" in lib.fjagg_last_error()
    for sd in (-1.0, float("nan"), float("inf")):
        assert dense(kernels.NoiseTable(sd, [0, 4], [4, 4], ok_keys)) == -1 and b"stddev" in lib.fjagg_last_error()
    assert dense(kernels.NoiseTable(0.1, [0, 3], [4, 4], ok_keys)) == -1 and b"overlaps" in lib.fjagg_last_error()
    assert dense(kernels.NoiseTable(0.1, [0, 4], [4, 5], ok_keys)) == -1 and b"row" in lib.fjagg_last_error()
    assert dense(kernels.NoiseTable(0.1, [0, 4], [4, -1], ok_keys)) == -1
    many = _lib.NOISE_MAX_LEAVES + 1
    big = kernels.NoiseTable(0.1, np.arange(many), np.ones(many, np.int64), np.zeros((many, 2), np.uint32))
    assert dense(big, P=many) == -3 and b"leaves" in lib.fjagg_last_error()
    good = kernels.NoiseTable(0.1, [0, 4], [4, 4], ok_keys)
    assert dense(good, flags=_lib.SCALE | _lib.ACCUMULATE) == -3 and b"ACCUMULATE" in lib.fjagg_last_error()
    assert dense(good, dtype=_lib.BF16) == -3
    assert dense(good, flags=_lib.SCALE | _lib.HOST_TABLES) == -3
    rc = lib.fjagg_wsum_clip_noise_dense(_lib.F32, 16, 8, tu._L2_MAX_CLIENTS + 1, 8, 16, 16, 1.0, 16, 16, good.ref,
                                         _lib.SCALE, 16, 1 << 20, None)
    assert rc == -3 and b"K <=" in lib.fjagg_last_error()
    # pytree entry: the plan's L, and more leaves than the arguments hold need the device table
    rc = lib.fjagg_wsum_clip_noise_ptrs(_lib.F32, 16, 3, 2, 1, 16, 16, 1.0, None, good.ref, _lib.SCALE, None, 0, None)
    assert rc == -1 and b"noise leaves" in lib.fjagg_last_error()
    rc = lib.fjagg_wsum_clip_noise_ptrs(_lib.F32, 16, many, 2, 1, 16, 16, 1.0, None, big.ref, _lib.SCALE, None, 0, None)
    assert rc == -3 and b"leaves" in lib.fjagg_last_error()
    assert lib.fjcomp_normal(None, 4, 16, None) == -1
    assert lib.fjcomp_normal(KEY.ctypes.data, -1, 16, None) == -1
    assert lib.fjcomp_normal(KEY.ctypes.data, 0, None, None) == 0
    assert lib.fjcomp_normal_from_bits(None, 4, 16, None) == -1
    assert lib.fjcomp_normal_from_bits(None, 0, None, None) == 0


def test_noise_table_layout():
    import ctypes
    assert ctypes.sizeof(_lib.NoiseLeaf) == 24 and ctypes.sizeof(_lib.Noise) == 24
    t = kernels.NoiseTable(0.5, [0, 7], [7, 2], np.array([[1, 2], [3, 4]], np.uint32))
    assert (t.desc.stddev, t.desc.L) == (0.5, 2)
    assert [(e.begin, e.n, e.k0, e.k1) for e in t.host] == [(0, 7, 1, 2), (7, 2, 3, 4)]


# ------------------------------------------------------------------------- aggregator
def test_aggregator_noise_stddev():
    """weights [1, 2, 5], max_norm 0.5, multiplier 1.1: f32(1.1 * 0.5 * 5 / 8), Python floats."""
    want = float(np.float32(1.1 * 0.5 * 5.0 / 8.0))
    assert agg_mod.dp_noise_stddev(1.1, 0.5, [1, 2, 5]) == want
    assert agg_mod.dp_noise_stddev(1.1, 0.5, [np.float32(1), 2.0, np.int64(5)]) == want
    assert want == float(np.float32(0.34375))


def test_aggregator_takes_one_key_per_apply(monkeypatch):
    seen = []

    def fake(pairs_, max_norm, stddev, key):
        seen.append((len(pairs_), max_norm, stddev, np.array(key)))
        z = torch.zeros(len(pairs_))
        return tu.ClippedMean({"a": None}, z, z.clone(), z.bool())

    monkeypatch.setattr(tu, "tree_dp_clipped_mean", fake)
    seq = fjr.PRNGSequence(11)
    agg = fedjax_amd.aggregators.dp_clipped_mean_aggregator(0.5, 1.1, seq)
    clients = [(b"a", {"a": None}, 1), (b"b", {"a": None}, 2), (b"c", {"a": None}, 5)]
    state = agg.init()
    assert state.noise_stddev is None
    _, state = agg.apply(clients, state)
    _, state2 = agg.apply(iter(clients[:2]), state)
    ref_seq = jr.PRNGSequence(jr.prng_key(11))
    k1, k2 = next(ref_seq), next(ref_seq)
    assert [s[0] for s in seen] == [3, 2]
    assert np.array_equal(seen[0][3], k1) and np.array_equal(seen[1][3], k2) and not np.array_equal(k1, k2)
    assert np.array_equal(seq.internal_state, ref_seq._key)  # two keys taken, no more
    assert state.noise_stddev == seen[0][2] == float(np.float32(1.1 * 0.5 * 5.0 / 8.0))
    assert state2.noise_stddev == seen[1][2] == float(np.float32(1.1 * 0.5 * 2.0 / 3.0))
    assert set(state.norms) == {b"a", b"b", b"c"} and set(state2.clipped) == {b"a", b"b"}
    # a plain key becomes a sequence of its own
    seen.clear()
    agg = fedjax_amd.aggregators.dp_clipped_mean_aggregator(0.5, 1.1, fjr.PRNGKey(11))
    agg.apply(clients, agg.init())
    assert np.array_equal(seen[0][3], k1)


def test_aggregator_state_keeps_its_shape():
    """The clipped aggregator's state still builds from three fields; noise_stddev is structure."""
    from fedjax_amd import pytree
    s3 = fedjax_amd.aggregators.ClippedMeanAggregatorState({}, {}, {})
    assert s3.noise_stddev is None
    s4 = s3.replace(noise_stddev=0.5)
    assert len(pytree.flatten(s3)[0]) == len(pytree.flatten(s4)[0])
    with pytest.raises(ValueError):
        fedjax_amd.aggregators.dp_clipped_mean_aggregator(1.0, -1.0, KEY)


def test_leaf_key_schedule_is_split(monkeypatch):
    """keys = split(key, L), jax leaf order (compression.py:105-122's schedule): what both routes
    hand the kernels."""
    for L in (1, 2, 5):
        assert np.array_equal(fjr.split(KEY, L), jr.split(KEY, L))
    seen = {}

    class Stop(Exception):
        pass

    def table(stddev, begins, sizes, keys, device=None):
        seen.update(stddev=stddev, begins=list(begins), sizes=list(sizes), keys=np.array(keys))
        raise Stop

    monkeypatch.setattr(kernels, "NoiseTable", table)
    monkeypatch.setattr(slab_mod.ClientDeltaSlab, "weight_vector", lambda self, w: None)
    with pytest.raises(Stop):
        cpu_slab().dp_clipped_mean([1.0, 2.0], 1.0, 0.25, KEY)
    assert seen["begins"] == [0, 3] and seen["sizes"] == [3, 4] and seen["stddev"] == 0.25
    assert np.array_equal(seen["keys"], jr.split(KEY, 2))


# ------------------------------------------------------------------------- the restatement
def test_restated_normal_moments():
    n = 1 << 20
    assert nr.SPAN == np.float32(2.0) and float(np.float32(1.0) - nr.LO) == 2.0
    z = nr.normal(jr.prng_key(7), (n,))
    assert z.dtype == np.float32 and np.isfinite(z).all()
    z64 = z.astype(np.float64)
    mean, var = z64.mean(), z64.var()
    print(f"restated normal: |mean| = {abs(mean):.3e} (< {5 / np.sqrt(n):.3e}), "
          f"|var - 1| = {abs(var - 1):.3e} (< {5 * np.sqrt(2 / n):.3e})")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)


def test_restated_normal_extremes_are_finite():
    bits = np.array([0, 1 << 9, 0x1FF, 0x80000000, 0xFFFFFFFF, 0xFFFFFE00], np.uint32)
    u = nr.uniform_from_bits(bits)
    assert u[0] == nr.LO and u[2] == nr.LO and (np.abs(u) < 1).all()
    z = nr.normal_from_bits(bits)
    assert np.isfinite(z).all() and z[0] < -5 and z[-1] > 5 and 0 < z[3] < 1e-7  # u = 2^-24 at f = 1/2
    assert nr.ulp_distance(np.array([1.0, -0.0], np.float32), np.array([np.nextafter(np.float32(1), 2), 0.0], np.float32)
                           ).tolist() == [1, 0]
