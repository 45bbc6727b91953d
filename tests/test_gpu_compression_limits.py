"""Directed edges of the compression kernels (fedjax_amd/csrc/fjcomp.hip) that the seeded sweep
(tests/test_gpu_compression_fuzz.py) cannot be relied on to reach, each at the smallest shape
that still reaches it: the level-table and histogram thresholds of k_quant_fold, its histogram
grouping, three-pass Walsh-Hadamard rotations, unaligned workspace interiors with a short last
batch, batches across the 256-client staging, degenerate statistics, the accuracy of sigma
against a plain float64 reference, and the refusals.

Bar: as in the sweep (means NaN where the oracle's are and bitwise equal elsewhere, num_bits equal
as float32, rng equal), except where a test says otherwise and why.
"""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import fedjax_amd
from fedjax_amd import _compress as C
from fedjax_amd import _lib
from fedjax_amd.aggregators import compression as comp
from fedjax_amd.aggregators import walsh_hadamard as wh
from oracle import compression_ref as cref
from oracle import jax_random_ref as jr
from tests.compression_cases import per_client_bytes
from tests.test_gpu_compression_fuzz import assert_same_bits_count, assert_same_mean

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def fleet(shapes, K, seed, cuda, edit=None):
    """(device clients, oracle clients): K clients of {name: normal * 0.01}; ``edit(k, tree)``
    changes client k's numpy tree in place first."""
    rs = np.random.RandomState(seed)
    trees = [{n: (rs.standard_normal(s) * 0.01).astype(F32) for n, s in shapes.items()} for _ in range(K)]
    if edit is not None:
        for k, t in enumerate(trees):
            edit(k, t)
    w = [int(v) for v in rs.randint(1, 500, K)]
    return ([(f"c{k}", {n: dev(v, cuda) for n, v in t.items()}, w[k]) for k, t in enumerate(trees)],
            [(f"c{k}", t, w[k]) for k, t in enumerate(trees)])


def build(kind, key, levels=4, ws=None):
    """(product aggregator, oracle (init, apply)) of one kind."""
    kw = {} if ws is None else {"workspace_bytes": ws}
    if kind in ("uniform", "uniform_arith"):
        enc = "arithmetic" if kind == "uniform_arith" else None
        return (comp.uniform_stochastic_quantizer(levels, key, enc), cref.uniform_stochastic_quantizer(levels, key, enc))
    if kind == "rotated":
        return (comp.rotated_uniform_stochastic_quantizer(levels, key, **kw),
                cref.rotated_uniform_stochastic_quantizer(levels, key, commute_inverse=True))
    if kind == "drive":
        return comp.structured_drive_quantizer(key, **kw), cref.structured_drive_quantizer(key)
    return comp.terngrad_quantizer(key), cref.terngrad_quantizer(key)


def check(kind, clients, ref_clients, key, *, levels=4, ws=None, rounds=1):
    """Run ``rounds`` rounds of both; returns the oracle's last mean."""
    q, (init, apply) = build(kind, key, levels, ws)
    st, rst = q.init(), init()
    for r in range(rounds):
        p, st = q.apply(iter(clients), st)
        with np.errstate(all="ignore"):
            rp, rst = apply(ref_clients, rst)
        assert sorted(p) == sorted(rp)
        for n in rp:
            assert_same_mean(host(p[n]), rp[n], f"{kind} round {r} leaf {n}")
        assert_same_bits_count(st.num_bits, rst.num_bits, f"{kind} round {r}")
        npt.assert_array_equal(np.asarray(st.rng, np.uint32), rst.rng)
    return rp


# ------------------------------------------------------------------ level thresholds
@pytest.mark.parametrize("enc", [None, "arithmetic"])
@pytest.mark.parametrize("levels", [1, 2, 4095, 4096, 4097, 65536])
def test_level_thresholds(levels, enc, cuda):
    """UniformTQ at its last sizes (4095, 4096: a 64 KiB level table), UniformQ above, the LDS
    histogram up to 4096 bins (hist_group == 1 at 2048..4095 levels) and global atomics above,
    and a single level (lm1 = 0: every quantized value is NaN, here and in the oracle)."""
    clients, ref_clients = fleet({"a": (3,), "w": (1000,)}, 3, levels, cuda)
    rp = check("uniform_arith" if enc else "uniform", clients, ref_clients, jr.prng_key(levels), levels=levels, rounds=2)
    assert np.isnan(rp["w"]).all() == (levels == 1)


@pytest.mark.parametrize("levels", [4096, 4097, 65536])
def test_single_leaf_levels(levels, cuda):
    v = (np.random.RandomState(levels).standard_normal(65537) * 0.1).astype(F32)
    key = jr.prng_key(levels + 1)
    got = host(comp.uniform_stochastic_quantize(dev(v, cuda), levels, key))
    assert_same_mean(got, cref.uniform_stochastic_quantize(v, levels, key), f"{levels} levels")
    assert len(np.unique(got)) > min(levels, 65537) // 8  # the levels are in use


@pytest.mark.parametrize("levels", [2, 257, 2049, 4097, 65537])
def test_draw_equal_to_the_threshold(levels, cuda):
    """``where(rand > threshold, floor, ceil)``: a draw equal to the threshold picks the ceiling.
    A random input meets that tie about once in 2^23 elements, so the input is built from the
    draws themselves. With v_min = 0, v_max = 1 and num_levels - 1 = lm1 a power of two, every
    step of the quantizer is exact for v = (j + t) / lm1 with j in {0, 1} and t a multiple of
    2^-23 below 1: a = v, floor = j and threshold = t. A third of the elements have t = u (the
    element's own draw: ceiling), a third t = u + 2^-23 (ceiling) and a third t = u - 2^-23
    (floor). Both the level table (lm1 <= 2048) and the per-element division (above) are run."""
    n, lm1 = 4099, levels - 1
    key = jr.prng_key(levels)
    u = jr.uniform(key, (n,)).astype(np.float64)
    assert (u * 2.0 ** 23 == np.round(u * 2.0 ** 23)).all()
    step = (np.arange(n) % 3 - 1) * 2.0 ** -23  # -1, 0, +1 units in turn
    t = u + step
    t = np.where((t < 0) | (t >= 1), u, t)
    step = t - u
    j = (np.arange(n) // 3 % 2).astype(np.float64) if lm1 > 1 else np.zeros(n)
    v64 = (j + t) / lm1
    v = v64.astype(F32)
    assert (v.astype(np.float64) == v64).all()  # exactly representable
    want = (np.where(step < 0, np.floor(j + t), np.ceil(j + t)) / lm1).astype(F32)
    assert (step == 0).sum() > n // 4 and (np.ceil(j + t) != np.floor(j + t)).sum() > n - 8
    got = host(comp.uniform_stochastic_quantize(dev(v, cuda), levels, key, 0.0, 1.0))
    npt.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    npt.assert_array_equal(cref.uniform_stochastic_quantize(v, levels, key, 0.0, 1.0).view(np.uint32),
                           want.view(np.uint32))
    if levels == 2:  # binary_stochastic_quantize: where(rand > a, v_min, v_max), a = t
        got = host(comp.binary_stochastic_quantize(dev(v, cuda), key, 0.0, 1.0))
        npt.assert_array_equal(got, np.where(step < 0, 0.0, 1.0).astype(F32))


# ------------------------------------------------------------------ histogram grouping
def oracle_levels(v, num_levels, key):
    """The level index uniform_stochastic_quantize (oracle/compression_ref.py) picks per element."""
    v = np.asarray(v, F32)
    v_min, v_max, lm1 = F32(np.min(v)), F32(np.max(v)), F32(num_levels - 1)
    with np.errstate(all="ignore"):
        a = cref.nan_to_num((v - v_min) / (v_max - v_min))
        a = np.maximum(F32(0), np.minimum(a, F32(1))).astype(F32)
        ce, fl = np.ceil(a * lm1), np.floor(a * lm1)
        v_ceil, v_floor = (ce / lm1).astype(F32), (fl / lm1).astype(F32)
        thr = cref.nan_to_num((a - v_floor) / (v_ceil - v_floor))
        return np.where(jr.uniform(key, v.shape) > thr, fl, ce).astype(np.int64)


@pytest.mark.parametrize("levels", [2, 1366, 2047])
def test_histogram_grouping(levels, cuda):
    """hist_group = 4096 // (num_levels + 1) clients share one LDS zero / count / flush cycle:
    1365, 2 and 2 here, against 257 clients (a last group of 257 % group clients, and the
    256-client staging inside a group). The per-client bit counts reach num_bits; the raw
    histogram is compared too, so that an error the mean over clients cancels cannot hide."""
    K, n = 257, 513
    clients, ref_clients = fleet({"w": (n,)}, K, levels, cuda)
    key = jr.prng_key(100 + levels)
    check("uniform_arith", clients, ref_clients, key, levels=levels)
    # the same round's keys: the aggregator's chain (oracle/compression_ref.py:263-267)
    _, use = jr.split(key)
    seq = jr.PRNGSequence(use)
    leaf_keys = np.stack([jr.split(next(seq), 1) for _ in range(K)])  # [K, 1, 2]
    rows = [[t["w"]] for _, t, _ in clients]
    out = torch.empty(n, dtype=torch.float32, device=cuda)
    h, _ = C.quantized_mean(_lib.COMP_UNIFORM, rows, leaf_keys, np.ones(K, F32), None, [out], num_levels=levels,
                            hist=True)
    got = host(h).reshape(K, levels + 1)
    want = np.stack([np.bincount(oracle_levels(t["w"], levels, leaf_keys[k, 0]), minlength=levels + 1)
                     for k, (_, t, _) in enumerate(ref_clients)])
    npt.assert_array_equal(got, want)
    assert (got.sum(axis=1) == n).all() and not got[:, -1].any()


# ------------------------------------------------------------------ three-pass rotations
N3 = (1 << 21) + 1  # pads to d = 2^22: Walsh-Hadamard passes of 13, 8 and 1 butterfly bits


@pytest.fixture(scope="module")
def big_clients():
    rs = np.random.RandomState(22)
    return [(f"c{k}", {"w": (rs.standard_normal(N3) * 0.01).astype(F32)}, w) for k, w in enumerate((3, 5))]


def test_three_pass_rotation_and_inverse(big_clients, cuda):
    x = big_clients[0][1]["w"]
    key = jr.prng_key(21)
    y, s = wh.structured_rotation(dev(x, cuda), key)
    ey, es = cref.structured_rotation(x, key)
    assert ey.size == 1 << 22 and tuple(s.tolist()) == es
    npt.assert_array_equal(host(y).view(np.uint32), ey.view(np.uint32))
    z = wh.inverse_structured_rotation(y, key, s)
    npt.assert_array_equal(host(z).view(np.uint32), cref.inverse_structured_rotation(ey, key, es).view(np.uint32))


@pytest.mark.parametrize("kind", ["rotated", "drive"])
def test_three_pass_aggregators(kind, big_clients, cuda):
    """ROTATE (zero padding, signs, last-pass tile partials), UNROTATE and UNROTATE_DRIVE at three
    passes, K = 2 clients of 16 MiB."""
    clients = [(c, {"w": dev(t["w"], cuda)}, w) for c, t, w in big_clients]
    check(kind, clients, big_clients, jr.prng_key(23), levels=4)


@pytest.mark.parametrize("sums", [False, True])
def test_three_pass_tile_partials_equal_row_stats(sums, big_clients, cuda):
    """The last pass's per-tile partials at d = 2^22 (512 tiles of the 1-bit pass) give the same
    min / max / absmax and qparams bytes as a k_row_stats pass over the rotated row."""
    x = dev(big_clients[1][1]["w"], cuda)
    d = 1 << 22
    key = jr.split(jr.prng_key(24), 1)
    signs, woff = C.rademacher_words(key, [d], cuda)
    y = torch.empty(d, dtype=torch.float32, device=cuda)
    tiles = C.wht_tiles(22, C.wht_passes(22) - 1)
    assert C.wht_passes(22) == 3 and tiles == 512
    pre = np.array([0, tiles], dtype=np.int64)
    slot = int(_lib.load().fjcomp_row_stats_workspace_bytes(1))
    part = torch.empty(tiles * slot, dtype=torch.uint8, device=cuda)
    yp = np.array([y.data_ptr()], dtype=np.uint64)
    keep = C.run_wht(C.wht_jobs([x.data_ptr()], yp, yp, [d], kind=_lib.WHT_ROTATE, n_in=[N3],
                                signs=[signs.data_ptr()], stats=[part.data_ptr()],
                                flags=C.WHT_F_SUMS if sums else 0), cuda)
    st_a, qp_a, up = C.stats_from_partials(yp, [d], pre, part, _lib.COMP_UNIFORM, cuda)
    st_b, qp_b = C.row_stats_table(yp, [d], _lib.COMP_UNIFORM, cuda)
    torch.cuda.synchronize()
    del keep, up
    a, b = host(st_a).view(C.STATS), host(st_b).view(C.STATS)
    for f in ("min", "max", "absmax"):
        npt.assert_array_equal(a[f].view(np.uint64), b[f].view(np.uint64), err_msg=f)
    npt.assert_array_equal(host(qp_a), host(qp_b))
    ey = cref.structured_rotation(big_clients[1][1]["w"], key[0])[0]
    assert a["min"][0] == ey.min() and a["max"][0] == ey.max()
    for f in ("sumsq", "sumabs"):  # f64 sums in tile order vs chunk order
        if sums:
            npt.assert_allclose(a[f], b[f], rtol=1e-13, err_msg=f)
        else:
            assert not a[f].any()


# ------------------------------------------------------------------ unaligned interiors, batches
UNALIGNED = {"a": (1,), "b": (3,), "c": (8193,), "d": (2,), "e": (4097,)}


@pytest.mark.parametrize("kind", ["rotated", "drive"])
def test_unaligned_interiors_short_last_batch(kind, cuda):
    """Leaves of 1, 3 and 2 elements take every later Y / Z / acc row and sign word off 16-byte
    alignment (k_wht's scalar load and store paths, n_out ending inside a quad); K = 5 in batches
    of 2 leaves a short last batch with accumulate and the deferred scale."""
    clients, ref_clients = fleet(UNALIGNED, 5, 7, cuda)
    ws = 2 * per_client_bytes(kind, [int(np.prod(s)) for s in UNALIGNED.values()])
    assert C._batch_size(5, ws // 2, ws) == 2
    check(kind, clients, ref_clients, jr.prng_key(31), levels=4, ws=ws, rounds=2)


def test_batches_across_the_staging_boundary(cuda):
    """K = 260 in batches of 129, 129 and 2: k_quant_fold accumulates across launches whose
    client ranges do not line up with its 256-client staging."""
    shapes = {"b": (17,), "w": (3001,)}
    clients, ref_clients = fleet(shapes, 260, 9, cuda)
    ws = 129 * per_client_bytes("rotated", [17, 3001])
    assert C._batch_size(260, ws // 129, ws) == 129
    check("rotated", clients, ref_clients, jr.prng_key(32), levels=4, ws=ws)


# ------------------------------------------------------------------ degenerate statistics
DEGEN = {"b": (17,), "w": (300,)}


@pytest.mark.parametrize("kind", ["uniform", "rotated"])
def test_constant_leaf(kind, cuda):
    """uniform: range == 0 and rcp_range == inf in every client's row, and the mean is the
    constant. rotated: the same leaf through the rotation (300 values padded to 512)."""
    def edit(k, t):
        t["w"][:] = 0.75
    clients, ref_clients = fleet(DEGEN, 3, 1, cuda, edit)
    rp = check(kind, clients, ref_clients, jr.prng_key(41), levels=5, rounds=2)
    if kind == "uniform":
        npt.assert_array_equal(rp["w"], np.full(300, 0.75, F32))


@pytest.mark.parametrize("kind", ["terngrad", "drive"])
def test_all_zero_leaf_of_one_client(kind, cuda):
    """terngrad: sigma = 0, thr = 0, vmax = 0. DRIVE: 0 / 0 makes that client's leaf NaN and so
    the mean; that is the oracle's (the reference's) behaviour too, pinned here."""
    def edit(k, t):
        if k == 1:
            t["w"][:] = 0.0
    clients, ref_clients = fleet(DEGEN, 3, 2, cuda, edit)
    rp = check(kind, clients, ref_clients, jr.prng_key(42))
    assert np.isnan(rp["w"]).all() == (kind == "drive") and np.isfinite(rp["b"]).all()


@pytest.mark.parametrize("kind", ["uniform", "uniform_arith", "rotated", "drive", "terngrad"])
def test_one_nan_in_one_client(kind, cuda):
    """The NaN takes its (client, leaf) row's statistics and the mean of that leaf is NaN (terngrad:
    sigma and vmax are NaN, every other element quantizes to 0 and only the NaN's own place is
    NaN); the other leaf is untouched. With arithmetic coding the row's counts land in the NaN
    bin, which feeds arithmetic_bits_host's slow branch from a real histogram."""
    def edit(k, t):
        if k == 2:
            t["w"][123] = np.nan
    clients, ref_clients = fleet(DEGEN, 3, 3, cuda, edit)
    rp = check(kind, clients, ref_clients, jr.prng_key(43), levels=5, rounds=2)
    nan = np.isnan(rp["w"])
    assert nan[123] and (nan.all() or kind == "terngrad") and np.isfinite(rp["b"]).all()


@pytest.mark.parametrize("value", [np.inf, -np.inf])
@pytest.mark.parametrize("kind", ["uniform", "uniform_arith"])
def test_inf_in_one_client(kind, value, cuda):
    """range == inf, rcp_range == 0."""
    def edit(k, t):
        if k == 0:
            t["w"][7] = value
    clients, ref_clients = fleet(DEGEN, 3, 4, cuda, edit)
    check(kind, clients, ref_clients, jr.prng_key(44), levels=5, rounds=2)


def test_constant_leaf_with_inexact_sums(cuda):
    """A constant leaf c = 0.1 over n = 3001 elements: the exact variance is 0 and a one-pass
    float64 variance is the rounding noise of its two sums, which depends on their order, so this
    is not compared bitwise (the kernel, which sums x - x[0], gives exactly 0; the oracle does not). var = s2/n - (s1/n)^2 with each term c^2 (1 + O(n 2^-53)), so var <=
    about c^2 n 2^-52, sigma <= c sqrt(n 2^-52) and every output magnitude (0 or
    min(|x|, 2.5 sigma)) is at most 2.5 c sqrt(n 2^-52). Signs follow the inputs."""
    c, n = 0.1, 3001
    bound = 2.5 * c * math.sqrt(n * 2.0 ** -52)
    for sign in (1.0, -1.0):
        v = np.full(n, sign * c, F32)
        got = host(comp.terngrad_quantize(dev(v, cuda), jr.prng_key(5)))
        print(f"constant {sign * c}: max |out| = {np.abs(got).max():.3e}, bound {bound:.3e}")
        assert np.isfinite(got).all() and np.abs(got).max() <= bound
        nz = got != 0
        assert (np.sign(got[nz]) == sign).all()
    with np.errstate(all="ignore"):
        assert np.abs(cref.terngrad_quantize(np.full(n, c, F32), jr.prng_key(5))).max() <= bound  # the oracle too


# ------------------------------------------------------------------ sigma accuracy
@pytest.mark.parametrize("ratio", [0, 1, 1e3, 1e5])
@pytest.mark.parametrize("n", [17, 3001, 147456])
def test_sigma_against_two_pass_f64(n, ratio, cuda):
    """the float64 sigma is at least as accurate as a two-pass float32 std for
    |mean| / sigma up to 1e5. Reference: a two-pass float64 std of the same float32 data; allowed
    error: that of numpy's two-pass float32 std of that data (measured here), or 2 ulp.

    Summing the plain x and x^2 missed this at (147456, 1e5): 4.2e-8 against 1.4e-8 allowed (the
    oracle's numpy order of the same formula: 9.6e-9); k_row_stats now sums x - x[0]."""
    rs = np.random.RandomState(n + int(ratio))
    x = (rs.standard_normal(n) * 0.01 + 0.01 * ratio).astype(F32)
    t = dev(x, cuda)
    _, qp = C.row_stats([(t.data_ptr(), n)], _lib.COMP_TERNGRAD, cuda)
    thr = np.frombuffer(host(qp).tobytes(), dtype=C.QPARAMS)["thr"][0]
    x64 = x.astype(np.float64)
    sigma64 = math.sqrt(((x64 - x64.mean()) ** 2).mean())
    err32 = abs(float(np.std(x, dtype=F32)) - sigma64)
    ulp = float(np.spacing(F32(sigma64)))
    err = abs(float(thr) / 2.5 - sigma64)
    err_oracle = abs(float(cref.std_f32(x)) - sigma64)
    print(f"n={n} ratio={ratio:g}: |thr/2.5 - s64| = {err:.3e} (oracle {err_oracle:.3e}), f32 two-pass {err32:.3e}, "
          f"2 ulp {2 * ulp:.3e}")
    assert err <= max(err32, 2 * ulp)
    assert err_oracle <= max(err32, 2 * ulp)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind", ["uniform", "rotated", "drive", "terngrad"])
def test_empty_leaf_refused(kind, cuda):
    q, _ = build(kind, jr.prng_key(0))
    clients = [(f"c{k}", {"a": torch.zeros(0, device=cuda), "w": torch.ones(4, device=cuda)}, 1) for k in range(2)]
    with pytest.raises(ValueError, match="empty"):
        q.apply(clients, q.init())


def test_empty_array_refused_by_the_single_leaf_quantizers(cuda):
    e = torch.zeros(0, device=cuda)
    for call in (lambda: comp.uniform_stochastic_quantize(e, 4, jr.prng_key(0)),
                 lambda: comp.binary_stochastic_quantize(e, jr.prng_key(0)),
                 lambda: comp.terngrad_quantize(e, jr.prng_key(0))):
        with pytest.raises(ValueError, match="empty"):
            call()


def test_histogram_too_large_refused(cuda):
    """K * L * (num_levels + 1) > 2^28 with arithmetic coding: 4096 clients of one 1-element leaf
    at 65536 levels reach the check; nothing of that size is allocated."""
    buf = torch.ones(4096, device=cuda)
    clients = [("c", {"w": buf[k:k + 1]}, 1) for k in range(4096)]
    assert 4096 * 1 * 65537 > 1 << 28
    q = comp.uniform_stochastic_quantizer(65536, jr.prng_key(0), "arithmetic")
    with pytest.raises(ValueError, match="histogram too large"):
        q.apply(clients, q.init())
    q = comp.uniform_stochastic_quantizer(65536, jr.prng_key(0))  # without the histogram it runs
    p, _ = q.apply(clients, q.init())
    assert host(p["w"]).shape == (1,)


def test_zero_levels_refused(cuda):
    q = comp.uniform_stochastic_quantizer(0, jr.prng_key(0))
    with pytest.raises(_lib.FjaggError, match="num_levels=0"):
        q.apply([("c", {"w": torch.ones(4, device=cuda)}, 1)], q.init())
    with pytest.raises(_lib.FjaggError, match="num_levels=0"):
        comp.uniform_stochastic_quantize(torch.ones(4, device=cuda), 0, jr.prng_key(0))


def test_bad_flags_refused(cuda, monkeypatch):
    """fjcomp_quant_fold takes FJAGG_SCALE and FJAGG_ACCUMULATE only."""
    x = torch.ones(8, device=cuda)
    out = torch.empty(8, device=cuda)
    _, qp = C.row_stats([(x.data_ptr(), 8)], _lib.COMP_UNIFORM, cuda)
    args = (_lib.COMP_UNIFORM, np.array([[x.data_ptr()]], np.uint64), np.zeros((1, 1, 2), np.uint32), qp.data_ptr(),
            np.ones(1, F32), np.array([8]), np.array([out.data_ptr()], np.uint64), cuda)
    C.quant_fold(*args, num_levels=4, scale=1.0)  # the call is well formed
    monkeypatch.setattr(_lib, "SCALE", _lib.NONTEMPORAL)
    with pytest.raises(_lib.FjaggError, match="unsupported flags"):
        C.quant_fold(*args, num_levels=4, scale=1.0)
    torch.cuda.synchronize()
