"""Limit, scan-edge and concurrency tests of the top-k sparsified mean on the GPU. Everything is
compared bit for bit with the numpy restatement (tests/topk_ref.py): thresholds raw, sent as int32,
means with every NaN as one pattern. Every select is also held to the definition itself by
comparisons alone (topk_cases.check_definition, on the device's own T and the host copy of the
rows), which shares no failure mode with the reference's sort. Cases are tests/topk_cases.py's;
tests/test_topk_cases.py shows on the CPU that they reach what they are for.

a. staircases: every lane of k_topk_scan is the finder at every position of its slice, at each
   level, lane 0 (inf / NaN patterns at level 0) and lane 255 included; ranks 1, 2, 3 inside the
   picked bin; the mean at two keep counts per level; the tree route over three unaligned leaves.
b. the definition check: `checked_select` below, applied to every select here and in the sweep.
c. `scaled`: the clients of one call differ in their level-0 digit, hence in every prefix and rank.
d. counts past 16 bits: 81 921 keys in one bin at every level; P = 2^20 + 1 (65 chunks).
e. the K axis: every K from 1 to 34 (client 0, batches of eight, tail), weights with a negative, a
   zero and, in a second pass, an inf; K = 1024 and K = 4096, the entry's limit.
f. the slab's own padding filled with NaN and inf: never read, never written.
g. the workspace: a caller's 0xFF-filled buffer of the exact size, reused; K up and down on one
   stream; two streams at once; eighteen streams past the cache's 16 entries; repeatability.
h. metamorphic relations that need no reference: column permutation, sign flip, scaling by 2^5.
i. a captured round whose keep count makes T = 0 for some clients only, replayed over a staircase
   and over equal keys."""
import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels
from tests import topk_cases as tc
from tests import topk_ref as ref
from tests.test_gpu_topk import assert_bits, assert_select, host, run_tree_and_slab, slab_of, ubits

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
CH = kernels.TOPK_CHUNK
STAIRS = [(level, mult) for level in tc.STAIR_LEVELS for mult in tc.STAIR_MULTS]
FINITE_W = [3, -1.5, 0, 2.25, 1, 7, 0.5]  # every prefix sums to more than 0


def checked_select(thr, sent, want, rows, c, what):
    """A device select against the reference (raw bits) and against the definition (comparisons only)."""
    assert_select(thr, sent, want, what)
    tc.check_definition(host(thr), host(sent), rows, c, what)


def raw(t):
    return np.ascontiguousarray(host(t)).view(np.uint32).ravel().copy()


def weights(K, inf_at=None):
    w = [float(v) for v in (FINITE_W * (K // len(FINITE_W) + 1))[:K]]
    if inf_at is not None:
        w[inf_at] = float("inf")
    return w


def mean_three_ways(s, x, w, c, dev, what, exact_fold=True):
    """slab.topk_mean against the reference, the definition and slab.mean over the masked rows."""
    got = s.topk_mean(w, c)
    mean, T, sent = ref.topk_mean_rows(list(x), w, c)
    checked_select(got.thresholds, got.sent, (T, sent), x, c, what)
    assert_bits(got.mean[0], mean, what + ": mean")
    if exact_fold:
        masked = slab_of(np.stack([ref.mask_row(r, t) for r, t in zip(x, T)]), dev)
        assert_bits(got.mean[0], masked.mean(w)[0], what + ": slab.mean over the masked rows")
    return got


# ------------------------------------------------------------------ a. staircases
@pytest.mark.parametrize("level,mult", STAIRS)
def test_staircase_thresholds(cuda, level, mult):
    x = tc.staircase(level, mult, np.random.RandomState(300 + 10 * level + mult))
    s = slab_of(x, cuda)
    cs = tc.staircase_counts(level, mult)
    want = ref.select_many(list(x), cs)
    picked, compared = set(), 0
    for c in cs:
        thr, sent = s.topk_thresholds(c)
        checked_select(thr, sent, want[c], x, c, f"staircase level {level} x{mult} c={c}")
        picked |= set(tc.stair_digit(raw(thr), level).tolist())
        compared += 1
    assert compared == len(cs) == (tc.stair_bins(level) // 256) * (3 if mult == 3 else 1)
    assert picked == set(range(tc.stair_bins(level)))  # (follows from the comparisons; tests/test_topk_cases.py)
    assert_bits(s.rows, x, "the slab was written")


@pytest.mark.parametrize("level", tc.STAIR_LEVELS)
def test_staircase_mean(cuda, level):
    x = tc.staircase(level, 1, np.random.RandomState(320 + level))
    s = slab_of(x, cuda)
    cs = tc.staircase_counts(level, 1)
    for c in (cs[0], cs[-1]):
        mean_three_ways(s, x, weights(256), c, cuda, f"staircase level {level} c={c}")
    if level == 0:  # 256 rows of NaN patterns leave few finite coordinates: four rows leave most
        y = np.ascontiguousarray(x[:4])
        for c in (cs[0], cs[-1]):
            mean_three_ways(slab_of(y, cuda), y, weights(4), c, cuda, f"staircase level 0, four rows, c={c}")
            assert np.isfinite(ref.topk_mean_rows(list(y), weights(4), c)[0]).sum() > y.shape[1] // 2
    assert_bits(s.rows, x, "the slab was written")


@pytest.mark.parametrize("level", tc.STAIR_LEVELS)
def test_staircase_through_the_tree_route(cuda, level):
    x = tc.staircase(level, 1, np.random.RandomState(340 + level))
    cuts = (0, 5, 1030, x.shape[1])  # three leaves at unaligned cuts
    trees = [{n: np.ascontiguousarray(r[a:b]) for n, a, b in zip("abc", cuts, cuts[1:])} for r in x]
    cs = tc.staircase_counts(level, 1)
    for c, offsets in ((cs[0], (0, 0)), (cs[-1], (1, 0, 2))):
        a, s = run_tree_and_slab(trees, weights(256), c, cuda, offsets=offsets, what=f"staircase level {level} c={c}")
        tc.check_definition(host(a.thresholds), host(a.sent), x, c, f"staircase level {level} c={c}: tree")


# ------------------------------------------------------------------ c. per-client prefixes
@pytest.mark.parametrize("K,P", [(16, 257), (64, 257), (16, CH + 1), (64, CH + 1)])
def test_scaled_clients_each_have_their_own_prefix(cuda, K, P):
    x = tc.family("scaled", K, P, np.random.RandomState(400 + K + P))
    s = slab_of(x, cuda)
    cs = ref.keep_counts(P)
    want = ref.select_many(list(x), cs)
    for c in cs:
        assert len(set(tc.stair_digit(want[c][0], 0).tolist())) >= 8, "distinct level-0 digits in one call"
        thr, sent = s.topk_thresholds(c)
        checked_select(thr, sent, want[c], x, c, f"scaled K={K} P={P} c={c}")
    mean_three_ways(s, x, weights(K), P // 10, cuda, f"scaled K={K} P={P} mean")
    assert_bits(s.rows, x, "the slab was written")


# ------------------------------------------------------------------ d. counts past 16 bits
@pytest.mark.parametrize("name", sorted(tc.LIMIT_ROWS))
def test_counts_past_sixteen_bits(cuda, name):
    x = tc.limit_rows(name)
    P = x.shape[1]
    s = slab_of(x, cuda)
    cs = tc.limit_counts(P)
    want = ref.select_many(list(x), cs)
    for c in cs:
        thr, sent = s.topk_thresholds(c)
        checked_select(thr, sent, want[c], x, c, f"{name} P={P} c={c}")
    if name == "equal":
        assert all(int(want[c][1][k]) == P for c in cs for k in range(2))  # every key ties: all are sent
    mean_three_ways(s, x, [2.0, -0.75], 65537, cuda, f"{name} P={P} mean")
    assert_bits(s.rows, x, "the slab was written")


# ------------------------------------------------------------------ e. the K axis
@pytest.mark.parametrize("name", ("five", "gauss"))
def test_every_k_from_1_to_34(cuda, name):
    rng = np.random.RandomState(500 + len(name))
    P, compared = 257, 0
    for K in range(1, 35):
        x = tc.family(name, K, P, rng)
        s = slab_of(x, cuda)
        mean_three_ways(s, x, weights(K), P // 10, cuda, f"{name} K={K}")
        # an inf weight in the tail (or alone): a masked coordinate times inf is NaN in the contract as well
        mean_three_ways(s, x, weights(K, inf_at=K - 1), P // 10, cuda, f"{name} K={K}, inf weight")
        if K >= 10:  # and inside the first batch of eight
            mean_three_ways(s, x, weights(K, inf_at=4), P // 10, cuda, f"{name} K={K}, inf weight in the batch")
        compared += 1
    assert compared == 34


@pytest.mark.parametrize("K,P", [(1024, 1025), (4096, 1), (4096, 257)])
def test_many_clients(cuda, K, P):
    assert K <= kernels.TOPK_MAX_CLIENTS
    x = tc.family("five" if P > 1 else "gauss", K, P, np.random.RandomState(K + P))
    s = slab_of(x, cuda)
    cs = ref.keep_counts(P)
    want = ref.select_many(list(x), cs)
    for c in cs:
        thr, sent = s.topk_thresholds(c)
        checked_select(thr, sent, want[c], x, c, f"K={K} P={P} c={c}")
    mean_three_ways(s, x, weights(K), max(1, P // 10), cuda, f"K={K} P={P} mean", exact_fold=False)
    assert_bits(s.rows, x, "the slab was written")


# ------------------------------------------------------------------ f. the slab's padding
@pytest.mark.parametrize("P", (257, CH + 5))
def test_slab_padding_is_neither_read_nor_written(cuda, P):
    K = 5
    x = tc.family("five", K, P, np.random.RandomState(600 + P))
    s = slab_of(x, cuda)
    assert s.row_stride == s.num_params + 3 == P + 3 and tuple(s.storage.shape) == (K, P + 3)
    cs, w = ref.keep_counts(P), weights(K)
    want = ref.select_many(list(x), cs)
    mean = ref.topk_mean_rows(list(x), w, P // 10)[0]
    for fill in (0.0, float("nan"), float("inf"), -float("inf")):
        s.storage[:, P:] = fill
        pad = raw(s.storage[:, P:])
        for c in cs:
            thr, sent = s.topk_thresholds(c)
            checked_select(thr, sent, want[c], x, c, f"padding {fill} P={P} c={c}")
        got = s.topk_mean(w, P // 10)
        assert_select(got.thresholds, got.sent, want[P // 10], f"padding {fill} P={P} mean")
        assert_bits(got.mean[0], mean, f"padding {fill} P={P}: mean")
        assert raw(s.storage[:, P:]).tolist() == pad.tolist(), f"padding {fill}: the padding was written"
        assert_bits(s.rows, x, "the slab was written")


# ------------------------------------------------------------------ g. the workspace
def test_callers_dirty_workspace_of_the_exact_size(cuda):
    K, P = 7, CH + 37
    x = tc.family("five", K, P, np.random.RandomState(700))
    xd = torch.from_numpy(x).to(cuda)
    need = int(_lib.load().fjcomp_topk_workspace_bytes(K))
    assert need == K * (2048 + 2) * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
    w = weights(K)
    wd = torch.tensor(w, dtype=torch.float32, device=cuda)
    scale = float(np.float32(1.0 / sum(w)))
    stream = kernels._stream_handle(cuda)

    def select(c):
        thr = torch.empty(K, dtype=torch.float32, device=cuda)
        sent = torch.empty(K, dtype=torch.int32, device=cuda)
        _lib.call("fjcomp_topk_select_dense", _lib.F32, xd.data_ptr(), P, K, P, c, thr.data_ptr(), sent.data_ptr(),
                  ws.data_ptr(), need, stream)
        return thr, sent

    def mean(c):
        thr = torch.empty(K, dtype=torch.float32, device=cuda)
        sent = torch.empty(K, dtype=torch.int32, device=cuda)
        out = torch.full((P,), float("nan"), dtype=torch.float32, device=cuda)
        _lib.call("fjcomp_topk_mean_dense", _lib.F32, xd.data_ptr(), P, K, P, c, wd.data_ptr(), scale, out.data_ptr(),
                  thr.data_ptr(), sent.data_ptr(), ws.data_ptr(), need, stream)
        return out, thr, sent

    for c in (P // 10, 2):  # the second call finds the first one's prefixes and ranks
        thr, sent = select(c)
        checked_select(thr, sent, ref.select(list(x), c), x, c, f"0xFF workspace, select c={c}")
    ws.fill_(0xFF)
    for c in (P - 1, P // 10):
        out, thr, sent = mean(c)
        want, T, n = ref.topk_mean_rows(list(x), w, c)
        checked_select(thr, sent, (T, n), x, c, f"0xFF workspace, mean c={c}")
        assert_bits(out, want, f"0xFF workspace, mean c={c}")
    assert_bits(xd, x, "the deltas were written")


def test_k_grows_and_shrinks_on_one_stream(cuda):
    rng = np.random.RandomState(710)
    P = CH + 1
    runs = []
    for K, name in ((17, "five"), (3, "hot_bin"), (20, "gauss"), (3, "last_digit")):
        x = tc.family(name, K, P, rng)
        xd = torch.from_numpy(x).to(cuda)
        for c in (P // 10, 2):
            runs.append((x, xd, c, kernels.topk_select_dense(xd, c), f"K={K} {name} c={c}"))
    torch.cuda.synchronize()
    for x, xd, c, (thr, sent), what in runs:
        checked_select(thr, sent, ref.select(list(x), c), x, c, what)
    assert len(runs) == 8


def test_two_streams_at_once(cuda):
    rng = np.random.RandomState(720)
    xa, xb = tc.family("five", 5, 3 * CH + 5, rng), tc.family("scaled", 12, CH + 1, rng)
    sa, sb = slab_of(xa, cuda), slab_of(xb, cuda)
    wa, wb = weights(5), weights(12)
    torch.cuda.synchronize()
    st = (torch.cuda.Stream(), torch.cuda.Stream())
    ca, cb = (1, xa.shape[1] // 10, 2, xa.shape[1] - 1), (xb.shape[1], 2, xb.shape[1] // 10, 1)
    got = []
    for i in range(4):  # eight alternating calls, no host synchronisation in between
        with torch.cuda.stream(st[0]):
            got.append((xa, wa, ca[i], sa.topk_mean(wa, ca[i])))
        with torch.cuda.stream(st[1]):
            got.append((xb, wb, cb[i], sb.topk_mean(wb, cb[i])))
    torch.cuda.synchronize()
    for i, (x, w, c, res) in enumerate(got):
        mean, T, sent = ref.topk_mean_rows(list(x), w, c)
        checked_select(res.thresholds, res.sent, (T, sent), x, c, f"call {i} c={c}")
        assert_bits(res.mean[0], mean, f"call {i} c={c}: mean")
    assert len(got) == 8


def test_eighteen_streams_pass_the_workspace_cache(cuda):
    rng = np.random.RandomState(730)
    K, P = 4, 1025
    x = tc.family("five", K, P, rng)
    xd = torch.from_numpy(x).to(cuda)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(18)]
    cs = [1 + (37 * i) % P for i in range(19)]
    got = []
    for st, c in zip(streams + streams[:1], cs):
        with torch.cuda.stream(st):
            got.append((c, kernels.topk_select_dense(xd, c)))
    torch.cuda.synchronize()
    want = ref.select_many(list(x), sorted(set(cs)))
    for c, (thr, sent) in got:
        checked_select(thr, sent, want[c], x, c, f"stream sweep c={c}")
    assert len(got) == 19


def test_the_same_call_three_times_gives_the_same_bits(cuda):
    x = tc.family("nan_inf", 9, 2 * CH + 3, np.random.RandomState(740))
    s = slab_of(x, cuda)
    w, c = weights(9), x.shape[1] // 10
    runs = [s.topk_mean(w, c) for _ in range(3)]
    first = [raw(runs[0].mean[0]), raw(runs[0].thresholds), raw(runs[0].sent)]
    for r in runs[1:]:
        for a, b in zip(first, (raw(r.mean[0]), raw(r.thresholds), raw(r.sent))):
            assert np.array_equal(a, b)
    mean, T, sent = ref.topk_mean_rows(list(x), w, c)
    checked_select(runs[0].thresholds, runs[0].sent, (T, sent), x, c, "repeat")
    assert_bits(runs[0].mean[0], mean, "repeat: mean")


# ------------------------------------------------------------------ h. metamorphic
def _run(x, w, c, dev):
    res = slab_of(x, dev).topk_mean(w, c)
    tc.check_definition(host(res.thresholds), host(res.sent), x, c, "metamorphic")
    return raw(res.thresholds), host(res.sent).copy(), host(res.mean[0]).copy()


@pytest.mark.parametrize("name", ("gauss", "five", "nan_inf", "signed_zero"))
def test_column_permutation_and_sign_flip(cuda, name):
    rng = np.random.RandomState(800 + len(name))
    K, P = 6, CH + 5
    x = tc.family(name, K, P, rng)
    w = weights(K)
    for c in (P // 10, P):
        T, sent, mean = _run(x, w, c, cuda)
        perm = rng.permutation(P)
        Tp, sentp, meanp = _run(np.ascontiguousarray(x[:, perm]), w, c, cuda)
        assert Tp.tolist() == T.tolist() and sentp.tolist() == sent.tolist()
        assert_bits(meanp, mean[perm], f"{name} c={c}: permuted columns")
        flipped = (x.view(np.uint32) ^ np.uint32(0x80000000)).view(F32)
        Tf, sentf, meanf = _run(flipped, w, c, cuda)
        assert Tf.tolist() == T.tolist() and sentf.tolist() == sent.tolist()
        # every term flips its sign except a masked coordinate's fl(+0 w_k), so the mean negates bit for
        # bit wherever it is not a zero, and a zero stays a zero (of whichever sign its +0 terms give)
        a, b = ubits(mean), ubits(meanf)
        nz = ((a & 0x7FFFFFFF) != 0) & (a != 0x7FC00000)
        assert np.array_equal(b[nz], a[nz] ^ np.uint32(0x80000000)), f"{name} c={c}: sign flip"
        assert np.array_equal(b[~nz] & 0x7FFFFFFF, a[~nz] & 0x7FFFFFFF), f"{name} c={c}: sign flip, zeros and NaNs"
        if name == "gauss":
            assert nz.sum() > (P // 2 if c == P else P // 10)


def test_scaling_by_a_power_of_two_moves_the_exponent(cuda):
    K, P = 6, CH + 5
    x = tc.family("gauss", K, P, np.random.RandomState(810))
    m = ref.keys(x)
    assert m.min() >= 0x00800000 and m.max() < 0x7F800000 - (5 << 23)  # normal before and after
    for c in ref.keep_counts(P):
        T, sent, _ = _run(x, weights(K), c, cuda)
        T32, sent32, _ = _run((x * F32(32.0)).astype(F32), weights(K), c, cuda)
        assert T32.tolist() == (T + np.uint32(5 << 23)).tolist() and sent32.tolist() == sent.tolist()


# ------------------------------------------------------------------ i. capture
def test_captured_round_with_zero_thresholds_for_some_clients(cuda):
    rng = np.random.RandomState(900)
    K, P, c = 256, 1280, 768  # a staircase's shape, and one of its keep counts
    assert c in tc.staircase_counts(1, 1)
    w = weights(K)
    x0 = tc.family("signed_zero", K, P, rng)
    s = slab_of(x0, cuda)
    out = torch.empty(P, device=cuda)
    s.topk_mean(w, c, out=out)  # the eager call: the weights are on the device
    torch.cuda.synchronize()
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            res = s.topk_mean(w, c, out=out)
            thr_only = s.topk_thresholds(c)
    rounds = (("signed_zero", tc.family("signed_zero", K, P, rng)), ("staircase", tc.staircase(1, 1, rng)),
              ("equal", tc.family("equal", K, P, rng)), ("signed_zero again", x0))
    for name, x in rounds:
        s.rows.copy_(torch.from_numpy(x))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        mean, T, sent = ref.topk_mean_rows(list(x), w, c)
        if name.startswith("signed_zero"):
            assert (T == 0).sum() >= 16 and (T != 0).sum() >= 16, "T = 0 for some clients and not for others"
        checked_select(res.thresholds, res.sent, (T, sent), x, c, f"replay {name}")
        checked_select(thr_only[0], thr_only[1], (T, sent), x, c, f"replay {name}, select alone")
        assert_bits(out, mean, f"replay {name}: mean")
