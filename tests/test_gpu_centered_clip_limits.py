"""Centered clipping at its limits, every comparison bit for bit against the closed numpy
restatement (tests/centered_clip_ref.py: centered_clip_ref(..., sizes=...) restates the norm
order too, so distances, factors and centres are all its own). All shapes are the smallest that
reach the path.

* the norm pass cut into launches of at most 65,535 rows: a slab of 4096 clients x 17 leaves, a
  pytree round of 1030 clients x 64 leaves with one leaf of two norm blocks on the cut, and
  center_l2sq_rows over 65,536 + 3 rows;
* the dense fold's workgroup edges (8,192 elements a workgroup with 16-byte units, the P % 4 tail
  workgroup) with NaN / inf / +-0 deltas, zero, negative and NaN factors and a centre holding +-0,
  around the four clients kept in flight; the same rows through the plan route;
* alignment moved for ONE operand at a time: the centre, the output, the slab base, the stride;
* empty leaves, empty rounds, P = 1, K = 1, K = 4096;
* tau denormal, float32's largest, exactly a client's distance; clients at the centre, of 1e30,
  holding NaN or inf; a NaN in the centre;
* an out that overlaps the deltas is refused with nothing launched;
* two streams, a growing workspace, the workspace table's 16-entry clear, a replay after the
  cached workspace was replaced.
"""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, slab as slab_mod, tree_util as tu
from tests import centered_clip_ref as ref
from tests.test_gpu_centered_clip import (arbitrary_factors, assert_bits, dev_vec, flat_of, fold_ptrs, host, nbits,
                                          on_device, plan_image, special_deltas)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
EUNSUPPORTED = -3
EDGE_PS = [8188, 8191, 8192, 8193, 8195, 8196, 16384 + 5]
EDGE_KS = [1, 3, 4, 5, 9]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def scaled_round(K, sizes, seed, lo=0.5, hi=4.0):
    """A centre and K clients around it, client k at its own scale in [lo, hi): every distance is
    distinct, and tau = the median distance clips about half of them."""
    P = int(sum(sizes))
    rng = np.random.default_rng(seed)
    v = (0.5 * rng.standard_normal(P, dtype=F32)).astype(F32)
    x = rng.standard_normal((K, P), dtype=F32)
    x *= (lo + (hi - lo) * rng.permutation(K) / K).astype(F32)[:, None]
    x += v
    return x, v


def signed_zero_centre(P, seed=0):
    """N(0, 1) with +0 at every 7th and -0 at every 11th entry (from 3)."""
    v = np.random.RandomState(900 + seed + P).standard_normal(P).astype(F32)
    v[::7] = 0.0
    v[3::11] = -0.0
    assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    return v


def make_slab(x, sizes, dev):
    s = slab_mod.ClientDeltaSlab([np.zeros(n, F32) for n in sizes], x.shape[0], device=dev)
    if x.shape[1]:
        s.rows.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return s


def row_trees(xd, sizes):
    """One tree (a list of leaves) per row of the device tensor xd: views of the row."""
    offs = offsets(sizes)
    return [[xd[k, o:o + n] for o, n in zip(offs[:-1], sizes)] for k in range(xd.shape[0])]


def leaf_list(vd, sizes):
    offs = offsets(sizes)
    return [vd[o:o + n] for o, n in zip(offs[:-1], sizes)]


def assert_round(got_centre, got_d, got_f, want, what):
    centre, dist, fac = want
    assert_bits(got_d, dist, what + ": distances")
    assert_bits(got_f, fac, what + ": factors")
    assert_bits(got_centre, centre, what + ": centre")


def both_routes(x, v, sizes, tau, L, dev, what, want=None):
    """The slab and the tree route over the same deltas against the closed restatement."""
    want = ref.centered_clip_ref(x, v, tau, L, sizes=sizes) if want is None else want
    vd = torch.from_numpy(np.array(v)).to(dev)
    a = make_slab(x, sizes, dev).centered_clip(tau, vd, iterations=L)
    assert_round(flat_of(a.center), a.distances, a.factors, want, what + " slab")
    xd = on_device(x, dev, ld=x.shape[1] + 1)
    b = tu.tree_centered_clip(row_trees(xd, sizes), tau, leaf_list(vd, sizes), iterations=L)
    assert [t.numel() for t in b.center] == list(sizes)
    assert_round(flat_of(b.center), b.distances, b.factors, want, what + " tree")
    assert_bits(vd, v, what + ": the centre is not written")
    return want


# ------------------------------------------------------------------ 1. the row split
def test_row_split_slab(cuda):
    K, sizes = 4096, [1 + i % 5 for i in range(17)]
    L = len(sizes)
    assert K * L == 69632 and 65535 // L == 3855 and 65535 % L == 0  # the second launch starts at client 3855
    x, v = scaled_round(K, sizes, seed=2)
    tau = float(np.median(ref.centered_distances_f64(x, v)))
    want = ref.centered_clip_ref(x, v, tau, 2, sizes=sizes)
    # a norm in another client's slot shows: the distances are distinct (among 4096 float32 values
    # within a factor of 8 a chance pair may coincide; no more than that)
    assert len(set(nbits(want[1][0]).tolist())) >= K - 2
    assert K // 2 - 64 <= int((want[2][0] < 1).sum()) <= K // 2 + 64
    vd = torch.from_numpy(v).to(cuda)
    got = make_slab(x, sizes, cuda).centered_clip(tau, vd, iterations=2)
    d, f = host(got.distances), host(got.factors)
    for k in (0, 3853, 3854, 3855, 3856, 4095):  # both sides of row 65,535, by name
        assert nbits(d[:, k]).tolist() == nbits(want[1][:, k]).tolist(), f"client {k} distance"
        assert nbits(f[:, k]).tolist() == nbits(want[2][:, k]).tolist(), f"client {k} factor"
    assert_round(flat_of(got.center), d, f, want, "slab 4096 x 17")


def test_row_split_tree(cuda):
    K, sizes = 1030, [1 + i % 5 for i in range(63)] + [65536 + 1]
    L = len(sizes)
    # row 65,535 = (client 1023, leaf 63): the two-block leaf is the second launch's first row
    assert K * L == 65920 and divmod(65535, L) == (1023, 63)
    x, v = scaled_round(K, sizes, seed=2)
    tau = float(np.median(ref.centered_distances_f64(x, v)))
    want = ref.centered_clip_ref(x, v, tau, 1, sizes=sizes)
    assert len(set(nbits(want[1][0]).tolist())) >= K - 2  # distinct, as above
    assert K // 2 - 32 <= int((want[2][0] < 1).sum()) <= K // 2 + 32
    xd = torch.from_numpy(x).to(cuda)
    vd = torch.from_numpy(v).to(cuda)
    got = tu.tree_centered_clip(row_trees(xd, sizes), tau, leaf_list(vd, sizes))
    d, f = host(got.distances), host(got.factors)
    for k in (0, 1022, 1023, 1024, 1029):
        assert nbits(d[:, k]).tolist() == nbits(want[1][:, k]).tolist(), f"client {k} distance"
        assert nbits(f[:, k]).tolist() == nbits(want[2][:, k]).tolist(), f"client {k} factor"
    assert_round(flat_of(got.center), d, f, want, "tree 1030 x 64")


@pytest.mark.parametrize("R,rpg", [(65536 + 3, 1), (65536 + 5, 7)])
def test_row_split_norm_rows(cuda, R, rpg):
    assert R % rpg == 0
    rng = np.random.default_rng(R)
    n = 1 + np.arange(R) % 3
    x = rng.standard_normal((R, 3), dtype=F32) * (1 + np.arange(R, dtype=F32) / 1024)[:, None]
    cen = rng.standard_normal((5, 3), dtype=F32)
    xd, cd = torch.from_numpy(x).to(cuda), torch.from_numpy(cen).to(cuda)
    image = np.concatenate([xd.data_ptr() + 12 * np.arange(R, dtype=np.int64), n.astype(np.int64),
                            cd.data_ptr() + 12 * (np.arange(R, dtype=np.int64) % 5)])
    d = (x - cen[np.arange(R) % 5]).astype(F32)
    d[np.arange(3)[None, :] >= n[:, None]] = 0.0  # past a row's end: a lane with no element, sum +0
    q = ref.centered_l2sq_rows_ref(d, np.zeros(3, F32), [3])  # fl(d - 0) = d: the row sums, in order
    g = np.zeros(R // rpg, dtype=F32)
    for i in range(rpg):  # k_center_groups: a group's rows in order from +0
        g = g + q.reshape(-1, rpg)[:, i]
    image_dev = torch.from_numpy(image).to(cuda)
    assert_bits(kernels.center_l2sq_rows(image_dev, R, 3, rows_per_group=rpg), g, f"R={R} groups of {rpg}")
    assert_bits(kernels.center_l2sq_rows(image_dev, R, 3, rows_per_group=rpg, take_sqrt=True), np.sqrt(g),
                f"R={R} groups of {rpg}, root")


# ------------------------------------------------------------------ 2. workgroup edges
@pytest.mark.parametrize("K", EDGE_KS)
def test_dense_workgroup_edges(cuda, K):
    for P in EDGE_PS:
        x, v, c = special_deltas(K, P, seed=3), signed_zero_centre(P), arbitrary_factors(K, seed=P)
        want = ref.centered_fold_ref(x, v, c)
        cd = torch.from_numpy(c).to(cuda)
        for off, ld, units in ((0, (P + 3) // 4 * 4, "16-byte"), (1, P + 1 + P % 2, "element")):
            xd = on_device(x, cuda, ld=ld, offset=off)
            assert (xd.data_ptr() % 16 == 0) == (off == 0)
            for nt in (False, True):
                tag = f"K={K} P={P} {units} units nt={nt}"
                vd = dev_vec(v, cuda, offset=off)
                assert_bits(kernels.center_fold_dense(xd, cd, vd, nontemporal=nt), want, tag + " fresh out")
                assert_bits(vd, v, tag + " the centre is not written")
                got = kernels.center_fold_dense(xd, cd, vd, out=vd, nontemporal=nt)
                assert got is vd
                assert_bits(vd, want, tag + " out is center")
            # the plan route: the row as one leaf, and cut into three
            vd = dev_vec(v, cuda, offset=off)
            for leaves in ([P], [P // 3, P // 3 + 1, P - 2 * (P // 3) - 1]):
                assert_bits(fold_ptrs(xd, leaves, cd, vd, cuda), want, f"K={K} P={P} {units} units, plan {leaves}")
                assert_bits(fold_ptrs(xd, leaves, cd, vd, cuda, nontemporal=True), want,
                            f"K={K} P={P} {units} units, plan {leaves} nt")


# ------------------------------------------------------------------ 3. alignment, one operand at a time
def placed(a, dev, offset):
    """A float32 vector `offset` elements into a NaN-filled, 16-byte aligned buffer."""
    t = dev_vec(a, dev, offset=offset)
    assert t.data_ptr() % 16 == 4 * offset
    return t


@pytest.mark.parametrize("K", EDGE_KS)
def test_dense_alignment_one_operand_at_a_time(cuda, K):
    lib, st = _lib.load(), torch.cuda.current_stream(cuda).cuda_stream
    for P in (8191, 8192, 8195, 16384 + 5):
        x, v, c = special_deltas(K, P, seed=4), signed_zero_centre(P, seed=1), arbitrary_factors(K, seed=P + 1)
        want = ref.centered_fold_ref(x, v, c)
        cd = torch.from_numpy(c).to(cuda)
        ld4 = (P + 3) // 4 * 4
        aligned = on_device(x, cuda, ld=ld4)
        tag = f"K={K} P={P}"

        def run(xd, vd, od, what):
            od.fill_(float("nan"))
            assert kernels.center_fold_dense(xd, cd, vd, out=od) is od
            assert_bits(od, want, f"{tag} {what}")
            od.fill_(float("nan"))
            kernels.center_fold_dense(xd, cd, vd, out=od, nontemporal=True)
            assert_bits(od, want, f"{tag} {what} nt")

        run(aligned, placed(v, cuda, 1), placed(v, cuda, 0), "only the centre is 4-byte aligned")
        run(aligned, placed(v, cuda, 0), placed(v, cuda, 1), "only the output is 4-byte aligned")
        run(on_device(x, cuda, ld=ld4, offset=1), placed(v, cuda, 0), placed(v, cuda, 0), "only the slab base")
        odd = on_device(x, cuda, ld=ld4 + 1)
        assert odd.data_ptr() % 16 == 0
        if K > 1:
            assert odd.stride(0) % 4 == 1
            run(odd, placed(v, cuda, 0), placed(v, cuda, 0), "only the stride")
        else:  # one row: the stride is never used, the call stays on 16-byte units and matches
            run(odd, placed(v, cuda, 0), placed(v, cuda, 0), "an odd stride with one client")
            od = placed(v, cuda, 0)
            od.fill_(float("nan"))
            _lib.check(lib.fjagg_center_fold_dense(_lib.F32, odd.data_ptr(), ld4 + 1, 1, P, cd.data_ptr(),
                                                   placed(v, cuda, 0).data_ptr(), od.data_ptr(), 0, st), "fold")
            assert_bits(od, want, f"{tag} an odd ld passed with one client")


def fold_ptrs_placed(xd, leaves, c, v, dev, cen_off=(), out_off=()):
    """center_fold_ptrs with every leaf's centre and output an allocation of its own, leaf l's
    centre (output) one element into its buffer when l is in cen_off (out_off). The plan comes
    from _leaf_plan. Returns (result [P], blocks)."""
    K, P = xd.shape
    offs = offsets(leaves)
    cens = [dev_vec(v[o:o + n], dev, offset=int(l in cen_off)) for l, (o, n) in enumerate(zip(offs[:-1], leaves))]
    outs = [dev_vec(np.full(n, np.nan, F32), dev, offset=int(l in out_off)) for l, n in enumerate(leaves)]
    rows = xd.data_ptr() + 4 * (np.arange(K, dtype=np.int64)[:, None] * xd.stride(0) + offs[None, :-1])
    in_ptrs = np.asarray(rows, dtype=np.int64)
    out_ptrs = np.array([t.data_ptr() for t in outs], dtype=np.int64)
    cen_ptrs = np.array([t.data_ptr() for t in cens], dtype=np.int64)
    blocks, _ = tu._leaf_plan(_lib.F32, np.asarray(leaves, dtype=np.int64), in_ptrs, out_ptrs, cen_ptrs, dev)
    image, nblk = plan_image(rows, out_ptrs, leaves, cen_ptrs, dev)
    kernels.center_fold_ptrs(image, len(leaves), K, nblk, c)
    return torch.cat(outs), np.asarray(blocks)


@pytest.mark.parametrize("K", EDGE_KS)
def test_plan_alignment_one_leaf_at_a_time(cuda, K):
    for P in (8191, 8195, 16384 + 5):
        x, v, c = special_deltas(K, P, seed=5), signed_zero_centre(P, seed=2), arbitrary_factors(K, seed=P + 2)
        want = ref.centered_fold_ref(x, v, c)
        cd = torch.from_numpy(c).to(cuda)
        leaves = [P // 3 // 4 * 4, P // 3 // 4 * 4, P - 2 * (P // 3 // 4 * 4)]  # 16-byte aligned row pieces
        xd = on_device(x, cuda, ld=(P + 3) // 4 * 4)
        got, base = fold_ptrs_placed(xd, leaves, cd, v, cuda)
        assert_bits(got, want, f"K={K} P={P} every leaf aligned")
        for l in range(3):
            for kind, kw in (("centre", dict(cen_off=(l,))), ("output", dict(out_off=(l,)))):
                got, blocks = fold_ptrs_placed(xd, leaves, cd, v, cuda, **kw)
                # that leaf alone walks element units
                assert blocks.tobytes() != base.tobytes(), (P, l, kind)
                only = np.asarray(kernels.ptrs_plan(_lib.F32, leaves, np.arange(3) == l))
                assert blocks.tobytes() == only.tobytes(), (P, l, kind)
                assert_bits(got, want, f"K={K} P={P} leaf {l}: only its {kind} is 4-byte aligned")


# ------------------------------------------------------------------ 4. empty and tiny
@pytest.mark.parametrize("K,sizes,L", [(3, [0, 5, 0, 0, 300, 0], 2), (3, [1], 2), (1, [5, 300], 2), (1, [1], 1),
                                       (4096, [2, 3], 2), (5, [0, 0, 7], 1), (5, [7, 0, 0], 1)])
def test_empty_leaves_and_tiny_rounds(cuda, K, sizes, L):
    x, v = scaled_round(K, sizes, seed=K + len(sizes))
    tau = float(np.median(ref.centered_distances_f64(x, v)))
    want = both_routes(x, v, sizes, tau, L, cuda, f"K={K} sizes={sizes}")
    assert K < 3 or ((want[2][0] < 1).any() and (want[2][0] == 1).any())


def test_round_of_empty_leaves(cuda):
    K, sizes = 4, [0, 0, 0]
    x, v = np.zeros((K, 0), F32), np.zeros(0, F32)
    want = ref.centered_clip_ref(x, v, 1.0, 2, sizes=sizes)
    assert (nbits(want[1]) == 0).all() and (want[2] == 1).all()  # q = +0: distance +0, factor 1
    both_routes(x, v, sizes, 1.0, 2, cuda, "all leaves empty", want)


def test_norm_rows_of_no_elements(cuda):
    R = 1500  # more rows than the smallest cached workspace has floats
    buf = torch.ones(4, device=cuda)
    image = torch.tensor([buf.data_ptr()] * R + [0] * R + [buf.data_ptr()] * R, dtype=torch.int64, device=cuda)
    for rpg in (1, 3):
        got = kernels.center_l2sq_rows(image, R, 0, rows_per_group=rpg, out=torch.full((R // rpg,), -7.0, device=cuda))
        assert (nbits(host(got)) == 0).all(), rpg


# ------------------------------------------------------------------ 5. tau and value extremes
def extreme_cases():
    K, sizes = 6, [5, 300, 2049]
    x, v = scaled_round(K, sizes, seed=11)
    P = x.shape[1]
    d0 = ref.centered_distances_ref(x, v, sizes)
    med = float(np.median(d0.astype(np.float64)))
    out = {}
    # a denormal tau: every factor is a denormal (tau / n is far below 2^-126), every term fl(c d)
    # underflows to a denormal or to 0, and the centre keeps its bits except where it is tiny
    out["tau denormal"] = (x, v, 1e-40)
    # float32's largest tau: tau / n >= 1 (or inf) for every client, so every factor is exactly 1
    # and an iteration is the plain mean taken around the centre
    out["tau float32 max"] = (x, v, float(np.finfo(F32).max))
    # tau exactly client 2's distance: its factor is fl(tau / n) = 1 exactly, by division not by min
    out["tau on the boundary"] = (x, v, float(d0[2]))
    # client 1 is the centre: q = +0, n = +0, tau / 0 = inf, c = 1, and its terms are all +0
    xa = x.copy()
    xa[1] = v
    out["a client at the centre"] = (xa, v, med)
    # a row of 1e30: the squares overflow, q = inf, n = inf, c = tau / inf = 0: skipped
    xb = x.copy()
    xb[3, :] = 1e30
    out["a row of 1e30"] = (xb, v, med)
    # a NaN in row 0 (c = NaN) and an inf in row 4 (q = inf, c = 0): both skipped, the centre finite
    xc = x.copy()
    xc[0, 6] = np.nan
    xc[4, P - 1] = np.inf
    out["a NaN row and an inf row"] = (xc, v, med)
    # a NaN in the centre: its column is NaN for good, every d holds a NaN, so every distance and
    # factor is NaN in every iteration, everyone is skipped and the other columns keep fl(v + 0)
    vn = v.copy()
    vn[7] = np.nan
    out["a NaN in the centre"] = (x, vn, med)
    return sizes, out


@pytest.mark.parametrize("L", [1, 3])
def test_tau_and_value_extremes(cuda, L):
    sizes, cases = extreme_cases()
    for name, (x, v, tau) in cases.items():
        want = both_routes(x, v, sizes, tau, L, cuda, f"{name} L={L}")
        centre, dist, fac = want
        if name == "tau denormal":
            assert (fac > 0).all() and (fac < 1.2e-38).all()
        elif name == "tau float32 max":
            assert (fac == 1).all()
        elif name == "tau on the boundary":
            assert fac[0, 2] == 1 and F32(tau) == dist[0, 2] and (fac[0] < 1).any()
        elif name == "a client at the centre":
            assert nbits(dist[0, 1:2])[0] == 0 and fac[0, 1] == 1
        elif name == "a row of 1e30":
            assert np.isinf(dist[:, 3]).all() and (fac[:, 3] == 0).all() and np.isfinite(centre).all()
        elif name == "a NaN row and an inf row":
            assert np.isnan(fac[:, 0]).all() and (fac[:, 4] == 0).all() and np.isfinite(centre).all()
        else:
            assert np.isnan(dist).all() and np.isnan(fac).all()
            assert np.flatnonzero(np.isnan(centre)).tolist() == [7]
            keep = np.arange(centre.size) != 7
            assert (centre[keep] == v[keep]).all()


# ------------------------------------------------------------------ 6. an out inside the deltas
def test_out_overlapping_the_deltas_is_refused(cuda):
    K, P, ld, tau = 3, 64, 72, 1.0
    lib, st = _lib.load(), torch.cuda.current_stream(cuda).cuda_stream
    x, v = scaled_round(K, [P], seed=21)
    span = (K - 1) * ld + P  # the slab's extent in elements
    store = torch.full((P + span + P,), -7.0, device=cuda)  # P elements of room on both sides
    xd = torch.as_strided(store, (K, P), (ld, 1), P)
    xd.copy_(torch.from_numpy(x))
    assert xd.data_ptr() == store.data_ptr() + 4 * P
    vd = torch.from_numpy(v).to(cuda)
    c = torch.full((K,), 0.5, device=cuda)
    dist, fac = torch.full((2, K), -7.0, device=cuda), torch.full((2, K), -7.0, device=cuda)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    before = store.clone()
    inside = [1, P, P + 1, P + ld - 3, P + ld + 5, P + span - 1]  # element offsets of out in `store`
    for o in inside:
        out = store[o:o + P]
        rc = lib.fjagg_center_fold_dense(_lib.F32, xd.data_ptr(), ld, K, P, c.data_ptr(), vd.data_ptr(), out.data_ptr(),
                                         0, st)
        assert rc == EUNSUPPORTED and b"overlaps the deltas" in lib.fjagg_last_error(), o
        rc = lib.fjagg_center_clip_dense(_lib.F32, xd.data_ptr(), ld, K, P, None, 1, P, tau, 2, vd.data_ptr(),
                                         out.data_ptr(), dist.data_ptr(), fac.data_ptr(), ws.data_ptr(), ws.numel(), 0,
                                         st)
        assert rc == EUNSUPPORTED and b"overlaps the deltas" in lib.fjagg_last_error(), o
        with pytest.raises(ValueError, match="overlap"):
            kernels.center_fold_dense(xd, c, vd, out=out)
        with pytest.raises(ValueError, match="overlap"):
            kernels.centered_clip_dense(xd, tau, vd, iterations=2, out=out)
    sl = make_slab(x, [P], cuda)
    rows_before = sl.rows.clone()
    with pytest.raises(ValueError, match="overlap"):
        sl.centered_clip(tau, vd, out=sl.rows[1])
    with pytest.raises(ValueError, match="overlap"):
        sl.centered_clip(tau, sl.rows[0], out=sl.rows[0])  # in place on a row: out is the centre AND a row
    torch.cuda.synchronize()
    assert torch.equal(store, before) and torch.equal(sl.rows, rows_before), "a refused call wrote something"
    assert (dist == -7.0).all() and (fac == -7.0).all()
    # an out that ends where the slab begins, or begins where it ends, is a valid call
    want = ref.centered_clip_ref(x, v, tau, 2, sizes=[P])
    for o in (0, P + span):
        out, d, f = kernels.centered_clip_dense(xd, tau, vd, iterations=2, out=store[o:o + P])
        assert_round(out, d, f, want, f"out beside the slab at {o}")
    assert_bits(xd, x, "the deltas are not written")
    # a centre that IS a row of the slab, with an output of its own, stays allowed
    want = ref.centered_clip_ref(x, x[1], tau, 2, sizes=[P])
    out, d, f = kernels.centered_clip_dense(xd, tau, xd[1], iterations=2)
    assert_round(out, d, f, want, "the centre is row 1")
    assert_bits(kernels.center_fold_dense(xd, c, xd[1]), ref.centered_fold_ref(x, x[1], np.full(K, 0.5, F32)),
                "fold, the centre is row 1")
    assert_bits(xd, x, "the deltas are not written")


# ------------------------------------------------------------------ 7. streams and the workspace
@functools.lru_cache(maxsize=None)
def stream_round(K, nleaves, seed):
    sizes = [5 + 3 * i for i in range(nleaves)]
    x, v = scaled_round(K, sizes, seed=seed)
    tau = float(np.median(ref.centered_distances_f64(x, v)))
    return x, v, sizes, tau, ref.centered_clip_ref(x, v, tau, 2, sizes=sizes)


def test_second_stream_sees_the_leaf_table(cuda):
    x, v, sizes, tau, want = stream_round(7, 12, 31)
    s = make_slab(x, sizes, cuda)
    vd = torch.from_numpy(v).to(cuda)
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    with torch.cuda.stream(a):
        ra = s.centered_clip(tau, vd, iterations=2)  # uploads the leaf table on stream a
    with torch.cuda.stream(b):
        rb = s.centered_clip(tau, vd, iterations=2)  # no synchronisation in between
    torch.cuda.synchronize()
    assert_round(flat_of(ra.center), ra.distances, ra.factors, want, "stream a")
    assert_round(flat_of(rb.center), rb.distances, rb.factors, want, "stream b")


def test_workspace_grows_and_shrinking_calls_still_match(cuda):
    small, large = stream_round(3, 1, 32), stream_round(64, 24, 33)
    need = _lib.load().fjagg_center_clip_workspace_bytes
    assert int(need(3, 1, max(small[2]))) <= 4096 < int(need(64, 24, max(large[2])))
    st = torch.cuda.Stream(cuda)
    key = (cuda.index if cuda.index is not None else torch.cuda.current_device(), st.cuda_stream)
    with torch.cuda.stream(st):
        sizes_seen = []
        for x, v, sizes, tau, want in (small, large, small):
            got = make_slab(x, sizes, cuda).centered_clip(tau, torch.from_numpy(v).to(cuda), iterations=2)
            sizes_seen.append(kernels._CENTER_WS[key].numel())
            st.synchronize()
            assert_round(flat_of(got.center), got.distances, got.factors, want, f"K={x.shape[0]} L={len(sizes)}")
    assert sizes_seen[0] == 4096 and sizes_seen[1] > 4096 and sizes_seen[2] == sizes_seen[1]  # replaced once, then kept


def test_seventeen_streams_pass_the_workspace_clear(cuda):
    x, v, sizes, tau, want = stream_round(7, 12, 31)
    s = make_slab(x, sizes, cuda)
    vd = torch.from_numpy(v).to(cuda)
    s.centered_clip(tau, vd)  # the leaf table is on the device
    torch.cuda.synchronize()
    kernels._CENTER_WS.clear()
    streams, results, counts = [torch.cuda.Stream(cuda) for _ in range(17)], [], []
    assert len({t.cuda_stream for t in streams}) == 17
    for t in streams:
        with torch.cuda.stream(t):
            r = s.centered_clip(tau, vd, iterations=2)
            ev = torch.cuda.Event()
            ev.record(t)
        results.append((r, ev))
        counts.append(len(kernels._CENTER_WS))
    assert counts == list(range(1, 17)) + [1]  # the 17th key cleared the table
    for i, (r, ev) in enumerate(results):
        ev.synchronize()
        assert_round(flat_of(r.center), r.distances, r.factors, want, f"stream {i}")


def test_replay_after_the_cached_workspace_was_replaced(cuda):
    x, v, sizes, tau, want = stream_round(7, 12, 31)
    big = stream_round(64, 24, 33)
    s = make_slab(x, sizes, cuda)
    buf = torch.from_numpy(v).to(cuda)
    s.centered_clip(tau, buf.clone())  # the eager call: the leaf table is on the device
    torch.cuda.synchronize()
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream(cuda)
    with torch.cuda.stream(st):
        s.centered_clip(tau, buf.clone())  # this stream's cached workspace, the smallest
        with torch.cuda.graph(graph, stream=st):
            res = s.centered_clip(tau, center=buf, iterations=2, out=buf)
        xb, vb, sb, tb, wb = big
        got = make_slab(xb, sb, cuda).centered_clip(tb, torch.from_numpy(vb).to(cuda), iterations=2)
        others = [torch.full((1 << 14,), float(i), device=cuda) for i in range(1, 5)]  # takes freed blocks, if any
        graph.replay()
        st.synchronize()
    assert_round(flat_of(got.center), got.distances, got.factors, wb, "the larger eager round")
    assert_round(buf, res.distances, res.factors, want, "the replay")
    for i, t in enumerate(others, 1):
        assert (t == float(i)).all(), "a tensor allocated after the capture was written"
