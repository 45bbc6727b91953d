"""Centered clipping on the GPU (fjagg_l2sq_rows_centered, fjagg_center_fold_dense / _ptrs,
fjagg_center_clip_dense / _ptrs and the Python surface over them) against the numpy float32
restatement in tests/centered_clip_ref.py.

The fold is held to the restatement bit for bit for ANY device factor vector; the norm pass is
held to the restated summation order bit for bit (centered_l2sq_ref), with a zero centre also to
fjagg_l2sq_rows' own bits, and independently to 2e-6 of a float64 norm, the bound the project
holds all its norms to. A whole round is checked closed: its distances are the restatement's of
the restatement's own running centre, its factors the restatement's function of those, and its
centre the restatement's fold driven by them: nothing is taken from the code under test. Bit
patterns are compared with every NaN mapped to one pattern, as tests/test_gpu_clipped_mean.py
does and for its reason.
"""
import functools

import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, pytree, slab as slab_mod, tree_util as tu
from tests import centered_clip_ref as ref
from tests import clipped_mean_ref as cm

pytestmark = pytest.mark.gpu
F32 = np.float32
NORM_RTOL = 2e-6
KS = [1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 130]
PS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 1027, 4099]
EMNIST_64 = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 1)},
             "linear": {"b": (128,), "w": (144, 128)}, "linear_1": {"b": (62,), "w": (2, 62)},
             "one": (1,), "zero": (0,)}


def nbits(a):
    """uint32 bit patterns with every NaN mapped to 0x7fc00000."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def assert_bits(got, want, what=""):
    g, w = nbits(host(got)).reshape(-1), nbits(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} vs {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


@functools.lru_cache(maxsize=None)
def normal(K, P, seed=0):
    x = np.random.RandomState(1000 * seed + 7 * K + P).standard_normal((K, P)).astype(F32)
    x.setflags(write=False)
    return x


def special_deltas(K, P, seed=0):
    """N(0, 1) deltas sprinkled with +-0, NaN, +-inf and 1e30."""
    rng = np.random.RandomState(17 * K + P + seed)
    x = np.array(normal(K, P, seed))
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e30], dtype=F32)
    hit = rng.random_sample((K, P)) < 0.03
    x[hit] = vals[rng.randint(0, len(vals), int(hit.sum()))]
    return x


def arbitrary_factors(K, seed=0):
    """1, fractions, 0, -1, NaN and a denormal, every kind present as soon as K allows."""
    rng = np.random.RandomState(31 * K + seed)
    c = rng.uniform(0.05, 1.0, K).astype(F32)
    c[::4] = 1.0
    for i, v in enumerate((0.0, -1.0, np.nan, 1e-40)):
        if K > i + 1:
            c[(i + 1) * K // 6 + 1 if K > 8 else i + 1] = v
    return c


def on_device(x, dev, ld=None, offset=0):
    """x [K, P] as a device view with row stride ld and a base offset in elements; everything
    around the rows holds NaN (never read)."""
    K, P = x.shape
    ld = P if ld is None else ld
    store = torch.full((offset + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:].view(K, ld)[:, :P]
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def dev_vec(a, dev, offset=0):
    """A float32 vector on the device, `offset` elements into a NaN-filled buffer."""
    a = np.asarray(a, dtype=F32)
    store = torch.full((offset + a.size + 3,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    return view


def nan_fill_unused(x, c):
    """Rows whose factor is <= 0 or NaN hold nothing but NaN: the result must not change."""
    x = np.array(x)
    x[~(c > 0)] = np.nan
    return x


def plan_image(in_ptrs, out_ptrs, leaf_n, center_ptrs, dev, unaligned=None):
    """The device image in_ptrs[K*L] | out_ptrs[L] | leaf_n[L] | blocks | center_ptrs[L]."""
    in_ptrs = np.asarray(in_ptrs, dtype=np.int64)
    out_ptrs, leaf_n, center_ptrs = (np.asarray(a, dtype=np.int64) for a in (out_ptrs, leaf_n, center_ptrs))
    if unaligned is None:
        blocks, _ = tu._leaf_plan(_lib.F32, leaf_n, in_ptrs, out_ptrs, center_ptrs, dev)
    else:
        blocks = kernels.ptrs_plan(_lib.F32, leaf_n, unaligned)
    image = np.concatenate([in_ptrs.ravel(), out_ptrs, leaf_n, blocks, center_ptrs])
    return torch.from_numpy(image).to(dev), len(blocks) // 2


def fold_ptrs(xd, leaves, c, vd, dev, **kw):
    """center_fold_ptrs over the rows of xd cut into `leaves` (sizes), centre vd -> fresh output."""
    K, P = xd.shape
    offs = np.concatenate([[0], np.cumsum(leaves)]).astype(np.int64)
    out = torch.full((P + 1,), float("nan"), dtype=torch.float32, device=dev)
    rows = xd.data_ptr() + 4 * (np.arange(K, dtype=np.int64)[:, None] * xd.stride(0) + offs[None, :-1])
    image, nblk = plan_image(rows, out.data_ptr() + 4 * offs[:-1], leaves, vd.data_ptr() + 4 * offs[:-1], dev,
                             unaligned=kw.get("unaligned"))
    kernels.center_fold_ptrs(image, len(leaves), K, nblk, c, **{k: v for k, v in kw.items() if v is not None})
    assert torch.isnan(out[P:]).all()
    return out[:P]


# ------------------------------------------------------------------ 1. fold pieces, bitwise
@pytest.mark.parametrize("K", KS)
def test_fold_pieces_bitwise(cuda, K):
    for P in PS:
        x = special_deltas(K, P)
        v = np.array(normal(1, P, seed=9)[0])
        v[:: 7] = 0.0
        c = arbitrary_factors(K, seed=P)
        want = ref.centered_fold_ref(x, v, c)
        cd = torch.from_numpy(c).to(cuda)
        tag = f"K={K} P={P}"
        for xs, what in ((x, ""), (nan_fill_unused(x, c), " unused rows NaN")):
            xd = on_device(xs, cuda, ld=(P + 3) // 4 * 4)
            vd = dev_vec(v, cuda)
            assert_bits(kernels.center_fold_dense(xd, cd, vd), want, tag + " dense" + what)
            leaves = [P] if P < 3 else [P // 3, P // 3, P - 2 * (P // 3)]
            assert_bits(fold_ptrs(xd, leaves, cd, vd, cuda), want, tag + " ptrs" + what)
        # element units: an odd stride and a base offset, everything around the rows NaN
        for off in (1, 3):
            xd = on_device(x, cuda, ld=P + 1 + (P % 2), offset=off)
            vd = dev_vec(v, cuda, offset=off)
            assert_bits(kernels.center_fold_dense(xd, cd, vd), want, f"{tag} dense offset {off}")
            assert_bits(kernels.center_fold_dense(xd, cd, vd, nontemporal=True), want, f"{tag} dense nt offset {off}")
            assert_bits(fold_ptrs(xd, [P], cd, vd, cuda), want, f"{tag} ptrs offset {off}")
        # out is center, and a plan made with FJAGG_UNALIGNED
        xd = on_device(x, cuda, ld=(P + 3) // 4 * 4 + 4)
        vd = dev_vec(v, cuda)
        got = kernels.center_fold_dense(xd, cd, vd, out=vd)
        assert got is vd
        assert_bits(got, want, tag + " out is center")
        assert_bits(fold_ptrs(xd, [P], cd, dev_vec(v, cuda), cuda, unaligned=True, nontemporal=True), want,
                    tag + " ptrs unaligned plan")


@pytest.mark.parametrize("K,P", [(1025, 65), (4096, 5)])
def test_fold_many_clients(cuda, K, P):
    x = special_deltas(K, P)
    v = np.array(normal(1, P, seed=9)[0])
    c = arbitrary_factors(K)
    want = ref.centered_fold_ref(x, v, c)
    cd = torch.from_numpy(c).to(cuda)
    xd = on_device(nan_fill_unused(x, c), cuda, ld=P + 3)
    assert_bits(kernels.center_fold_dense(xd, cd, dev_vec(v, cuda)), want, "dense")
    assert_bits(fold_ptrs(xd, [P], cd, dev_vec(v, cuda), cuda), want, "ptrs")
    xa = on_device(x, cuda, ld=(P + 3) // 4 * 4)
    assert_bits(kernels.center_fold_dense(xa, cd, dev_vec(v, cuda)), want, "dense, 16-byte units")


def test_fold_ptrs_in_place(cuda):
    K, P = 9, 1027
    x, v, c = special_deltas(K, P), np.array(normal(1, P, seed=9)[0]), arbitrary_factors(K)
    xd, vd = on_device(x, cuda, ld=1028), dev_vec(v, cuda)
    rows = xd.data_ptr() + 4 * np.arange(K, dtype=np.int64)[:, None] * xd.stride(0)
    image, nblk = plan_image(rows, [vd.data_ptr()], [P], [vd.data_ptr()], cuda)
    kernels.center_fold_ptrs(image, 1, K, nblk, torch.from_numpy(c).to(cuda))
    assert_bits(vd, ref.centered_fold_ref(x, v, c), "a leaf's centre is its output")


# ------------------------------------------------------------------ 2. the norm pass
def norm_rows(cuda, sizes, clients, seed=0):
    """`clients` clients of leaves `sizes`, each leaf its own odd-offset view; the rows in order."""
    rng = np.random.RandomState(seed)
    xs = [[rng.standard_normal(n).astype(F32) for n in sizes] for _ in range(clients)]
    held = [[dev_vec(a, cuda, offset=1 + (i % 3)) for i, a in enumerate(row)] for row in xs]
    return xs, held


def test_norm_pass_zero_centre_has_l2sq_rows_bits(cuda):
    sizes = [70001, 5, 1027]  # the first crosses the 64 Ki-element block
    xs, held = norm_rows(cuda, sizes, 2)
    R, max_n = 6, max(sizes)
    zeros = torch.zeros(max_n, dtype=torch.float32, device=cuda)
    ptrs = [t.data_ptr() for row in held for t in row]
    n = sizes * 2
    image = torch.tensor(ptrs + n + [zeros.data_ptr()] * R, dtype=torch.int64, device=cuda)
    plain = torch.tensor(ptrs + n, dtype=torch.int64, device=cuda)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    for rpg in (1, 3):
        for sq in (False, True):
            want = torch.empty(R // rpg, dtype=torch.float32, device=cuda)
            need = int(_lib.load().fjagg_l2sq_rows_workspace_bytes(R, max_n))
            ws = torch.empty(need, dtype=torch.uint8, device=cuda)
            _lib.call("fjagg_l2sq_rows", _lib.F32, plain.data_ptr(), R, max_n, rpg, int(sq), want.data_ptr(),
                      ws.data_ptr(), ws.numel(), stream)
            got = kernels.center_l2sq_rows(image, R, max_n, rows_per_group=rpg, take_sqrt=sq)
            assert_bits(got, host(want), f"rows_per_group={rpg} sqrt={sq}")
            assert_bits(kernels.center_l2sq_rows(image, R, max_n, rows_per_group=rpg, take_sqrt=sq), host(got), "repeat")


def test_norm_pass_random_centre(cuda):
    sizes = [70001, 5, 1027]
    xs, held = norm_rows(cuda, sizes, 2, seed=1)
    vs, vheld = norm_rows(cuda, sizes, 1, seed=2)
    ptrs = [t.data_ptr() for row in held for t in row]
    image = torch.tensor(ptrs + sizes * 2 + [t.data_ptr() for t in vheld[0]] * 2, dtype=torch.int64, device=cuda)
    got = host(kernels.center_l2sq_rows(image, 6, max(sizes), take_sqrt=True))
    want = np.array([ref.centered_distances_f64(x[None], v)[0] for row in xs for x, v in zip(row, vs[0])])
    for r in range(6):
        print(f"row {r}: got {got[r]!r} f64 {want[r]!r} rel {abs(got[r] - want[r]) / want[r]:.3e}")
    assert (np.abs(got - want) <= NORM_RTOL * want).all()
    assert_bits(kernels.center_l2sq_rows(image, 6, max(sizes), take_sqrt=True), got, "repeats its bits")
    grouped = host(kernels.center_l2sq_rows(image, 6, max(sizes), rows_per_group=3, take_sqrt=True))
    want3 = np.sqrt((want.reshape(2, 3) ** 2).sum(axis=1))
    assert (np.abs(grouped - want3) <= NORM_RTOL * want3).all()
    # the order itself: every row, and every client's three rows in order, with and without the root
    q1 = np.array([ref.centered_l2sq_ref([x], [v]) for row in xs for x, v in zip(row, vs[0])], dtype=F32)
    q3 = np.array([ref.centered_l2sq_ref(row, vs[0]) for row in xs], dtype=F32)
    for rpg, q in ((1, q1), (3, q3)):
        assert_bits(kernels.center_l2sq_rows(image, 6, max(sizes), rows_per_group=rpg), q,
                    f"restated order, {rpg} rows a group")
        assert_bits(kernels.center_l2sq_rows(image, 6, max(sizes), rows_per_group=rpg, take_sqrt=True), np.sqrt(q),
                    f"restated order, {rpg} rows a group, root")
    # rows enough that the order of the four wave sums shows: on this data the reversed order gives
    # other bits in a good share of the rows (on the six rows above it happens to give the same)
    xs, held = norm_rows(cuda, [1027], 48, seed=3)
    x48, v0 = np.stack([row[0] for row in xs]), vs[0][2]
    q = ref.centered_l2sq_rows_ref(x48, v0, [1027])
    assert (nbits(q) != nbits(ref.centered_l2sq_rows_ref(x48, v0, [1027], wave_order=(3, 2, 1, 0)))).sum() >= 8
    image = torch.tensor([row[0].data_ptr() for row in held] + [1027] * 48 + [vheld[0][2].data_ptr()] * 48,
                         dtype=torch.int64, device=cuda)
    assert_bits(kernels.center_l2sq_rows(image, 48, 1027), q, "48 rows of 1027, restated order")


# ------------------------------------------------------------------ 3. the whole round, closed
def check_round(x, v, tau, L, centre, distances, factors, what, sizes):
    """factors = f(distances) bit for bit; the centre is the restatement's folds driven by these
    factors; each distance bit for bit centered_distances_ref's, from the restatement's own running
    centre and summed over the leaf cut `sizes` ([P]: the row as one leaf), and, independently,
    within 2e-6 of the float64 distance to that centre."""
    sizes = [int(n) for n in sizes]
    distances, factors = host(distances), host(factors)
    assert distances.shape == factors.shape == (L, x.shape[0]), what
    cur = np.asarray(v, dtype=F32)
    for l in range(L):
        assert_bits(factors[l], cm.clip_factors_ref(distances[l], tau), f"{what}: factors[{l}]")
        assert_bits(distances[l], ref.centered_distances_ref(x, cur, sizes), f"{what}: distances[{l}], restated order")
        want = ref.centered_distances_f64(x, cur)
        with np.errstate(all="ignore"):
            over = np.isfinite(want) & (want * want > 3.5e38)  # the float32 squares overflow: n = inf
        assert np.isinf(distances[l][over]).all(), f"{what}: distances[{l}] of overflowing rows"
        assert np.isnan(distances[l][np.isnan(want)]).all(), f"{what}: distances[{l}] of NaN rows"
        ok = np.isfinite(want) & ~over
        rel = np.abs(distances[l][ok] - want[ok]) / np.maximum(want[ok], 1e-300)
        print(f"{what}: iteration {l} max rel distance error {rel.max() if rel.size else 0:.3e}")
        assert (np.abs(distances[l][ok] - want[ok]) <= NORM_RTOL * want[ok]).all(), f"{what}: distances[{l}]"
        cur = ref.centered_fold_ref(x, cur, factors[l])
    assert_bits(centre, cur, f"{what}: centre after {L}")


def tmap(f, t):
    return {k: tmap(f, v) for k, v in t.items()} if isinstance(t, dict) else f(t)


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def emnist_round(K):
    sizes = [z.size for z in pytree.leaves_of(tmap(lambda s: np.zeros(s, F32), EMNIST_64))]
    P = sum(sizes)
    rng = np.random.RandomState(9 + K)
    v = (0.5 * rng.standard_normal(P)).astype(F32)
    x = (v + rng.standard_normal((K, P)) * (2.0 ** (np.arange(K) % 4 - 2))[:, None]).astype(F32)
    x.setflags(write=False)
    v.setflags(write=False)
    return x, v, np.concatenate([[0], np.cumsum(sizes)])


def separate_clients(x, offs, dev, misalign_leaf=3):
    """Client pytrees of the scaled EMNIST layout, every (client, leaf) its own allocation; one
    leaf of every client is a view one element into its buffer (4-byte aligned only)."""
    shapes, td = pytree.flatten(tmap(lambda s: np.zeros(s, F32), EMNIST_64))
    clients = []
    for k in range(x.shape[0]):
        leaves = []
        for l, z in enumerate(shapes):
            a = torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]]))
            if l == misalign_leaf:
                buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=dev)
                buf[1:].copy_(a)
                leaves.append(buf[1:].view(z.shape))
            else:
                leaves.append(a.to(dev).view(z.shape))
        clients.append(pytree.unflatten(td, leaves))
    return clients


def emnist_slab(x, dev):
    s = slab_mod.ClientDeltaSlab(tmap(lambda s: torch.zeros(s), EMNIST_64), x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x)))
    return s


def taus(x, v):
    d = ref.centered_distances_f64(x, v)
    return {"median": float(np.median(d)), "huge": 1e30, "tiny": 1e-3 * float(d.min())}


@pytest.mark.parametrize("L", [1, 2, 3])
def test_whole_round_closed(cuda, L):
    K = 10
    x, v, offs = emnist_round(K)
    s = emnist_slab(x, cuda)
    clients = separate_clients(x, offs, cuda)
    assert clients[0]["conv2_d_1"]["w"].data_ptr() % 16 == 4  # the misaligned view
    before = [flat_of(c) for c in clients[:2]]
    vd = torch.from_numpy(np.array(v)).to(cuda)
    vtree = s.unflatten(vd.clone())
    for name, tau in taus(x, v).items():
        what = f"L={L} tau={name}"
        a = s.centered_clip(tau, vd, iterations=L)
        check_round(x, v, tau, L, flat_of(a.center), a.distances, a.factors, what + " slab", np.diff(offs))
        fa = host(a.factors)
        if name == "median":
            assert (fa[0] < 1).sum() in (K // 2, K // 2 + 1)
        elif name == "huge":
            assert (fa == 1).all()
        else:
            assert (fa < 1).all()
        b = tu.tree_centered_clip(iter(clients), tau, vtree, iterations=L)  # a one-shot iterable
        assert pytree.flatten(b.center)[1] == pytree.flatten(vtree)[1]
        assert b.center["zero"].numel() == 0 and b.center["one"].numel() == 1
        check_round(x, v, tau, L, flat_of(b.center), b.distances, b.factors, what + " tree", np.diff(offs))
        # the two routes, bit for bit
        assert_bits(flat_of(b.center), flat_of(a.center), what + " slab against tree")
        assert_bits(b.distances, host(a.distances), what + " distances, slab against tree")
        assert_bits(b.factors, host(a.factors), what + " factors, slab against tree")
        # the pytree centre, and the centre given to the slab as a pytree
        c = s.centered_clip(tau, vtree, iterations=L)
        assert_bits(flat_of(c.center), flat_of(a.center), what + " slab, pytree centre")
        # the two C drivers on their own: the row as one leaf (another norm order, the same contract)
        xd = on_device(x, cuda, ld=x.shape[1] + 3, offset=1)
        out, dist, fac = kernels.centered_clip_dense(xd, tau, vd, iterations=L)
        check_round(x, v, tau, L, out, dist, fac, what + " dense driver", [x.shape[1]])
        res = torch.full((x.shape[1],), float("nan"), dtype=torch.float32, device=cuda)
        rows = xd.data_ptr() + 4 * np.arange(K, dtype=np.int64)[:, None] * xd.stride(0)
        image, nblk = plan_image(rows, [res.data_ptr()], [x.shape[1]], [vd.data_ptr()], cuda)
        dist2, fac2 = kernels.centered_clip_ptrs(image, 1, K, nblk, x.shape[1], tau, iterations=L)
        check_round(x, v, tau, L, res, dist2, fac2, what + " ptrs driver", [x.shape[1]])
        assert_bits(res, host(out), what + " the two drivers")
        assert_bits(dist2, host(dist), what + " the two drivers' distances")
    assert_bits(vd, v, "the centre is not written")
    for c, b0 in zip(clients[:2], before):
        assert_bits(flat_of(c), b0, "the inputs are not written")


def test_default_centre_is_zeros_and_empty_rounds(cuda):
    K = 5
    x, _, offs = emnist_round(K)
    s = emnist_slab(x, cuda)
    tau = taus(x, np.zeros(x.shape[1], F32))["median"]
    a = s.centered_clip(tau, iterations=2)
    check_round(x, np.zeros(x.shape[1], F32), tau, 2, flat_of(a.center), a.distances, a.factors, "slab, no centre",
                np.diff(offs))
    b = tu.tree_centered_clip(separate_clients(x, offs, cuda), tau, iterations=2)
    assert_bits(flat_of(b.center), flat_of(a.center), "tree, no centre")
    assert tu.tree_centered_clip([], 1.0) is None
    e = slab_mod.ClientDeltaSlab({"z": torch.zeros(0)}, 3, device=cuda).centered_clip(1.0, iterations=2)
    assert e.center["z"].numel() == 0 and (host(e.distances) == 0).all() and (host(e.factors) == 1).all()
    e = tu.tree_centered_clip([{"z": torch.zeros(0, device=cuda)}] * 3, 1.0)
    assert e.center["z"].numel() == 0 and host(e.factors).shape == (1, 3)


# ------------------------------------------------------------------ 4. cross-check with clipped_mean
@pytest.mark.parametrize("K", [1, 9, 64])
def test_zero_centre_one_iteration_is_clipped_mean(cuda, K):
    x, _, _ = emnist_round(K)
    x = np.array(normal(K, x.shape[1], seed=4))  # N(0, 1): no product is zero
    s = emnist_slab(x, cuda)
    tau = float(np.median(cm.f64_norms(x)))
    want = s.clipped_mean([1] * K, tau)
    got = s.centered_clip(tau)
    assert_bits(got.distances[0], host(want.norms), "distances are clipped_mean's norms")
    assert_bits(got.factors[0], cm.clip_factors_ref(host(want.norms), tau), "factors rebuilt from its norms")
    assert_bits(flat_of(got.center), flat_of(want.mean), "the centre is its mean")


# ------------------------------------------------------------------ 5. attacks
def byzantine_bound(x, v, fac, nbyz, tau):
    """|B| tau / K (1 + 1e-5) in l2 plus the float32 fold bound (K + 2) 2^-24 sum_k |t_k| per
    element taken in l2: tests/test_centered_clip_ref.py's bound (c)."""
    K = x.shape[0]
    with np.errstate(all="ignore"):
        d = (x - v).astype(F32)
        t = np.where((fac > 0)[:, None], (fac[:, None] * d).astype(F32), F32(0)).astype(np.float64)
    fold = (K + 2) * 2.0 ** -24 * np.abs(t).sum(axis=0)
    return nbyz * tau / K * (1 + 1e-5) + float(np.sqrt((fold * fold).sum()))


def test_attacks(cuda):
    K = 16
    x0, v, offs = emnist_round(K)
    vd = torch.from_numpy(np.array(v)).to(cuda)
    tau = taus(x0, v)["median"]
    for name, fill in (("NaN", np.nan), ("1e30", 1e30)):
        x = np.array(x0)
        if name == "NaN":
            x[3, 100] = fill
        else:
            x[3, :] = fill
        s = emnist_slab(x, cuda)
        plain = flat_of(s.mean([1] * K))
        if name == "NaN":
            assert not np.isfinite(plain).all()
        else:  # 1e30 / 16 stays finite in float32: the plain mean is ruined in every coordinate instead
            assert (np.abs(plain) > 1e28).all()
        got = s.centered_clip(tau, vd, iterations=2)
        centre = flat_of(got.center)
        assert np.isfinite(centre).all(), name
        check_round(x, v, tau, 2, centre, got.distances, got.factors, f"{name} row", np.diff(offs))
        f = host(got.factors)[:, 3]
        assert np.isnan(f).all() if name == "NaN" else (f == 0).all()
    rng = np.random.RandomState(5)
    B = [1, 6, 11]
    attacked, clean = np.array(x0), np.array(x0)
    attacked[B] = (1e6 * rng.standard_normal((len(B), x0.shape[1]))).astype(F32)
    clean[B] = v
    got = emnist_slab(attacked, cuda).centered_clip(tau, vd)
    base = emnist_slab(clean, cuda).centered_clip(tau, vd)
    moved = float(np.sqrt(((flat_of(got.center).astype(np.float64) - flat_of(base.center)) ** 2).sum()))
    bound = byzantine_bound(attacked, v, host(got.factors)[0], len(B), tau)
    print(f"1e6 outliers: moved {moved!r} bound {bound!r} ratio {moved / bound:.6f}")
    assert moved <= bound


# ------------------------------------------------------------------ 6. no host synchronisation
def test_no_host_synchronisation(cuda):
    K = 9
    x, v, _ = emnist_round(K)
    s = emnist_slab(x, cuda)
    vd = torch.from_numpy(np.array(v)).to(cuda)
    tau = taus(x, v)["median"]
    first = s.centered_clip(tau, vd, iterations=2)  # first call: library load, the leaf table upload
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = s.centered_clip(tau, vd, iterations=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_bits(flat_of(got.center), flat_of(first.center), "under sync debug mode")
    assert_bits(got.factors, host(first.factors), "factors under sync debug mode")


# ------------------------------------------------------------------ 7. capture
def test_capture_and_replay(cuda):
    K = 8
    x, v, offs = emnist_round(K)
    s = emnist_slab(x, cuda)
    P = x.shape[1]
    buf = torch.from_numpy(np.array(v)).to(cuda)
    tau = taus(x, v)["median"]
    s.centered_clip(tau, buf.clone(), iterations=2)  # the eager call: the leaf table is on the device
    torch.cuda.synchronize()
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            res = s.centered_clip(tau, center=buf, iterations=2, out=buf)
    for seed in (1, 2):
        rng = np.random.RandomState(seed)
        x2 = (np.array(x) + rng.standard_normal(x.shape)).astype(F32)
        v2 = (np.array(v) + 0.1 * rng.standard_normal(P)).astype(F32)
        s.rows.copy_(torch.from_numpy(x2))
        buf.copy_(torch.from_numpy(v2))
        graph.replay()
        torch.cuda.synchronize()
        replayed, rf = host(buf).copy(), host(res.factors).copy()
        buf.copy_(torch.from_numpy(v2))
        eager = s.centered_clip(tau, center=buf, iterations=2, out=buf)
        assert_bits(replayed, host(buf), f"replay {seed}")
        assert_bits(rf, host(eager.factors), f"replay {seed} factors")
        check_round(x2, v2, tau, 2, replayed, eager.distances, eager.factors, f"replay {seed}", np.diff(offs))
    clients = separate_clients(x, offs, cuda)
    vtree = s.unflatten(torch.from_numpy(np.array(v)).to(cuda))
    want = flat_of(tu.tree_centered_clip(clients, tau, vtree).center)
    fresh = emnist_slab(x, cuda)
    torch.cuda.synchronize()
    # the tree route uploads its plan image, a slab's first call its leaf table: both refuse a capture
    for call in (lambda: tu.tree_centered_clip(clients, tau, vtree), lambda: fresh.centered_clip(tau, vtree)):
        g1, st1 = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(st1):
            with pytest.raises(RuntimeError, match="not capturable"):
                with torch.cuda.graph(g1, stream=st1):
                    call()
        torch.cuda.synchronize()
        assert_bits(flat_of(call().center), want, "eager after the refused capture")


# ------------------------------------------------------------------ 8. the aggregator
def test_aggregator_carries_the_centre(cuda):
    K = 6
    agg = fedjax_amd.aggregators.centered_clip_aggregator(3.0, iterations=2)
    state = agg.init()
    assert state.center is None
    prev = None
    for r in range(3):
        x, _, offs = emnist_round(K + r)
        clients = separate_clients(x[:K], offs, cuda)
        consumed = []

        def triples():
            for k, c in enumerate(clients):
                consumed.append(k)
                yield f"c{k}", c, 1 + 100 * k  # the weights change nothing

        got, state = agg.apply(triples(), state)
        assert consumed == list(range(K))
        assert state.center is got
        want = tu.tree_centered_clip(clients, 3.0, prev, iterations=2)
        assert_bits(flat_of(got), flat_of(want.center), f"round {r}")
        assert sorted(state.factors) == sorted(f"c{k}" for k in range(K))
        assert_bits(torch.stack([state.factors[f"c{k}"] for k in range(K)]), host(want.factors[-1]), f"round {r} factors")
        assert_bits(torch.stack([state.distances[f"c{k}"] for k in range(K)]), host(want.distances[-1]), f"round {r} d")
        prev = got
    none, same = agg.apply([], state)
    assert none is None and same is state


# ------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing(cuda):
    K, P = 3, 64
    bf = slab_mod.ClientDeltaSlab({"a": np.zeros(8, F32)}, K, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        bf.centered_clip(1.0)
    for dt in (torch.bfloat16, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            tu.tree_centered_clip([{"a": torch.ones(8, dtype=dt, device=cuda)} for _ in range(K)], 1.0)
    good = [{"a": torch.ones(8, device=cuda)} for _ in range(K)]
    with pytest.raises(TypeError, match="float32"):
        tu.tree_centered_clip(good, 1.0, {"a": torch.ones(8, dtype=torch.bfloat16, device=cuda)})
    with pytest.raises(ValueError):
        tu.tree_centered_clip(good, 1.0, {"a": torch.ones(9, device=cuda)})
    with pytest.raises(ValueError):
        tu.tree_centered_clip(good, 1.0, {"a": torch.ones(8)})  # a host centre
    sl = slab_mod.ClientDeltaSlab({"a": np.zeros(P, F32)}, K, device=cuda)
    for tau in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="tau"):
            sl.centered_clip(tau)
        with pytest.raises(ValueError, match="tau"):
            fedjax_amd.aggregators.centered_clip_aggregator(tau)
    with pytest.raises(TypeError):
        sl.centered_clip(True)
    with pytest.raises(ValueError, match="iterations"):
        sl.centered_clip(1.0, iterations=0)
    with pytest.raises(TypeError):
        sl.centered_clip(1.0, iterations=1.5)
    both = torch.zeros(P + 4, device=cuda)
    with pytest.raises(ValueError, match="overlap"):
        sl.centered_clip(1.0, both[:P], out=both[4:])
    with pytest.raises(ValueError, match="4096"):
        kernels.center_fold_dense(torch.zeros(4097, 4, device=cuda), torch.ones(4097, device=cuda),
                                  torch.zeros(4, device=cuda))
    # the raw entries: every line of fjagg.h's refusal list returns FJAGG_EUNSUPPORTED and launches nothing
    lib = _lib.load()
    st = torch.cuda.current_stream(cuda).cuda_stream
    x = torch.ones(K, P, device=cuda)
    c = torch.full((K,), 0.5, device=cuda)
    cen = torch.zeros(P, device=cuda)
    out = torch.full((P + 4,), -7.0, device=cuda)
    diag = torch.full((2, 2, K), -7.0, device=cuda)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    image, nblk = plan_image([[x[k].data_ptr()] for k in range(K)], [out.data_ptr()], [P], [cen.data_ptr()], cuda)
    xp, cp, vp, op, ip = x.data_ptr(), c.data_ptr(), cen.data_ptr(), out.data_ptr(), image.data_ptr()
    dp, fp, wp, wn = diag[0].data_ptr(), diag[1].data_ptr(), ws.data_ptr(), ws.numel()

    def fold_dense(dt=_lib.F32, x=xp, ld=P, K=K, P=P, c=cp, v=vp, o=op, fl=0):
        return lib.fjagg_center_fold_dense(dt, x, ld, K, P, c, v, o, fl, st)

    def fold_ptrs(dt=_lib.F32, img=ip, L=1, K=K, nblk=nblk, c=cp, fl=0):
        return lib.fjagg_center_fold_ptrs(dt, img, L, K, nblk, c, fl, st)

    def clip_dense(dt=_lib.F32, x=xp, ld=P, K=K, P=P, tau=1.0, it=2, v=vp, o=op, d=dp, f=fp, w=wp, wb=wn, fl=0):
        return lib.fjagg_center_clip_dense(dt, x, ld, K, P, None, 1, P, tau, it, v, o, d, f, w, wb, fl, st)

    def clip_ptrs(dt=_lib.F32, img=ip, K=K, tau=1.0, it=2, d=dp, f=fp, w=wp, wb=wn, fl=0):
        return lib.fjagg_center_clip_ptrs(dt, img, 1, K, nblk, P, tau, it, d, f, w, wb, fl, st)

    def norms(dt=_lib.F32, img=ip, R=1, o=dp, w=wp, wb=wn):
        return lib.fjagg_l2sq_rows_centered(dt, img, R, P, 1, 0, o, w, wb, st)

    for entry in (fold_dense, fold_ptrs, clip_dense, clip_ptrs):
        for dt in (_lib.BF16, _lib.I32):
            assert entry(dt=dt) == -3, (entry.__name__, dt)
        for bad_k in (0, -1, 4097):
            assert entry(K=bad_k) == -3, (entry.__name__, bad_k)
        for fl in (_lib.SCALE, _lib.ACCUMULATE, _lib.NARROW, _lib.HOST_TABLES, _lib.ZEROED_WS, _lib.UNBALANCED, 12 << 8,
                   1 << 20):
            assert entry(fl=fl) == -3, (entry.__name__, fl)
    assert fold_dense(fl=_lib.UNALIGNED) == -3  # the dense entries choose their units themselves
    assert clip_dense(fl=_lib.UNALIGNED) == -3
    for entry in (fold_dense, clip_dense):
        assert entry(P=0) == -3 and entry(ld=P - 1) == -3
        assert entry(x=None) == -3 and entry(v=None) == -3 and entry(o=None) == -3
        assert entry(P=(1 << 28) + 1, ld=(1 << 28) + 1) == -3  # rows over 1 GiB
        assert entry(v=op + 16) == -3 and entry(v=op, o=op + 4) == -3  # a partial overlap
    assert fold_dense(c=None) == -3 and fold_ptrs(c=None) == -3 and fold_ptrs(img=None) == -3
    assert fold_ptrs(nblk=0) == -3 and fold_ptrs(L=0) == -3
    for entry in (clip_dense, clip_ptrs):
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            assert entry(tau=tau) == -3, (entry.__name__, tau)
        assert entry(it=0) == -3 and entry(it=-2) == -3
        assert entry(d=None) == -3 and entry(f=None) == -3
        assert entry(w=None) == -3 and entry(wb=8) == -3  # too small a workspace
    assert clip_ptrs(img=None) == -3
    assert norms(dt=_lib.BF16) == -3 and norms(R=0) == -3 and norms(img=None) == -3 and norms(o=None) == -3
    assert norms(w=None) == -3 and norms(wb=0) == -3
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (diag == -7.0).all() and (cen == 0).all()
    # the same buffers are valid calls without the faults, and out may be the centre
    assert clip_dense(it=2) == 0 and fold_ptrs() == 0 and fold_dense(v=op, o=op) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:P]).all() and (out[P:] == -7.0).all() and (diag != -7.0).all()
