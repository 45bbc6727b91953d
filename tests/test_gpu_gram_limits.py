"""The Gram pass at its limits (fjagg_gram_dense / fjagg_gram_ptrs): the arithmetic bit for bit
against the restatement of tests/robust_select_ref.py on integer data that is sensitive to the
chain length, to the order inside the matrix instruction and to a missing fold (the CPU tests of
tests/test_robust_select_ref.py show that it is); exact power-of-two scaling; underflow, overflow
and their containment."""
import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, robust, slab as slab_mod, tree_util as tu
from tests import robust_select_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
C = kernels.GRAM_CHAIN
GAMMA = C * 2.0 ** -24 / (1 - C * 2.0 ** -24)
# an empty leaf, a 1-element leaf, leaves around one chain and past two; leaves 3 and 5 of every
# client are views one element into their buffer
LEAVES = [300, 0, 1, 515, 1027, 259]
MISALIGNED = (3, 5)


def placed(x, dev):
    """x [K, P] as a device view with an odd row stride, its base one element into the buffer,
    NaN all around (never read)."""
    K, P = x.shape
    ld = P + 3
    store = torch.full((1 + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = store[1:].view(K, ld)[:, :P]
    view.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return view


def bits(g):
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    return np.ascontiguousarray(g, dtype=np.float64).view(np.uint64)


def slab_of(x, dev):
    s = slab_mod.ClientDeltaSlab({"w": torch.zeros(x.shape[1])}, x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return s


def which_arithmetic(got, x, ranges=None):
    """For a failure message: the restatements that give exactly `got`."""
    ranges = [(0, x.shape[1])] if ranges is None else ranges
    names = []
    for chain in (64, 128, 256, 512, 1024, 4096):
        for arithmetic in ("fmaf", "pairwise", "unfused"):
            for drop in (False, True):
                if (bits(ref.gram_of_ranges(x, ranges, chain, arithmetic, drop)) == bits(got)).all():
                    names.append(f"chain {chain} {arithmetic}{' without the last fold' if drop else ''}")
    x64 = x.astype(np.float64)
    if (bits(x64 @ x64.T) == bits(got)).all():
        names.append("exact")
    return names or ["none of the restatements"]


def assert_bits(got, want, x, what, ranges=None):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.argwhere(bits(got) != bits(want))
    if bad.size:
        i, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, first at ({i}, {j}): got {got[i, j]!r}, "
                             f"want {want[i, j]!r}; the result equals: {which_arithmetic(got, x, ranges)}")


def clients_of(x, leaves, dev, misaligned=()):
    """K client pytrees, every (client, leaf) its own allocation; the `misaligned` leaves of every
    client are views one element into their buffer (4-byte aligned only)."""
    offs = np.concatenate([[0], np.cumsum(leaves)])
    clients = []
    for k in range(x.shape[0]):
        tree = {}
        for l in range(len(leaves)):
            v = torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]], dtype=F32))
            if l in misaligned:
                buf = torch.full((v.numel() + 2,), float("nan"), dtype=torch.float32, device=dev)
                buf[1:-1].copy_(v)
                tree[f"l{l:02d}"] = buf[1:-1]
            else:
                tree[f"l{l:02d}"] = v.to(dev)
        clients.append(tree)
    return clients


def pointer_table(clients):
    return np.array([[c[name].data_ptr() for name in sorted(c)] for c in clients], dtype=np.int64)


def elem_mask(clients):
    """The leaves that tree_gram walks in element units: some client's pointer is not 16-byte aligned."""
    return (np.bitwise_or.reduce(pointer_table(clients), axis=0) & 15) != 0


def gram_over_plan(clients, leaves, blocks, dev, unaligned):
    """kernels.gram_ptrs over a plan image the test builds itself."""
    ptrs = pointer_table(clients)
    L = len(leaves)
    image = np.concatenate([ptrs.ravel(), np.zeros(L, np.int64), np.array(leaves, np.int64), blocks])
    image_dev = torch.from_numpy(image).to(dev)
    return kernels.gram_ptrs(image_dev, L, len(clients), len(blocks) // 2, unaligned=unaligned)


# ------------------------------------------------------------------ A. the arithmetic, bit for bit
@pytest.mark.parametrize("K", ref.BITWISE_KS)
def test_dense_route_is_the_256_column_fmaf_chain_bit_for_bit(cuda, K):
    assert C == ref.GRAM_CHAIN
    cc = kernels.gram_chunk_columns(K, 2 * C + 3)
    assert kernels.gram_chunk_columns(K, 2 * cc + 1) == cc
    for P in ref.bitwise_columns(cc, C):
        x = ref.midsize_case(K, P)
        want = ref.chain_gram(x, C)
        assert_bits(kernels.gram_dense(placed(x, cuda)), want, x, f"gram_dense K={K} P={P}")
        assert_bits(slab_of(x, cuda).gram(), want, x, f"slab.gram K={K} P={P}")


def test_products_are_fused(cuda):
    """Products of 2^14-sized integers need more than 24 bits: rounding them before the addition
    (no fmaf) gives other bits in most entries (test_wide_integers_tell_fused_from_unfused)."""
    x = ref.wide_ints(np.random.default_rng(11), 5, 700)
    assert_bits(kernels.gram_dense(placed(x, cuda)), ref.chain_gram(x, C), x, "wide integers")


def test_absorption_probe_dense(cuda):
    """G_ii - 2^24 counts the ones after the first fold (ref.absorption_rows): it shows the column
    at which the chain that holds the 2^12 was folded."""
    starts = [0, 1, 200, 255, 256, 257]
    x = ref.absorption_rows(starts, 600)
    got = kernels.gram_dense(placed(x, cuda)).cpu().numpy()
    want = ref.chain_gram(x, C)
    for c, g, w in zip(starts, np.diagonal(got), np.diagonal(want)):
        print(f"2^12 at column {c}: {int(g - 2.0 ** 24)} of 300 ones counted (restatement: {int(w - 2.0 ** 24)})")
    assert_bits(got, want, x, "absorption probe")


@pytest.mark.parametrize("misaligned", [(), (1,)])
def test_absorption_probe_on_pytrees(cuda, misaligned):
    """A leaf boundary inside the run of ones (row 0) folds the chain there; in a leaf walked in
    element units (row 1, misaligned) the plan's ranges, and so the chains, are 64 columns."""
    leaves = [111, 489]
    x = ref.absorption_rows([10, 120], 600)
    clients = clients_of(x, leaves, cuda, misaligned)
    mask = elem_mask(clients)
    assert mask.tolist() == [l in misaligned for l in range(2)]
    blocks = kernels.ptrs_plan(_lib.F32, leaves, mask if mask.any() else False)
    ranges = ref.plan_ranges(blocks, leaves, 4)
    want = ref.gram_of_ranges(x, ranges, C)
    got = tu.tree_gram(clients).cpu().numpy()
    print(f"misaligned={misaligned}: ones counted {(np.diagonal(got) - 2.0 ** 24).astype(int).tolist()}, "
          f"restatement {(np.diagonal(want) - 2.0 ** 24).astype(int).tolist()}")
    assert_bits(got, want, x, "absorption probe on pytrees", ranges)
    # row 0: the plan range that holds the 2^12 (column 10) ends inside the run of ones, at the
    # leaf's end or before its tail entry; the ones up to there are absorbed, the rest counted
    start, end = next(r for r in ranges if r[0] <= 10 < r[1])
    assert 11 < end <= 111 and end - start <= C and want[0, 0] == 2.0 ** 24 + 300 - (end - 11)


@pytest.mark.parametrize("K", [3, 129])
def test_pytree_route_is_the_fmaf_chain_of_its_plan_bit_for_bit(cuda, K):
    P = sum(LEAVES)
    x = ref.midsize_ints(np.random.default_rng(ref.MIDSIZE_SEED + K), K, P)
    clients = clients_of(x, LEAVES, cuda, MISALIGNED)
    mask = elem_mask(clients)
    assert mask.tolist() == [l in MISALIGNED for l in range(len(LEAVES))]
    # the plan tree_gram makes: element units for the misaligned leaves, 16-byte units for the others
    blocks = kernels.ptrs_plan(_lib.F32, LEAVES, mask)
    ranges = ref.plan_ranges(blocks, LEAVES, 4)
    want = ref.gram_of_ranges(x, ranges, C)
    assert np.mean(want != ref.chain_gram(x, C)) >= 0.5  # not the dense route's bits
    assert_bits(tu.tree_gram(iter(clients)), want, x, f"tree_gram K={K}", ranges)
    assert_bits(gram_over_plan(clients, LEAVES, blocks, cuda, False), want, x, f"gram_ptrs K={K}", ranges)
    # the same leaves under a plan made with FJAGG_UNALIGNED: element units everywhere
    blocks1 = kernels.ptrs_plan(_lib.F32, LEAVES, True)
    ranges1 = ref.plan_ranges(blocks1, LEAVES, 1)
    want1 = ref.gram_of_ranges(x, ranges1, C)
    assert np.mean(want1 != want) >= 0.5
    assert_bits(gram_over_plan(clients, LEAVES, blocks1, cuda, True), want1, x, f"gram_ptrs unaligned K={K}", ranges1)


# ------------------------------------------------------------------ B. scaling and magnitude limits
def clamped_normal(K, P, seed):
    """N(0, 1) with |x| clamped to [2^-20, 2^20]: scaled by 2^e, |e| <= 30, no product (at least
    2^-100, at most 2^100) and no partial sum of a chain leaves float32's normal range, so every
    rounding of the scaled run is the unscaled run's rounding."""
    x = np.random.default_rng(seed).standard_normal((K, P))
    x = np.where(x < 0, -1.0, 1.0) * np.clip(np.abs(x), 2.0 ** -20, 2.0 ** 20)
    return x.astype(F32)


@pytest.mark.parametrize("K", [3, 129])
def test_power_of_two_scaling_is_exact(cuda, K):
    P = 2 * C + 3
    x = clamped_normal(K, P, 31 * K)
    base = kernels.gram_dense(placed(x, cuda)).cpu().numpy()
    assert np.isfinite(base).all()
    for e in (-30, -8, 8, 30):
        scaled = np.ldexp(x, e).astype(F32)
        assert (np.ldexp(scaled.astype(np.float64), -e) == x).all()
        got = kernels.gram_dense(placed(scaled, cuda)).cpu().numpy()
        assert (bits(got) == bits(np.ldexp(base, 2 * e))).all(), f"K={K} e={e}"


def test_power_of_two_scaling_is_exact_on_pytrees(cuda):
    K = 3
    x = clamped_normal(K, sum(LEAVES), 5)
    base = tu.tree_gram(clients_of(x, LEAVES, cuda, MISALIGNED)).cpu().numpy()
    for e in (-30, -8, 8, 30):
        got = tu.tree_gram(clients_of(np.ldexp(x, e).astype(F32), LEAVES, cuda, MISALIGNED)).cpu().numpy()
        assert (bits(got) == bits(np.ldexp(base, 2 * e))).all(), f"e={e}"


@pytest.mark.parametrize("K", [3, 129])
def test_underflowing_products(cuda, K):
    """Scaled by 2^-70 every product (about 2^-140) is subnormal or zero in float32. A product or a
    partial sum flushed or rounded in the subnormal range loses less than 2^-126, so
    |G - exact| <= gamma_C * mass + P * 2^-126."""
    P = 2 * C + 3
    x = np.ldexp(clamped_normal(K, P, 17 * K), -70).astype(F32)
    x64 = x.astype(np.float64)
    exact, mass = x64 @ x64.T, np.abs(x64) @ np.abs(x64).T
    for got, what in ((kernels.gram_dense(placed(x, cuda)).cpu().numpy(), "dense"),
                      (tu.tree_gram(clients_of(x, [P - 200, 200], cuda, (1,))).cpu().numpy(), "tree")):
        err = np.abs(got - exact)
        bound = GAMMA * mass + P * 2.0 ** -126
        kept = np.diagonal(got) / np.diagonal(exact)
        print(f"K={K} {what}: products near 2^-140: {'kept (no flush)' if (got != 0).any() else 'flushed to zero'}; "
              f"G_kk / exact in [{kept.min():.4f}, {kept.max():.4f}]; max error {float((err / bound).max()):.3g} of the bound")
        assert (err <= bound).all()
        assert np.isfinite(np.diagonal(got)).all() and (np.diagonal(got) >= 0).all()
        assert (bits(got) == bits(got.T)).all()


def test_everything_underflows(cuda):
    """Scaled by 2^-80 every product is below half the smallest subnormal: G is zero, every client
    is usable, and the two rounds do what fedjax_amd.robust does on the zero matrix."""
    K, P, f, m = 9, 2 * C + 3, 2, 3
    x = np.ldexp(clamped_normal(K, P, 3), -80).astype(F32)
    assert (x != 0).all()
    s = slab_of(x, cuda)
    zero = np.zeros((K, K))
    for G in (s.gram().cpu().numpy(), tu.tree_gram(clients_of(x, [P - 200, 200], cuda, (1,))).cpu().numpy()):
        assert (G == 0).all()
    assert robust.usable(zero).all() and robust.krum_select(zero, f, m).tolist() == [0, 1, 2]
    uniform, dist = robust.weiszfeld_weights(zero, None, 1e-6, 4)
    assert uniform.tolist() == [1.0 / K] * K
    clients = clients_of(x, [P - 200, 200], cuda, (1,))
    for r in (s.krum(f, m), tu.tree_krum(clients, f, m)):
        assert r.selected.tolist() == [0, 1, 2] and r.scores.tolist() == [0.0] * K
    for r in (s.geometric_median(iterations=4, nu=1e-6), tu.tree_geometric_median(clients, iterations=4, nu=1e-6)):
        assert r.weights.tobytes() == uniform.astype(F32).tobytes() and r.distances.tolist() == dist.tolist()
        assert r.median is not None


@pytest.mark.parametrize("K,big,huge,large", [(3, 0, 2, 1), (257, 5, 256, 130)])
def test_overflow_is_contained(cuda, K, big, huge, large):
    """Client `big` at 2^62 with |x| in [1, 2]: every product is finite (at most 2^126) and a
    256-column chain of its squares (at least 2^132) is not. Client `huge` at 2^65: its squares
    overflow as products. Both have a non-finite G_kk, and no entry outside their rows and columns
    changes a bit. Client `large` at 2^60 with |x| <= 1/2: a chain of its squares is at most 2^126,
    it stays usable and within the bound."""
    P = 2 * C + 3
    x = clamped_normal(K, P, 7 * K)
    x[large] = np.ldexp(np.clip(x[large], -0.5, 0.5), 60)
    zeroed = x.copy()
    zeroed[[big, huge]] = 0
    want = kernels.gram_dense(placed(zeroed, cuda)).cpu().numpy()
    bad = x.copy()
    bad[big] = np.ldexp(np.where(x[big] < 0, -1.0, 1.0) * np.clip(np.abs(x[big]), 1.0, 2.0), 62)
    bad[huge] = np.ldexp(x[huge], 65)
    assert np.isfinite(bad).all()
    sq = bad[big].astype(np.float64) ** 2
    assert sq.max() < 2.0 ** 128 and sq[:C].sum() > 2.0 ** 128 and (bad[huge].astype(np.float64) ** 2).max() > 2.0 ** 128
    got = kernels.gram_dense(placed(bad, cuda)).cpu().numpy()
    assert not np.isfinite(got[big, big]) and not np.isfinite(got[huge, huge])
    assert robust.usable(got).tolist() == [k not in (big, huge) for k in range(K)]
    keep = np.ones((K, K), dtype=bool)
    keep[[big, huge], :] = keep[:, [big, huge]] = False
    assert (bits(got)[keep] == bits(want)[keep]).all() and np.isfinite(got[keep]).all()
    x64 = zeroed.astype(np.float64)
    exact, mass = x64 @ x64.T, np.abs(x64) @ np.abs(x64).T
    err = np.abs(got - exact)[keep]
    print(f"K={K}: the 2^60 client's G_kk = 2^{np.log2(got[large, large]):.1f}; "
          f"max error {float((err / mass[keep]).max() / GAMMA):.4f} of gamma_C * mass")
    assert (err <= 1.01 * GAMMA * mass[keep]).all()  # (d), with the float64 additions' 1 % (include/fjagg.h)
