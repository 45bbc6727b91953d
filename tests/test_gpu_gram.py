"""The Gram pass on the GPU (fjagg_gram_dense / fjagg_gram_ptrs, kernels.gram_*, slab.gram,
tree_gram): exact on small integers, within the chain bound gamma_C on normal data, bitwise
reproducible and symmetric, a non-finite client confined to its row and column, and the pytree
route against the slab route."""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import kernels, pytree, slab as slab_mod, tree_util as tu

pytestmark = pytest.mark.gpu
F32 = np.float32
C = kernels.GRAM_CHAIN
KS = [1, 2, 3, 31, 32, 33, 64, 65, 127, 128, 129, 160, 257]  # 257: a second and a third panel
U = 2.0 ** -24
GAMMA = C * U / (1 - C * U)
# the EMNIST-CNN leaf layout with its large leaves at 1/64 scale, a 1-element and an empty leaf
EMNIST_64 = {"conv2_d": {"b": (32,), "w": (3, 3, 1, 32)}, "conv2_d_1": {"b": (64,), "w": (3, 3, 32, 1)},
             "linear": {"b": (128,), "w": (144, 128)}, "linear_1": {"b": (62,), "w": (2, 62)},
             "one": (1,), "zero": (0,)}


def chunk_columns(K):
    """Columns per workgroup at the sizes used here, asked from the library."""
    cc = kernels.gram_chunk_columns(K, 2 * C + 3)
    assert kernels.gram_chunk_columns(K, 2 * cc + 1) == cc and cc % C == 0
    return cc


def columns(K):
    cc = chunk_columns(K)
    ps = sorted({1, 2, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3, 2 * cc - 1, 2 * cc, 2 * cc + 1})
    assert ps[-1] <= 20000
    return ps


def on_device(x, dev, ld=None, offset=0):
    """x [K, P] as a device view with row stride ld and a base offset in elements; everything
    around the rows holds NaN (never read)."""
    K, P = x.shape
    ld = P if ld is None else ld
    store = torch.full((offset + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:].view(K, ld)[:, :P]
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def placed(x, dev):
    return on_device(x, dev, ld=x.shape[1] + 3, offset=1)


def bits(g):
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    return np.ascontiguousarray(g, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def int_data(K, P):
    x = np.random.RandomState(1000 * K + P).randint(-7, 8, size=(K, P))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def normal_data(K, P):
    x = np.random.default_rng(77 * K + P).standard_normal((K, P)).astype(F32)
    x.setflags(write=False)
    return x


def assert_within_bound(G, x, what):
    x64 = np.asarray(x, dtype=np.float64)
    want, mass = x64 @ x64.T, np.abs(x64) @ np.abs(x64).T
    err = np.abs(G - want)
    worst = float((err / np.maximum(mass, 1e-300)).max() / GAMMA)
    print(f"{what}: max error {worst:.4f} of gamma_C * |X||X|^T")
    assert (err <= 1.01 * GAMMA * mass).all(), f"{what}: {worst} of the bound"


# ------------------------------------------------------------------ 1. exact on small integers
@pytest.mark.parametrize("K", KS)
def test_integer_gram_is_exact(cuda, K):
    for P in columns(K):
        x = int_data(K, P)
        want = x.astype(np.int64) @ x.astype(np.int64).T
        got = kernels.gram_dense(placed(x.astype(F32), cuda)).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (K, K)
        bad = np.argwhere(got != want.astype(np.float64))
        assert bad.size == 0, f"K={K} P={P}: {len(bad)} entries differ, first at {bad[:4].tolist()}"


def test_integer_gram_at_the_client_limit(cuda):
    K, P = kernels.GRAM_MAX_CLIENTS, 2 * C + 3  # 8 panels, 36 panel pairs
    x = int_data(K, P)
    want = (x.astype(np.int64) @ x.astype(np.int64).T).astype(np.float64)
    assert (kernels.gram_dense(placed(x.astype(F32), cuda)).cpu().numpy() == want).all()


# ------------------------------------------------------------------ 2. + 3. the bound; same bits twice; symmetry
@pytest.mark.parametrize("K", KS)
def test_bound_determinism_symmetry(cuda, K):
    cc = chunk_columns(K)
    for P in (65, C + 1, 2 * C + 3, 2 * cc + 1):
        x = normal_data(K, P)
        xd = placed(x, cuda)
        g1 = kernels.gram_dense(xd)
        out = torch.full((K, K), -1.0, dtype=torch.float64, device=cuda)
        g2 = kernels.gram_dense(xd, out=out)
        assert g2 is out
        G = g1.cpu().numpy()
        assert (bits(G) == bits(g2)).all(), f"K={K} P={P}: two calls differ"
        assert (bits(G) == bits(G.T)).all(), f"K={K} P={P}: not symmetric"
        assert_within_bound(G, x, f"K={K} P={P}")


# ------------------------------------------------------------------ 4. containment
@pytest.mark.parametrize("K,js", [(257, (0, 130, 256)), (33, (0, 17, 32)), (3, (1,))])
def test_a_non_finite_client_stays_in_its_row_and_column(cuda, K, js):
    P = 2 * chunk_columns(K) + 1
    x = np.array(normal_data(K, P))
    for j in js:
        zeroed = x.copy()
        zeroed[j] = 0
        want = kernels.gram_dense(placed(zeroed, cuda)).cpu().numpy()
        bad = x.copy()
        bad[j, 5] = np.nan
        bad[j, P - 2] = np.inf
        got = kernels.gram_dense(placed(bad, cuda)).cpu().numpy()
        assert not np.isfinite(got[j, j])
        keep = np.ones((K, K), dtype=bool)
        keep[j, :] = keep[:, j] = False
        assert (bits(got)[keep] == bits(want)[keep]).all(), f"K={K} j={j}: an entry outside row/column {j} changed"
        assert np.isfinite(got[keep]).all()


# ------------------------------------------------------------------ 5. the pytree route
def tmap(f, t):
    return {k: tmap(f, v) for k, v in t.items()} if isinstance(t, dict) else f(t)


def separate_clients(x, offs, dev, misalign_leaves=(3, 5)):
    """K client pytrees of the scaled EMNIST layout, every (client, leaf) its own allocation; some
    leaves of every client are views one element into their buffer (4-byte aligned only)."""
    template = tmap(lambda s: np.zeros(s, F32), EMNIST_64)
    shapes, td = pytree.flatten(template)
    clients = []
    for k in range(x.shape[0]):
        leaves = []
        for l, z in enumerate(shapes):
            v = torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]], dtype=F32))
            if l in misalign_leaves:
                buf = torch.empty(v.numel() + 1, dtype=torch.float32, device=dev)
                buf[1:].copy_(v)
                leaves.append(buf[1:].view(z.shape))
            else:
                leaves.append(v.to(dev).view(z.shape))
        clients.append(pytree.unflatten(td, leaves))
    return clients


def emnist_slab(x, dev):
    s = slab_mod.ClientDeltaSlab(tmap(lambda s: torch.zeros(s), EMNIST_64), x.shape[0], device=dev)
    s.rows.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return s


@pytest.mark.parametrize("K", [10, 129])
def test_pytree_route(cuda, K):
    sizes = [z.size for z in pytree.leaves_of(tmap(lambda s: np.zeros(s, F32), EMNIST_64))]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    P = int(offs[-1])
    # integers: both routes are exact, whatever their chains
    xi = np.random.RandomState(K).randint(-7, 8, size=(K, P))
    want = (xi.astype(np.int64) @ xi.astype(np.int64).T).astype(np.float64)
    clients = separate_clients(xi, offs, cuda)
    assert sum(leaf.data_ptr() % 16 == 4 for leaf in pytree.leaves_of(clients[0])) >= 1  # misaligned views
    before = [leaf.clone() for c in clients for leaf in pytree.leaves_of(c)]
    got = tu.tree_gram(iter(clients))  # a one-shot iterable, consumed once
    assert got.dtype == torch.float64 and tuple(got.shape) == (K, K)
    assert (got.cpu().numpy() == want).all()
    assert (emnist_slab(xi, cuda).gram().cpu().numpy() == want).all()
    assert all(torch.equal(a, b) for a, b in zip(before, (leaf for c in clients for leaf in pytree.leaves_of(c))))
    # normal data: the pytree route's chains stop at every leaf's end and the slab's run through
    # the row, so the two agree within the bound, not bit for bit
    x = np.random.default_rng(K).standard_normal((K, P)).astype(F32)
    g_tree = tu.tree_gram(separate_clients(x, offs, cuda)).cpu().numpy()
    g_slab = emnist_slab(x, cuda).gram().cpu().numpy()
    assert_within_bound(g_tree, x, f"tree_gram K={K}")
    assert_within_bound(g_slab, x, f"slab.gram K={K}")
    assert (bits(g_tree) == bits(g_tree.T)).all()
    assert (bits(g_tree) == bits(tu.tree_gram(separate_clients(x, offs, cuda)))).all()


def test_empty_leaves_only(cuda):
    clients = [{"zero": torch.zeros(0, device=cuda)} for _ in range(4)]
    assert (tu.tree_gram(clients).cpu().numpy() == np.zeros((4, 4))).all()
    s = slab_mod.ClientDeltaSlab({"zero": torch.zeros(0)}, 4, device=cuda)
    assert (s.gram().cpu().numpy() == np.zeros((4, 4))).all()


# ------------------------------------------------------------------ 6. the diagonal against the norms
@pytest.mark.parametrize("K", [3, 33, 129])
def test_diagonal_against_l2_norms(cuda, K):
    sizes = [z.size for z in pytree.leaves_of(tmap(lambda s: np.zeros(s, F32), EMNIST_64))]
    x = np.random.default_rng(5 + K).standard_normal((K, sum(sizes))).astype(F32)
    s = emnist_slab(x, cuda)
    diag = np.diagonal(s.gram().cpu().numpy())
    sq = s.l2_norms().cpu().numpy().astype(np.float64) ** 2
    mass = (x.astype(np.float64) ** 2).sum(axis=1)
    print(f"K={K}: diag vs l2_norms^2, max {float((np.abs(diag - sq) / mass).max() / GAMMA):.4f} of gamma_C * sum x^2")
    assert (np.abs(diag - sq) <= 1.01 * GAMMA * mass).all()


def test_refusals_on_the_device(cuda):
    x = torch.zeros(4, 16, device=cuda)
    with pytest.raises(ValueError):
        kernels.gram_dense(x, out=torch.zeros(4, 4, device=cuda))  # float32 out
    with pytest.raises(ValueError):
        kernels.gram_dense(x, out=torch.zeros(4, 5, dtype=torch.float64, device=cuda))
    with pytest.raises(TypeError):
        slab_mod.ClientDeltaSlab({"w": torch.zeros(8)}, 4, dtype=torch.bfloat16, device=cuda).gram()
    with pytest.raises(TypeError, match="float32"):
        tu.tree_gram([{"w": torch.zeros(8, dtype=torch.bfloat16, device=cuda)} for _ in range(3)])
