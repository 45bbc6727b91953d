"""Krum and the geometric median on float data with a common component (where the Gram form
d2 = G_ii + G_jj - 2 G_ij cancels), against the brute force on the vectors and the derived bound
of tests/robust_select_ref.py; and a seeded sweep of the Gram pass and Krum over client counts,
leaf layouts and plan shapes on small integers, where everything is exact."""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, pytree, robust, slab as slab_mod, tree_util as tu
from tests import robust_select_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
LAYOUT = {"a": (1000,), "b": (1,), "c": (0,), "d": (1002,)}  # ref.OFFSET_P = 2003 parameters
SIZES = [1000, 1, 0, 1002]


def make_slab(x, dev, shapes):
    s = slab_mod.ClientDeltaSlab({k: torch.zeros(v) for k, v in shapes.items()}, x.shape[0], device=dev)
    assert tuple(s.rows.shape) == x.shape
    s.rows.copy_(torch.from_numpy(np.array(x, dtype=F32)))
    return s


def make_clients(x, dev):
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    return [{name: torch.from_numpy(np.array(x[k, offs[l]:offs[l + 1]], dtype=F32)).to(dev)
             for l, name in enumerate(LAYOUT)} for k in range(x.shape[0])]


def flat_of(tree):
    return torch.cat([x.reshape(-1) for x in pytree.leaves_of(tree)]).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bits(g):
    g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    return np.ascontiguousarray(g, dtype=np.float64).view(np.uint64)


def ids_of(selected, K):
    ids = np.full(K, -1, dtype=np.int64)
    ids[selected] = 0
    return ids


@functools.lru_cache(maxsize=None)
def offset_case(K, ratio):
    """The clients of one (K, ratio) case: made once, shared by the tests, never written."""
    assert sum(SIZES) == ref.OFFSET_P
    x = ref.offset_data(np.random.default_rng(ref.offset_seed(K, ratio)), K, ref.OFFSET_P, ratio, ref.offset_outliers(K))
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------ C. Krum on float data
@pytest.mark.parametrize("K,f,m", ref.OFFSET_KRUM)
def test_krum_with_a_common_component(cuda, K, f, m):
    """ratio 0 and 1: the brute-force scores are more than 2 E apart around and inside the selection
    (tests/test_robust_select_ref.py), so the selection must be the brute-force one, order included.
    Every ratio: the scores are within E (ref.krum_error_bound), no selected client is more than 2 E
    worse than an unselected one, and the mean is the grouped fold over the selection."""
    for ratio in ref.OFFSET_RATIOS:
        x = offset_case(K, ratio)
        want_sel, true = ref.krum_select(x, f, m)
        E = ref.krum_error_bound(x, f)
        s = make_slab(x, cuda, LAYOUT)
        clients = make_clients(x, cuda)
        for r, what in ((s.krum(f, m), "slab"), (tu.tree_krum(iter(clients), f, m), "tree")):
            sel = r.selected.tolist()
            finite = np.isfinite(r.scores)
            err = float(np.abs(r.scores - true)[finite].max())
            print(f"K={K} f={f} m={m} ratio={ratio:g} {what}: err/E = {err / E:.4f}, selection "
                  f"{'equal to' if sel == want_sel.tolist() else 'DIFFERENT from'} the brute force's")
            assert finite.all() and len(sel) == m
            if ratio in (0, 1):
                assert sel == want_sel.tolist(), (what, ratio)
            assert err <= E, (what, ratio)
            unselected = np.setdiff1d(np.arange(K), r.selected)
            assert true[r.selected].max() <= true[unselected].min() + 2 * E, (what, ratio)
            ids = ids_of(r.selected, K)
            if what == "slab":
                assert same_bits(flat_of(r.mean), flat_of(s.grouped_mean([1] * K, ids, 1)[0]))
            else:
                assert same_bits(flat_of(r.mean), flat_of(tu.tree_grouped_mean([(c, 1) for c in clients], ids, 1)[0]))


# ------------------------------------------------------------------ C. the geometric median on the same data
def fold_f32(x, w32):
    """The grouped fold in numpy: s = +0; s = s + x_k * w_k (float32, no FMA); s * f32(1 / W)."""
    W = 0
    for w in w32:
        W += w
    s = np.zeros(x.shape[1], dtype=F32)
    for k in range(x.shape[0]):
        s = (s + (x[k] * w32[k]).astype(F32)).astype(F32)
    return (s * F32(tu._inverse(W))).astype(F32)


@pytest.mark.parametrize("K", [K for K, _, _ in ref.OFFSET_KRUM])
def test_geometric_median_with_a_common_component(cuda, K):
    """End to end against the direct-form float64 iteration on the vectors; the yardstick is the
    same pipeline in numpy on the emulated float32-chain Gram, the margin the 8 x of
    tests/test_gpu_robust_select.py::test_geometric_median."""
    for ratio in ref.OFFSET_RATIOS:
        x = offset_case(K, ratio)
        emulated = ref.chain_gram(x, kernels.GRAM_CHAIN)
        s = make_slab(x, cuda, LAYOUT)
        clients = make_clients(x, cuda)
        for T in (1, 4):
            _, want = ref.weiszfeld(x, np.ones(K), 1e-6, T)
            ya, _ = robust.weiszfeld_weights(emulated, None, 1e-6, T)
            yard = np.abs(fold_f32(x, ya.astype(F32)) - want).max() / np.abs(want).max()
            for r, what in ((s.geometric_median(iterations=T, nu=1e-6), "slab"),
                            (tu.tree_geometric_median(iter(clients), iterations=T, nu=1e-6), "tree")):
                a, _ = robust.weiszfeld_weights(r.gram.cpu().numpy(), None, 1e-6, T)
                assert same_bits(r.weights, a.astype(F32))
                err = np.abs(flat_of(r.median).astype(np.float64) - want).max() / np.abs(want).max()
                # the same error measured against the clients' spread, not the common component
                spread = np.abs(flat_of(r.median).astype(np.float64) - want).max() / np.abs(want - x[:1].astype(np.float64)).max()
                print(f"K={K} ratio={ratio:g} T={T} {what}: error {err:.3g} of max|median| ({spread:.3g} of the "
                      f"distance to a client), yardstick {yard:.3g}")
                assert err <= 8 * yard, (what, ratio, T)


# ------------------------------------------------------------------ D. the seeded sweep
def sweep_clients(x, leaves, views, dev):
    """Every odd client's leaves are views into its row at any element offset (with `views`), the
    other clients' leaves separate allocations."""
    offs = np.concatenate([[0], np.cumsum(leaves)])
    clients = []
    for k in range(x.shape[0]):
        row = torch.from_numpy(x[k]).to(dev)
        clients.append({f"l{j}": (row[offs[j]:offs[j + 1]] if views and k % 2 else row[offs[j]:offs[j + 1]].clone())
                        for j in range(len(leaves))})
    return clients


@pytest.mark.parametrize("part", range(5))
def test_seeded_sweep(cuda, part):
    cases = ref.sweep_cases()
    assert len(cases) == 40
    for i in range(part, len(cases), 5):
        K, leaves, views, f, m, seed = cases[i]
        if sum(leaves) == 0:
            leaves = leaves + [1]
        P = sum(leaves)
        L = len(leaves)
        x = np.random.RandomState(seed).randint(-7, 8, size=(K, P)).astype(F32)
        x64 = x.astype(np.float64)
        want = x64 @ x64.T  # exact: integers below 2^21
        what = f"case {i} K={K} leaves={leaves} views={views}"
        # the dense route, with a row stride of its own
        ld = P + i % 3
        store = torch.full((K * ld,), float("nan"), dtype=torch.float32, device=cuda)
        rows = store.view(K, ld)[:, :P]
        rows.copy_(torch.from_numpy(x))
        g = kernels.gram_dense(rows).cpu().numpy()
        assert (g == want).all(), what
        assert (bits(g) == bits(g.T)).all() and (bits(g) == bits(kernels.gram_dense(rows))).all(), what
        s = make_slab(x, cuda, {f"l{j}": (n,) for j, n in enumerate(leaves)})
        assert (bits(s.gram()) == bits(g)).all(), what
        # the pytree route: per-leaf units as tree_gram chooses them
        clients = sweep_clients(x, leaves, views, cuda)
        ptrs = np.array([[c[f"l{j}"].data_ptr() for j in range(L)] for c in clients], dtype=np.int64)
        nonempty = np.array(leaves) > 0
        mask = (np.bitwise_or.reduce(ptrs, axis=0) & 15) != 0
        assert (mask & nonempty).tolist() == ref.sweep_elem_mask(K, leaves, views).tolist(), what
        t = tu.tree_gram(clients).cpu().numpy()
        assert (t == want).all(), what
        assert (bits(t) == bits(t.T)).all() and (bits(t) == bits(tu.tree_gram(iter(clients)))).all(), what
        # the same leaves under a plan made with FJAGG_UNALIGNED
        blocks = kernels.ptrs_plan(_lib.F32, leaves, True)
        image = np.concatenate([ptrs.ravel(), np.zeros(L, np.int64), np.array(leaves, np.int64), blocks])
        u = kernels.gram_ptrs(torch.from_numpy(image).to(cuda), L, K, len(blocks) // 2, unaligned=True).cpu().numpy()
        assert (u == want).all() and (bits(u) == bits(u.T)).all(), what
        if f is not None:
            want_sel, want_scores = ref.int_krum(x, f, m)
            for r in (s.krum(f, m), tu.tree_krum(clients, f, m)):
                assert r.selected.tolist() == want_sel.tolist(), what
                assert r.scores.tolist() == want_scores.tolist(), what
