"""Seeded random sweep of centered clipping against the closed numpy restatement
(tests/centered_clip_ref.py), over the cases of tests/centered_clip_cases.py: K from 1 to 257,
1-9 leaves with sizes on every unit, lane-block, workgroup and norm-block boundary, a 0-3 element
offset per (client, leaf) allocation and per centre leaf, 1-4 iterations, four tau regimes, NaN /
inf / 1e30 / +-0 in some clients, a centre with +-0 entries, in place or into a fresh output.

Every case runs four routes, each compared bit for bit (distances, factors, centre; every NaN
one pattern) with the restatement for its own leaf cut: ClientDeltaSlab.centered_clip and
tree_centered_clip over the case's leaves (and with each other), centered_clip_dense over the
whole row as one leaf, and centered_clip_ptrs over the row cut into two leaves. The inputs are
checked unchanged. Every case is compared: each group counts its cases and asserts the count.
"""
import numpy as np
import pytest
import torch

from fedjax_amd import kernels, slab as slab_mod, tree_util as tu
from tests import centered_clip_cases as cc
from tests.test_gpu_centered_clip import assert_bits, flat_of, host, plan_image

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
GROUPS = 6
assert cc.NCASES % GROUPS == 0


def placed(a, dev, offset):
    """A device copy of the float32 vector `a`, `offset` elements into a NaN-filled allocation."""
    store = torch.full((offset + a.numel() + 3,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:offset + a.numel()]
    view.copy_(a)
    return view


def assert_round(centre, distances, factors, want, what):
    assert_bits(distances, want[1], what + ": distances")
    assert_bits(factors, want[2], what + ": factors")
    assert_bits(centre, want[0], what + ": centre")


def run_case(c, dev):
    K, P, sizes, offs, L, tau = c["K"], c["P"], c["sizes"], c["offs"], c["iterations"], c["tau"]
    what = cc.describe(c)
    X = torch.from_numpy(np.array(c["x"])).to(dev)
    V = torch.from_numpy(np.array(c["v"])).to(dev)
    want = cc.reference(c)

    # the slab route
    sl = slab_mod.ClientDeltaSlab([np.zeros(n, F32) for n in sizes], K, device=dev)
    sl.rows.copy_(X)
    centre = V.clone()
    a = sl.centered_clip(tau, centre, iterations=L, out=centre if c["in_place"] else None)
    assert_round(flat_of(a.center), a.distances, a.factors, want, what + " slab")
    assert_bits(sl.rows, c["x"], what + ": the slab was written")
    if not c["in_place"]:
        assert_bits(centre, c["v"], what + ": the centre was written")

    # the tree route: every (client, leaf) and every centre leaf an allocation of its own
    trees = [[placed(X[k, o:o + n], dev, int(d)) for o, n, d in zip(offs[:-1], sizes, c["delta_offsets"][k])]
             for k in range(K)]
    vtree = [placed(V[o:o + n], dev, int(d)) for o, n, d in zip(offs[:-1], sizes, c["centre_offsets"])]
    b = tu.tree_centered_clip(trees, tau, vtree, iterations=L)
    assert [t.numel() for t in b.center] == sizes
    assert_round(flat_of(b.center), b.distances, b.factors, want, what + " tree")
    assert_bits(flat_of(b.center), flat_of(a.center), what + ": slab against tree")
    assert_bits(b.distances, host(a.distances), what + ": slab against tree, distances")
    assert_bits(torch.cat(vtree), c["v"], what + ": the centre leaves were written")
    for k in (0, K - 1):
        assert_bits(torch.cat(trees[k]), c["x"][k], what + f": client {k}'s leaves were written")

    # the dense driver: the row as one leaf, its own base offset and stride
    ld = P + c["dense_pad"]
    store = torch.full((c["dense_offset"] + K * ld,), float("nan"), dtype=torch.float32, device=dev)
    xd = store[c["dense_offset"]:].view(K, ld)[:, :P]
    xd.copy_(X)
    centre = placed(V, dev, int(c["centre_offsets"][0]))
    out, dist, fac = kernels.centered_clip_dense(xd, tau, centre, iterations=L, out=centre if c["in_place"] else None)
    assert_round(out, dist, fac, cc.reference(c, [P]), what + " dense driver")
    assert_bits(xd, c["x"], what + ": the dense rows were written")

    # the plan driver: the same rows cut into two leaves, the centre's second leaf at its own offset
    cut = [P // 2, P - P // 2]
    starts = np.array([0, cut[0]], dtype=np.int64)
    cens = [placed(V[:cut[0]], dev, int(c["centre_offsets"][0])), placed(V[cut[0]:], dev, int(c["centre_offsets"][-1]))]
    outs = cens if c["in_place"] else [placed(torch.full((n,), float("nan"), device=dev), dev, 0) for n in cut]
    rows = xd.data_ptr() + 4 * (np.arange(K, dtype=np.int64)[:, None] * ld + starts[None, :])
    image, nblk = plan_image(rows, [t.data_ptr() for t in outs], cut, [t.data_ptr() for t in cens], dev)
    dist, fac = kernels.centered_clip_ptrs(image, 2, K, nblk, max(cut), tau, iterations=L)
    assert_round(torch.cat(outs), dist, fac, cc.reference(c, cut), what + " plan driver")
    assert_bits(xd, c["x"], what + ": the plan driver wrote the rows")


@pytest.mark.parametrize("group", range(GROUPS))
def test_centered_clip_sweep(cuda, group):
    compared = 0
    per = cc.NCASES // GROUPS
    for s in range(group * per, (group + 1) * per):
        run_case(cc.case(cc.SEED0 + s), cuda)
        compared += 1
    assert compared == per
