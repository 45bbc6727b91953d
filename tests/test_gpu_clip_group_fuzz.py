"""Seeded random sweep of the clipped and the grouped weighted mean against their numpy
restatements (tests/clipped_mean_ref.py, tests/grouped_mean_ref.py), over the cases of
tests/clip_group_cases.py: random pytree structures of 1-70 leaves with sizes on every unit
boundary, a placement per leaf (own allocation, offset view, non-contiguous view, host numpy,
float64), K from 1 to 257, five kinds of weights, five kinds of clip norm, G in [1, K + 3] with
emptied, single-member, zero-total and NaN-weight groups, and a sprinkle of NaN / inf / -0.

Per case, the clipped sweep checks tree_clipped_mean against the restatement evaluated with
the factors restated from the device norms (mean bit for bit, norms within 2e-6 of the float64
norms where those are finite, clipped == (c != 1), clipped norms verbatim where nothing was
clipped and within 2e-6 otherwise) and ClientDeltaSlab.clipped_mean over the same data against
the same restatement; a test of its own compares the two routes' means bit for bit; the grouped
sweep checks tree_grouped_mean against grouped_mean_ref (None pattern, treedef, leaf shapes, mean bits) and
ClientDeltaSlab.grouped_mean against tree_grouped_mean. Both check that no input leaf changed.
Every NaN is one bit pattern (IEEE 754 leaves a generated NaN's sign and payload open).

No case is skipped: each sweep counts the cases it compared and asserts the count.
"""
import os

import numpy as np
import pytest
import torch

from fedjax_amd import pytree, slab as slab_mod, tree_util as tu
from tests import clip_group_cases as cg
from tests import clipped_mean_ref as cref
from tests import grouped_mean_ref as gref

pytestmark = pytest.mark.gpu
F32 = np.float32
NORM_RTOL = 2e-6  # the bound the project holds all its norms to (tests/test_gpu_clipped_mean.py)
# FJ_FUZZ_CASES / FJ_FUZZ_SEED0: a longer campaign over other seeds (the suite runs the defaults)
NCASES = int(os.environ.get("FJ_FUZZ_CASES", "40"))
SEED0 = int(os.environ.get("FJ_FUZZ_SEED0", "5000"))


def assert_bits(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    g, w = gref.bits(got).reshape(-1), gref.bits(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} against {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at {bad[:4]}"


def flat(tree, dev):
    """A tree's leaves (device tensors of either float type, or numpy) as one float32 device row."""
    parts = [(x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).to(dev))
             .reshape(-1).to(torch.float32) for x in pytree.leaves_of(tree)]
    return torch.cat(parts) if parts else torch.empty(0, device=dev)


def versions(trees):
    return [[x._version for x in pytree.leaves_of(t) if isinstance(x, torch.Tensor)] for t in trees]


def assert_inputs_unchanged(c, trees, before, dev, what):
    assert versions(trees) == before, f"{what}: an input leaf was written in place"
    rows = torch.stack([flat(t, dev) for t in trees])
    assert_bits(rows, c["x"], f"{what}: the input leaves changed")


def check_shapes(c, tree, like, what):
    assert pytree.flatten(tree)[1] == pytree.flatten(like)[1], f"{what}: treedef"
    assert [tuple(t.shape) for t in pytree.leaves_of(tree)] == [tuple(s) for s in c["shapes"]], f"{what}: shapes"
    assert all(t.dtype == torch.float32 for t in pytree.leaves_of(tree)), what


def check_clipped(c, got, dev, what):
    """``got`` (a ClippedMean) against the restatement with the factors restated from got.norms."""
    x, K, C = c["x"], c["K"], c["max_norm"]
    norms = got.norms.cpu().numpy()
    assert norms.dtype == F32 and norms.shape == (K,), what
    with np.errstate(all="ignore"):
        n64 = cref.f64_norms(x)
    fin = np.isfinite(n64)
    err = np.abs(norms[fin] - n64[fin])
    assert (err <= NORM_RTOL * n64[fin]).all(), f"{what}: norms off by {(err / n64[fin]).max():.3e}"
    assert not np.isfinite(norms[~fin]).any(), f"{what}: a finite norm of non-finite deltas"
    fac, mean = cg.clipped_reference(c, norms)
    clipped = got.clipped.cpu().numpy()
    assert clipped.dtype == np.bool_ and (clipped == (fac != 1)).all(), f"{what}: clipped flags"
    assert_bits(flat(got.mean, dev), mean, what + " mean")
    cn = got.clipped_norms.cpu().numpy()
    assert (gref.bits(cn)[~clipped] == gref.bits(norms)[~clipped]).all(), f"{what}: unclipped norms not verbatim"
    with np.errstate(all="ignore"):
        p64 = cref.f64_norms(cref.clipped_products(x, fac))
    m = clipped & np.isfinite(p64)
    assert (np.abs(cn - p64)[m] <= NORM_RTOL * p64[m]).all(), f"{what}: clipped norms"
    assert not np.isfinite(cn[clipped & ~np.isfinite(p64)]).any(), f"{what}: clipped norms of non-finite products"
    return fac


def filled_slab(c, dev):
    sl = slab_mod.ClientDeltaSlab(cg.template(c), c["K"], device=dev)
    assert sl.num_params == c["P"]
    if c["P"]:
        sl.rows.copy_(torch.from_numpy(np.array(c["x"])))
    return sl


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # inf - inf, inf * 0 in the numpy restatements
def test_clipped_mean_sweep(cuda):
    compared = 0
    for s in range(NCASES):
        c = cg.case(SEED0 + s)
        what = f"seed {SEED0 + s} (K={c['K']} L={len(c['sizes'])} P={c['P']} {c['wkind']} {c['clip_kind']})"
        trees = cg.place(c, cuda)
        before = versions(trees)
        got = tu.tree_clipped_mean(list(zip(trees, c["weights"])), c["max_norm"])
        assert isinstance(got, tu.ClippedMean)
        check_shapes(c, got.mean, trees[0], what)
        check_clipped(c, got, cuda, what + " pytree")
        sl = filled_slab(c, cuda)
        dense = sl.clipped_mean(c["weights"], c["max_norm"])
        check_shapes(c, dense.mean, trees[0], what + " slab")
        check_clipped(c, dense, cuda, what + " slab")
        assert_bits(sl.rows, c["x"], what + ": the slab was written")
        assert_inputs_unchanged(c, trees, before, cuda, what)
        compared += 1
    assert compared == NCASES


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_slab_and_pytree_clipped_means_have_the_same_bits(cuda):
    """ClientDeltaSlab.clipped_mean over a case's rows against tree_clipped_mean over its trees:
    the same mean, bit for bit, in every case (its own test, so that a difference here does not
    end the sweep above before its other checks have run).

    Both routes sum a client's squares leaf by leaf in one order (fjagg_l2sq_rows), so their
    norms and factors are the same bits, and both folds are the restatement's sequence.
    """
    compared, differ = 0, []
    for s in range(NCASES):
        c = cg.case(SEED0 + s)
        trees = cg.place(c, cuda)
        got = tu.tree_clipped_mean(list(zip(trees, c["weights"])), c["max_norm"])
        dense = filled_slab(c, cuda).clipped_mean(c["weights"], c["max_norm"])
        a, b = flat(dense.mean, cuda).cpu().numpy(), flat(got.mean, cuda).cpu().numpy()
        bad = int((gref.bits(a) != gref.bits(b)).sum())
        if bad:
            n1, n2 = dense.norms.cpu().numpy().astype(np.float64), got.norms.cpu().numpy().astype(np.float64)
            with np.errstate(all="ignore"):
                dn = np.nanmax(np.where(n1 == n2, 0.0, np.abs(n1 - n2) / np.abs(n2)))
                dm = np.nanmax(np.where(a == b, 0.0, np.abs(a.astype(np.float64) - b) / np.abs(b)))
            differ.append(f"seed {SEED0 + s} (K={c['K']} L={len(c['sizes'])} P={c['P']} {c['clip_kind']}): {bad} of "
                          f"{a.size} elements; norms differ by up to {dn:.2e}, means by up to {dm:.2e} (relative)")
        compared += 1
    assert compared == NCASES
    print(f"{len(differ)} of {NCASES} cases differ")
    for line in differ:
        print(line)
    assert not differ, f"{len(differ)} of {NCASES} cases differ; first: {differ[0]}"


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_grouped_mean_sweep(cuda):
    compared = 0
    for s in range(NCASES):
        c = cg.case(SEED0 + s)
        G, ids, gw = c["G"], c["ids"], c["gweights"]
        what = f"seed {SEED0 + s} (K={c['K']} L={len(c['sizes'])} P={c['P']} G={G} {c['wkind']} {c['group_edits']})"
        trees = cg.place(c, cuda)
        before = versions(trees)
        want = cg.grouped_reference(c)
        got = tu.tree_grouped_mean(list(zip(trees, gw)), ids, G)
        assert isinstance(got, list) and len(got) == G, what
        assert [g is None for g in got] == [w is None for w in want], f"{what}: which groups have a mean"
        sl = filled_slab(c, cuda)
        dense = sl.grouped_mean(gw, ids, G)
        assert [g is None for g in dense] == [w is None for w in want], f"{what}: slab: which groups have a mean"
        alive = [g for g in range(G) if want[g] is not None]
        for g in alive:
            check_shapes(c, got[g], trees[0], f"{what} group {g}")
            check_shapes(c, dense[g], trees[0], f"{what} slab group {g}")
        if alive:  # one device-to-host copy per route, not one per group
            rows = torch.stack([flat(got[g], cuda) for g in alive]).cpu().numpy()
            drows = torch.stack([flat(dense[g], cuda) for g in alive]).cpu().numpy()
            for i, g in enumerate(alive):
                assert_bits(rows[i], want[g], f"{what} group {g}")
                assert_bits(drows[i], rows[i], f"{what} group {g}: slab against pytree")
        assert_bits(sl.rows, c["x"], what + ": the slab was written")
        assert_inputs_unchanged(c, trees, before, cuda, what)
        compared += 1
    assert compared == NCASES

