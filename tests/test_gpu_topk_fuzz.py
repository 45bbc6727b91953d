"""The seeded sweep of the top-k sparsified mean on the GPU: tc.NCASES layouts from tc.SEED0
(tests/topk_cases.py: K around the fold's batches of eight, up to 40 leaves with empty ones first,
last and adjacent, a 0-dimensional leaf, per-leaf element offsets, a strided leaf, a client on the
host, every data family, weights down to the smallest subnormal). Each case runs through
tree_util.tree_topk_mean and through a ClientDeltaSlab of the same deltas; both are compared with
the numpy restatement (thresholds and sent raw, every leaf's mean bit for bit with every NaN as one
pattern, shapes kept), with each other, and with the definition by comparisons alone; the inputs,
and the NaN guard elements around them, are verified unchanged. tests/test_topk_cases.py shows
on the CPU what the committed seeds reach."""
import numpy as np
import pytest
import torch

from fedjax_amd import tree_util as tu
from fedjax_amd.slab import ClientDeltaSlab
from tests import topk_cases as tc
from tests import topk_ref as ref
from tests.test_gpu_topk import assert_bits, host
from tests.test_gpu_topk_limits import checked_select, raw

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
GROUPS = 8
NAN_BITS = np.array(float("nan"), F32).view(np.uint32)


def place(a, dev, offset, strided):
    """(leaf, allocation, the allocation's expected bits): a device copy of `a`, `offset` elements
    into a NaN-filled allocation with three guard elements behind it; `strided`: every other
    element of the allocation (a non-contiguous view)."""
    n, step = a.size, 2 if strided else 1
    store = torch.full((offset + step * n + 3,), float("nan"), dtype=torch.float32, device=dev)
    view = store[offset:offset + step * n:step].view(a.shape)
    assert view.is_contiguous() != bool(strided)
    view.copy_(torch.from_numpy(a))
    expect = np.full(store.numel(), NAN_BITS, np.uint32)
    expect[offset:offset + step * n:step] = a.view(np.uint32).ravel()
    return view, store, expect


def run_case(lay, dev):
    what = tc.describe(lay)
    trees = tc.trees(lay)
    K, names, w, c = lay["K"], lay["names"], lay["weights"], lay["c"]
    clients, watched = [], []
    for k, t in enumerate(trees):
        if k == lay["host_client"]:
            clients.append({n: t[n].copy() for n in names})  # numpy arrays on the host
            continue
        d = {}
        for l, n in enumerate(names):
            strided = lay["strided"] == (k, l)
            d[n], store, expect = place(t[n], dev, int(lay["offsets"][k, l]), strided)
            if k in (0, K - 1) or strided:
                watched.append((k, n, store, expect))
        clients.append(d)
    a = tu.tree_topk_mean(list(zip(clients, w)), c)
    s = ClientDeltaSlab(trees[0], K, device=dev)
    for k, t in enumerate(trees):
        s.set_client(k, t)
    b = s.topk_mean(w, c)

    mean, T, sent = ref.topk_mean_trees(trees, w, c)
    rows = [ref.flat_row([t[n] for n in names]) for t in trees]
    assert rows[0].size == lay["P"]
    checked_select(a.thresholds, a.sent, (T, sent), rows, c, what + " tree")
    checked_select(b.thresholds, b.sent, (T, sent), rows, c, what + " slab")
    for n, shape in zip(names, lay["shapes"]):
        assert tuple(a.mean[n].shape) == tuple(b.mean[n].shape) == shape, (what, n)
        assert_bits(a.mean[n], np.asarray(mean[n], dtype=F32), what + f" tree leaf {n}")
        assert_bits(b.mean[n], np.asarray(mean[n], dtype=F32), what + f" slab leaf {n}")
        assert_bits(a.mean[n], b.mean[n], what + f" tree against slab, leaf {n}")
    for k, n, store, expect in watched:
        assert np.array_equal(raw(store), expect), (what, f"client {k} leaf {n}: the leaf or its guards were written")
    for k in {0, K - 1, lay["host_client"]} - {None}:
        for n in names:
            assert np.array_equal(raw(clients[k][n]), trees[k][n].view(np.uint32).ravel()), (what, k, n)
    assert np.array_equal(raw(s.rows), np.stack(rows).view(np.uint32).ravel()), (what, "the slab was written")


@pytest.mark.parametrize("group", range(GROUPS))
def test_fuzz(cuda, group):
    per = tc.NCASES // GROUPS
    assert per * GROUPS == tc.NCASES
    compared = 0
    for i in range(group * per, (group + 1) * per):
        run_case(tc.layout(tc.SEED0 + i), cuda)
        compared += 1
    assert compared == per
