"""Top-k's transmitted form without a GPU: the C entries refuse bad arguments before any launch,
and the Python layer refuses malformed clients before it looks for a device."""
import numpy as np
import pytest
import torch

from fedjax_amd import _lib
from fedjax_amd.aggregators import compression as comp

EINVAL, EUNSUPPORTED = -1, -3
PTR = 4096  # a non-null address: nothing dereferences it before the refusal


def compact_dense(K=2, P=100, thr=PTR, off=PTR, cap=10, idx=PTR, val=PTR, ws=PTR, ws_bytes=1 << 20):
    return _lib.load().fjcomp_topk_compact_dense(_lib.F32, PTR, P, K, P, thr, off, cap, idx, val, ws, ws_bytes, None)


def compact_ptrs(K=2, P=100, tables=PTR, ws_bytes=1 << 20):
    return _lib.load().fjcomp_topk_compact_ptrs(_lib.F32, tables, K, 1, tables, tables, 1, P, PTR, PTR, 10, PTR, PTR,
                                                PTR, ws_bytes, 0, None)


def fold(K=2, P=100, idx=PTR, val=PTR, cnt=PTR):
    return _lib.load().fjcomp_sparse_fold(idx, val, cnt, K, P, PTR, 1.0, PTR, 0, None)


@pytest.mark.parametrize("call,want,word", [
    (lambda: compact_dense(K=0), EINVAL, "K must be"), (lambda: compact_dense(K=4097), EUNSUPPORTED, "4096"),
    (lambda: compact_dense(P=1 << 31), EUNSUPPORTED, "2^31"), (lambda: compact_dense(off=None), EINVAL, "null"),
    (lambda: compact_dense(idx=None), EINVAL, "null"), (lambda: compact_dense(ws_bytes=7), EINVAL, "workspace"),
    (lambda: compact_ptrs(K=0), EINVAL, "K must be"), (lambda: compact_ptrs(K=4097), EUNSUPPORTED, "4096"),
    (lambda: compact_ptrs(P=1 << 31), EUNSUPPORTED, "2^31"), (lambda: compact_ptrs(tables=None), EINVAL, "null"),
    (lambda: compact_ptrs(ws_bytes=7), EINVAL, "workspace"),
    (lambda: fold(K=0), EINVAL, "K must be"), (lambda: fold(K=4097), EUNSUPPORTED, "4096"),
    (lambda: fold(P=1 << 31), EUNSUPPORTED, "2^31"), (lambda: fold(idx=None), EINVAL, "null"),
    (lambda: fold(val=None), EINVAL, "null"), (lambda: fold(cnt=None), EINVAL, "null"),
])
def test_c_entries_refuse_before_any_launch(call, want, word):
    assert call() == want
    assert word in _lib.load().fjagg_last_error().decode()


def test_compact_workspace_bytes():
    ws = _lib.load().fjcomp_topk_compact_workspace_bytes
    assert (ws(3, 5), ws(0, 5), ws(3, 0)) == (60, 0, 0)


def delta(idx=(1, 4), val=(0.5, -2.0), shapes=((3,), (2, 2)), idt=torch.int32):
    return comp.SparseDelta(torch.tensor(idx, dtype=idt), torch.tensor(val, dtype=torch.float32), shapes)


@pytest.mark.parametrize("bad,error", [
    (lambda: delta(idt=torch.int64), TypeError), (lambda: delta(val=(0.5,)), ValueError),
    (lambda: delta(shapes=((3,), (4,))), ValueError), (lambda: {"w": torch.zeros(7)}, TypeError),
    (lambda: delta(idx=((1, 4),), val=((0.5, -2.0),)), ValueError),
])
def test_aggregator_refuses_malformed_clients(bad, error):
    agg = comp.sparse_mean_aggregator()
    with pytest.raises(error):
        agg.apply([("a", delta(), 1.0), ("b", bad(), 2.0)], agg.init())


def test_template_shapes_are_checked_and_empty_round():
    agg = comp.sparse_mean_aggregator(template={"a": np.zeros(3, np.float32), "b": np.zeros(5, np.float32)})
    with pytest.raises(ValueError, match="leaf shapes"):
        agg.apply([("a", delta(), 1.0)], agg.init())
    state = agg.init()
    mean, after = agg.apply([], state)
    assert mean is None and after is state
