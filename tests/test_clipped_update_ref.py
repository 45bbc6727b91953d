"""The restatement of a clipped round's server side (tests/clipped_update_ref.py) pinned on the
CPU: the reference's own numbers (mime_lite_test.py:92-119), the identity that makes the fused
SGD step Mime Lite's server update bit for bit, and the host-side refusals of the two raw
entries (fjagg_server_update_clip_dense / _ptrs), which need no GPU.
"""
import ctypes

import numpy as np
import numpy.testing as npt

from fedjax_amd import _lib, server
from oracle import tree_util_ref as oref
from tests import algorithms_restated as ar
from tests import clipped_mean_ref as cref
from tests.clipped_update_ref import clipped_update_ref, mime_lite_sgd_ref
from tests.test_gpu_parity import _np_server_step

F32 = np.float32


def nbits(a):
    """uint32 bit patterns with every NaN mapped to 0x7fc00000 (the sign and payload of a
    generated NaN are the implementation's, tests/test_gpu_clipped_mean.py)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=F32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


class _Recording:
    """oracle.tree_util_ref with the argument of every tree_clip_by_global_norm call kept:
    the unclipped client deltas as algorithms_restated.mime_lite_round forms them."""

    def __init__(self):
        self.deltas = []

    def __getattr__(self, name):
        return getattr(oref, name)

    def tree_clip_by_global_norm(self, tree, max_norm):
        self.deltas.append(tree)
        return oref.tree_clip_by_global_norm(tree, max_norm)


def mime_lite_fixture():
    """(x [2, 1], weights, max_norm, lr, params, the restated round's own result)."""
    rec = _Recording()
    want = ar.mime_lite_clip_round(rec, np.asarray, np.asarray, lambda w: w)
    x = np.array([[F32(d["w"])] for d in rec.deltas], dtype=F32)  # one scalar leaf "w" per client
    assert x.shape == (2, 1)
    return x, [3, 2], 0.5, 0.2, np.array([4.0], F32), want


def test_reference_kat_mime_lite_clipped_round():
    """mime_lite_test.py:92-119: params 3.904 and clipped norms 0.5, 0.45000005, at
    npt.assert_allclose's default tolerance (the reference's own)."""
    x, weights, C, lr, params, want = mime_lite_fixture()
    with np.errstate(all="ignore"):
        norms = np.sqrt((x * x).sum(axis=1, dtype=F32))
    c = cref.clip_factors_ref(norms, C)
    assert list(c != 1) == [True, False]
    prod = cref.clipped_products(x, c)
    clipped_norms = np.where(c == 1, norms, np.sqrt((prod * prod).sum(axis=1, dtype=F32)))
    p, m, v, count, mean = clipped_update_ref(x, weights, c, server.sgd(lr), params, None, None, 0)
    assert m is None and v is None and count == 1
    npt.assert_allclose(p, [3.904])
    npt.assert_allclose(clipped_norms, [0.5, 0.45000005])
    # and the restated round (through the oracle) agrees with the composed reference bit for bit
    assert nbits(p)[0] == nbits(want["params"]) and nbits(mean)[0] == nbits(want["mean_delta"])
    assert [nbits(t) for t in clipped_norms] == [nbits(want["clipped_norms"][k]) for k in (b"cid0", b"cid1")]


def test_fused_sgd_step_is_mime_lites_server_update_bitwise():
    """fl(p + fl(f32(-lr) * y)) == fl(p - fl(f32(lr) * y)): negation is exact, so both products
    have one magnitude and the sum and the difference round the same value."""
    rs = np.random.RandomState(11)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1.0],
                       dtype=F32)
    y = np.concatenate([(rs.standard_normal(100_000) * np.exp(rs.uniform(-30, 30, 100_000))).astype(F32),
                        np.repeat(special, special.size)])
    p = np.concatenate([rs.standard_normal(100_000).astype(F32), np.tile(special, special.size)])
    for lr in (0.2, 0.5, 1e-3, 3.0, 1e-30):
        opt = server.sgd(lr)
        d = opt.descriptor(1)
        assert F32(d.neg_lr) == -F32(lr)
        with np.errstate(all="ignore"):
            got, _, _ = _np_server_step(opt, d, y, p, None, None)
        want = mime_lite_sgd_ref(p, y, lr)
        assert got.dtype == F32 and np.array_equal(nbits(got), nbits(want)), lr


def test_host_side_refusals_without_gpu():
    """Every refusal of the two raw entries is decided on the host, before any launch: fake
    addresses are never dereferenced and no device is needed."""
    lib = _lib.load()
    EINVAL, EUNSUP = -1, -3
    adam, sgd = server.adam(0.01).descriptor(1), server.sgd(0.2).descriptor(1)
    A = 4096  # a fake, 16-byte aligned device address
    K, P = 4, 64

    def dense(in_dtype=_lib.F32, x=A, ld=P, K=K, P=P, w=A, c=A, opt=adam, params=A, m=A, v=A, mean=None, l2sq=None,
              flags=0, ws=None, ws_bytes=0):
        return lib.fjagg_server_update_clip_dense(in_dtype, x, ld, K, P, w, c, 1.0,
                                                  None if opt is None else ctypes.byref(opt), params, m, v, mean,
                                                  l2sq, flags, ws, ws_bytes, None)

    def ptrs(in_dtype=_lib.F32, image=A, L=1, K=K, nblk=1, w=A, c=A, opt=adam, state=A, l2sq=None, flags=0,
             ws=None, ws_bytes=0):
        return lib.fjagg_server_update_clip_ptrs(in_dtype, image, L, K, nblk, w, c, 1.0,
                                                 None if opt is None else ctypes.byref(opt), state, l2sq, flags,
                                                 ws, ws_bytes, None)

    bad7, bad0, badf = server.adam(0.01).descriptor(1), server.adam(0.01).descriptor(1), server.adam(0.01).descriptor(1)
    bad7.kind, bad0.kind, badf.flags = 7, 0, _lib.OPT_F_CENTERED
    cases = [("bf16", dict(in_dtype=_lib.BF16), EUNSUP), ("int32", dict(in_dtype=_lib.I32), EUNSUP),
             ("FJAGG_NARROW", dict(flags=_lib.NARROW), EUNSUP), ("FJAGG_HOST_TABLES", dict(flags=_lib.HOST_TABLES), EUNSUP),
             ("FJAGG_ZEROED_WS", dict(flags=_lib.ZEROED_WS), EUNSUP), ("a variant byte", dict(flags=12 << 8), EUNSUP),
             ("FJAGG_ACCUMULATE", dict(flags=_lib.ACCUMULATE), EUNSUP), ("FJAGG_SCALE", dict(flags=_lib.SCALE), EUNSUP),
             ("FJAGG_UNBALANCED", dict(flags=_lib.UNBALANCED), EUNSUP),
             ("kind 7", dict(opt=bad7), EINVAL), ("kind 0", dict(opt=bad0), EINVAL),
             ("a flag adam does not have", dict(opt=badf), EINVAL), ("no descriptor", dict(opt=None), EINVAL),
             ("null w", dict(w=None), EINVAL), ("null c", dict(c=None), EINVAL),
             ("K = 0", dict(K=0), EINVAL),
             ("K > 4096 with norms", dict(K=4097, l2sq=A, ws=A, ws_bytes=1 << 30), EUNSUP),
             ("norms without a workspace", dict(l2sq=A), EINVAL),
             ("a workspace that is too small", dict(l2sq=A, ws=A, ws_bytes=4), EINVAL)]
    for what, kw, want in cases:
        for name, entry in (("dense", dense), ("ptrs", ptrs)):
            rc = entry(**kw)
            assert rc == want and lib.fjagg_last_error(), (name, what, rc, lib.fjagg_last_error())
    for what, rc, want in [
        ("FJAGG_UNALIGNED on the dense entry", dense(flags=_lib.UNALIGNED), EUNSUP),
        ("null x", dense(x=None), EINVAL), ("null params", dense(params=None), EINVAL),
        ("null m under adam", dense(m=None), EINVAL), ("null v under adam", dense(v=None), EINVAL),
        ("null m under momentum", dense(opt=server.sgd(0.1, momentum=0.9).descriptor(1), m=None, v=None), EINVAL),
        ("P = 0", dense(P=0), EINVAL), ("ld < P", dense(ld=P - 1), EINVAL),
        ("rows over 1 GiB", dense(P=(1 << 28) + 1, ld=(1 << 28) + 4), EUNSUP),
        ("null image", ptrs(image=None), EINVAL), ("null state table", ptrs(state=None), EINVAL),
        ("L = 0", ptrs(L=0), EINVAL), ("nblk = 0", ptrs(nblk=0), EINVAL), ("nblk < 0", ptrs(nblk=-1), EINVAL),
        ("nblk over 2^31", ptrs(nblk=1 << 31), EINVAL),
    ]:
        assert rc == want, (what, rc, lib.fjagg_last_error())
    assert b"ACCUMULATE" in (dense(flags=_lib.ACCUMULATE) and lib.fjagg_last_error())
    # sgd reads no moments: null m and v pass that check (and the call is refused for another reason)
    assert dense(opt=sgd, m=None, v=None, K=0) == EINVAL and b"K must be" in lib.fjagg_last_error()
