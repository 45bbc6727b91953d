"""FLTrust at its limits on the GPU: more than 65535 (client, leaf) rows in one row pass, the
refusals of the new entries with real device buffers (nothing is launched: a NaN-filled output stays
as it was), and the empty rounds of the two surfaces."""
import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, slab as slab_mod, tree_util as tu
from tests import fltrust_cases as fc
from tests import fltrust_ref as ref

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def test_more_rows_than_one_grid_holds(cuda):
    """R = K L = 64 x 1025 = 65600 rows of one element each: the grid's y-dimension is split."""
    K, L = 64, 1025
    x, g = fc.mixed_round(K, L, seed=7)
    sizes = (1,) * L
    want = fc.mixed_reference(K, L, sizes, seed=7)
    xd, gd = fc.on_device(x, cuda, ld=L + 3), torch.from_numpy(np.array(g)).to(cuda)
    tab = torch.from_numpy(np.concatenate([np.arange(L), np.ones(L)]).astype(np.int64)).to(cuda)
    a, q = kernels.dotsq_dense(xd, gd, leaf_table=tab, max_n=1)
    fc.assert_same_bits(a, want["a"], "65600 rows, dense dot")
    fc.assert_same_bits(q, want["q"], "65600 rows, dense squares")
    rows = (xd.data_ptr() + 4 * xd.stride(0) * np.arange(K, dtype=np.int64)[:, None]
            + 4 * np.arange(L, dtype=np.int64)[None]).reshape(-1)
    image = torch.from_numpy(np.concatenate([rows, np.ones(K * L, np.int64),
                                             np.tile(gd.data_ptr() + 4 * np.arange(L, dtype=np.int64), K)])).to(cuda)
    a, q = kernels.dotsq_rows(image, K * L, 1, rows_per_group=L)
    fc.assert_same_bits(a, want["a"], "65600 rows, table dot")
    fc.assert_same_bits(q, want["q"], "65600 rows, table squares")
    # and the whole round over that layout
    out, d = kernels.fltrust_dense(xd, gd, leaf_table=tab, max_n=1)
    fc.assert_same_bits(out, np.concatenate(want["mean"]), "65600 rows, whole round: mean")
    fc.assert_same_bits(d.trust, want["trust"], "65600 rows, whole round: trust")
    fc.assert_same_bits(d.count, want["count"], "65600 rows, whole round: count")


def test_refusals_launch_nothing(cuda):
    lib = _lib.load()
    for sym in ("fjagg_dotsq_rows_workspace_bytes", "fjagg_dotsq_rows", "fjagg_dotsq_dense", "fjagg_fltrust_select",
                "fjagg_fltrust_workspace_bytes", "fjagg_fltrust_dense", "fjagg_fltrust_ptrs"):
        assert hasattr(lib, sym)
    K, P = 8, 100
    x, g = fc.mixed_round(K, P)
    xd, gd = fc.on_device(x, cuda), torch.from_numpy(np.array(g)).to(cuda)
    out = torch.full((P,), float("nan"), dtype=torch.float32, device=cuda)
    diag = torch.full((16 * K,), float("nan"), dtype=torch.float64, device=cuda)
    need = int(lib.fjagg_fltrust_workspace_bytes(K, 1, P))
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    s = torch.cuda.current_stream(cuda).cuda_stream
    d = [diag.data_ptr() + 8 * K * i for i in range(7)]

    def dense(dtype=_lib.F32, xp=xd.data_ptr(), ld=P, K_=K, P_=P, gp=gd.data_ptr(), op=out.data_ptr(), wp=ws.data_ptr(),
              wb=need, flags=0):
        return lib.fjagg_fltrust_dense(dtype, xp, ld, K_, P_, None, 1, P_, gp, op, *d, wp, wb, flags, s)

    for kwargs in (dict(dtype=_lib.BF16), dict(K_=0), dict(K_=4097), dict(P_=0), dict(ld=P - 1), dict(xp=None),
                   dict(gp=None), dict(op=None), dict(wp=None), dict(wb=need - 1), dict(op=xd.data_ptr() + 4 * P),
                   dict(op=gd.data_ptr()), dict(op=ws.data_ptr()), dict(op=diag.data_ptr() + 8 * K), dict(flags=_lib.SCALE), dict(flags=_lib.UNALIGNED),
                   dict(flags=_lib.ACCUMULATE)):
        assert dense(**kwargs) == -3, kwargs
        assert lib.fjagg_last_error() != b""
    torch.cuda.synchronize()
    assert np.isnan(fc.np_of(out)).all() and np.isnan(fc.np_of(diag)).all() and not fc.np_of(ws).any()
    fc.assert_same_bits(xd, x, "the deltas after the refusals")
    # the same call, accepted: the buffers are written
    assert dense() == 0
    torch.cuda.synchronize()
    want = ref.fltrust([x], [g])
    fc.assert_same_bits(out, want["mean"][0], "accepted call: mean")
    fc.assert_same_bits(diag[:K], want["cos"], "accepted call: cosines")
    # the Python surfaces refuse before the library
    sl = slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, device=cuda)
    with pytest.raises(ValueError):
        sl.fltrust(None)
    with pytest.raises(TypeError):
        sl.fltrust(gd.double())
    with pytest.raises(ValueError):
        sl.fltrust(gd[:-1])
    with pytest.raises(ValueError):
        sl.fltrust(gd, out=torch.empty(P + 1, device=cuda))
    with pytest.raises(ValueError, match="overlap"):
        sl.fltrust(gd, out=gd)
    with pytest.raises(ValueError, match="overlap"):
        sl.fltrust(gd, out=sl.storage[1, :P])
    with pytest.raises(TypeError):
        slab_mod.ClientDeltaSlab({"w": torch.zeros(P)}, K, dtype=torch.bfloat16, device=cuda).fltrust(gd)
    with pytest.raises(TypeError):
        tu.tree_fltrust([{"w": torch.zeros(4, dtype=torch.bfloat16, device=cuda)}], {"w": torch.zeros(4, device=cuda)})
    with pytest.raises(ValueError):
        tu.tree_fltrust([{"w": torch.zeros(4, device=cuda)}], {"w": torch.zeros(5, device=cuda)})
    with pytest.raises(TypeError):
        tu.tree_fltrust([{"w": torch.zeros(4, device=cuda)}], {"w": torch.zeros(4, device=cuda).double()})


def test_empty_rounds(cuda):
    assert tu.tree_fltrust([], {"z": torch.zeros(0, device=cuda)}) is None
    for e in (slab_mod.ClientDeltaSlab({"z": torch.zeros(0)}, 3, device=cuda).fltrust({"z": torch.zeros(0, device=cuda)}),
              tu.tree_fltrust([{"z": torch.zeros(0, device=cuda)}] * 3, {"z": torch.zeros(0, device=cuda)})):
        assert e.mean["z"].numel() == 0 and int(fc.np_of(e.count)) == 0
        assert not fc.np_of(e.trust).any() and fc.np_of(e.trust).shape == (3,) and np.isnan(fc.np_of(e.cosines)).all()
    # one client, one element
    x, g = np.array([[2.0]], F32), np.array([0.5], F32)
    got = tu.tree_fltrust([{"w": torch.from_numpy(x[0]).to(cuda)}], {"w": torch.from_numpy(g).to(cuda)})
    fc.check_result(got, ref.fltrust([x], [g]), "one client, one element")
    assert fc.flat_of(got.mean)[0] == 0.5
