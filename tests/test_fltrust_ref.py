"""FLTrust without a GPU: the numpy restatement of the contract (tests/fltrust_ref.py) against
itself — the order of its sums, the special clients, the clamp, the empty round, the convex bound —
the selection rule of fedjax_amd/csrc/fjtrust_dev.h built for the host against it bit for bit, and
every refusal of the C entries and of the Python surfaces that needs no device."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import _lib, kernels, tree_util
from tests import clipped_mean_ref
from tests import fltrust_host as host
from tests import fltrust_ref as ref

F32, F64 = np.float32, np.float64
NEW_SYMBOLS = ("fjagg_dotsq_rows_workspace_bytes", "fjagg_dotsq_rows", "fjagg_dotsq_dense", "fjagg_fltrust_select",
               "fjagg_fltrust_workspace_bytes", "fjagg_fltrust_dense", "fjagg_fltrust_ptrs")


def bits(a):
    return host.bits(a).tolist()


# ------------------------------------------------------------------ the order of the sums
@pytest.mark.parametrize("sizes", [(1,), (255,), (257,), (2049,), (65537,), (300, 0, 700), (2 * 65536 + 3, 5)])
def test_squares_in_product_order_have_l2sq_rows_bits(sizes):
    rng = np.random.RandomState(len(sizes) + sizes[0])
    xs = [rng.standard_normal((3, n)).astype(F32) for n in sizes]
    q = ref.product_order_sums(xs, xs)
    for k in range(3):
        assert bits(q[k]) == bits(clipped_mean_ref.l2sq_rows_ref([x[k] for x in xs]))


def test_dot_order_can_be_told_from_a_sequential_sum():
    """On near-orthogonal pairs the sign of the dot product depends on the order of its sum: the
    library's order and a plain sequential sum disagree on many seeds, so a reference that had
    degenerated to another order would be noticed."""
    differ = 0
    for seed in range(200):
        rng = np.random.RandomState(seed)
        x, g = rng.standard_normal(4096), rng.standard_normal(4096)
        x = (x - (x @ g) / (g @ g) * g).astype(F32)
        g = g.astype(F32)
        a = ref.product_order_sums([x[None]], [g])[0]
        differ += np.signbit(a) != np.signbit(ref.sequential_dot(x, g))
    print("seeds whose sign differs:", differ)
    assert differ >= 20


# ------------------------------------------------------------------ the rule
def _attack_round(P=1000, seed=0):
    """(xs, gs, names): one leaf, honest clients first, then the attack set of the prototype."""
    rng = np.random.RandomState(seed)
    g = rng.standard_normal(P).astype(F32)
    honest = [(g * F32(s) + F32(0.01) * rng.standard_normal(P).astype(F32)).astype(F32) for s in (0.5, 1.0, 2.0)]
    nan = honest[0].copy()
    nan[P // 2] = np.nan
    attacks = {"minus": -10 * g, "huge": np.full(P, 1e30, F32), "nan": nan, "zero": np.zeros(P, F32),
               "inf": np.full(P, np.inf, F32), "tiny": F32(1e-30) * g}
    rows = honest + [v.astype(F32) for v in attacks.values()]
    return [np.stack(rows)], [g], ["h0", "h1", "h2"] + list(attacks)


def test_special_clients_get_no_trust():
    xs, gs, names = _attack_round()
    got = ref.fltrust(xs, gs)
    for k, name in enumerate(names):
        if name in ("h0", "h1", "h2"):
            assert got["trust"][k] > 0.99 and got["factors"][k] > 0, name
        else:
            assert bits(got["trust"][k]) == bits(F64(0)) and bits(got["factors"][k]) == bits(F32(0)), name
    assert got["count"] == 3 and got["order"][:3].tolist() == [0, 1, 2] and not got["order"][3:].any()
    # what each special hits on its way to 0
    k = {n: i for i, n in enumerate(names)}
    assert got["cos"][k["minus"]] < -0.99
    assert np.isinf(got["q"][k["huge"]]) and np.isnan(got["cos"][k["nan"]]) and np.isnan(got["cos"][k["zero"]])
    assert np.isinf(got["q"][k["inf"]]) and got["q"][k["tiny"]] == 0
    y = got["mean"][0]
    assert np.isfinite(y).all()
    assert np.linalg.norm(y.astype(F64)) <= np.linalg.norm(gs[0].astype(F64)) * (1 + 1e-5)


@pytest.mark.parametrize("qs", [0.0, np.inf, np.nan])
def test_a_zero_or_non_finite_server_delta_trusts_nobody(qs):
    a, q = np.array([1.0, 2.0, -1.0], F32), np.array([1.0, 4.0, 1.0], F32)
    got = ref.select(a, q, F32(qs))
    assert got["count"] == 0 and not got["trust"].any() and not got["factors"].any()
    assert bits(got["total"]) == bits(F64(0)) and bits(got["gscale"]) == bits(F32(0))


def test_the_clamp_holds_a_cosine_at_one():
    """Exact multiples of g: the float32 sums put cos a little over 1 for some, and ts stays 1."""
    rng = np.random.RandomState(1)
    g = rng.standard_normal(4097).astype(F32)
    xs = [g[None] * rng.uniform(0.1, 10.0, 64).astype(F32)[:, None]]
    got = ref.fltrust(xs, [g])
    print("largest cosine - 1:", got["cos"].max() - 1)
    assert 1 < got["cos"].max() <= 1 + 1.5e-7 and got["trust"].max() == 1.0
    assert (got["trust"] == np.minimum(got["cos"], 1.0)).all()
    a, q = np.array([1.0000001], F32), np.array([1.0], F32)
    one = ref.select(a, q, F32(1.0))
    assert one["cos"][0] > 1 and one["trust"][0] == 1.0 and one["factors"][0] == 1.0


def test_nobody_trusted_gives_all_plus_zero():
    rng = np.random.RandomState(2)
    g = rng.standard_normal(300).astype(F32)
    got = ref.fltrust([np.stack([-g, -2 * g, np.zeros_like(g)])], [g])
    assert got["count"] == 0 and bits(got["total"]) == bits(F64(0))
    assert not np.asarray(bits(got["mean"][0])).any()  # +0, not -0
    assert not got["order"].any() and not got["wperm"].any() and got["seg"].tolist() == [0, 0]


@pytest.mark.parametrize("P", [1000, 4097, 65539])
@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_convex_bound_on_positive_multiples(P, noise):
    """y is a convex combination of vectors of norm n_s, so |y| <= |g| up to rounding."""
    K = 64
    rng = np.random.RandomState(P)
    g = rng.standard_normal(P).astype(F32)
    scales = rng.uniform(0.1, 10.0, K).astype(F32)
    x = g[None] * scales[:, None]
    if noise:
        x = x + F32(noise) * scales[:, None] * rng.standard_normal((K, P)).astype(F32)
    got = ref.fltrust([x.astype(F32)], [g])
    assert got["count"] == K
    ratio = np.linalg.norm(got["mean"][0].astype(F64)) / np.linalg.norm(g.astype(F64))
    print(f"P={P} noise={noise}: |y|/|g| - 1 = {ratio - 1:.3e}")
    assert ratio <= 1 + 1e-5
    assert ratio - 1 < 1e-8  # the reference's own excess


# ------------------------------------------------------------------ the host build of the rule
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return host.build(tmp_path_factory.mktemp("fltrust_select"), sanitize=True)


def test_host_build_of_the_rule_equals_numpy(host_program, tmp_path):
    cases = [host.seeded_rows(seed, 1 + (seed * 37) % 130) for seed in range(200)]
    cases += [host.seeded_rows(1000, 4096), (np.array([1.0000001], F32), np.array([1.0], F32), F32(1.0))]
    got = host.run(host_program, cases, tmp_path)
    trusted = 0
    for i, ((a, q, qs), g) in enumerate(zip(cases, got)):
        want = ref.select(a, q, qs)
        host.same(g, want, f"case {i}")
        s = F32(0)
        with np.errstate(all="ignore"):
            for v in a:
                s = s + v
        assert bits(g["combined"]) == bits(s) or (np.isnan(s) and np.isnan(g["combined"]))
        trusted += int(want["count"])
    assert trusted > 1000  # (the cases are not all gated out)


# ------------------------------------------------------------------ refusals that need no GPU
def test_the_new_entries_are_declared_and_exported():
    for sym in NEW_SYMBOLS:
        assert sym in _lib.SYMBOLS
        assert hasattr(_lib.load(), sym)
    assert _lib.load().fjagg_abi_version() == 4


def _err():
    return _lib.load().fjagg_last_error().decode()


def test_c_entries_refuse_with_nothing_launched():
    lib = _lib.load()
    A = 1 << 20  # plausible non-null, 16-byte aligned addresses; never dereferenced
    ws = lib.fjagg_fltrust_workspace_bytes(8, 1, 100)
    assert ws > 0 and lib.fjagg_fltrust_workspace_bytes(0, 1, 100) == 0

    def dense(dtype=_lib.F32, x=A, ld=100, K=8, P=100, tab=None, L=1, max_n=100, g=2 * A, out=3 * A, cos=4 * A,
              ws_ptr=5 * A, ws_bytes=ws, flags=0):
        d = [4 * A + 4096 * i for i in range(1, 7)]  # the other six diagnostics
        return lib.fjagg_fltrust_dense(dtype, x, ld, K, P, tab, L, max_n, g, out, cos, *d, ws_ptr, ws_bytes, flags, None)

    for kwargs, word in [(dict(dtype=_lib.BF16), "float32"), (dict(K=0), "clients"), (dict(K=4097), "4096"),
                         (dict(P=0), "P"), (dict(ld=99), "ld"), (dict(P=(1 << 28) + 1, ld=(1 << 28) + 1), "1 GiB"),
                         (dict(x=None), "null"), (dict(g=None), "null"), (dict(out=None), "null"),
                         (dict(cos=None), "null"), (dict(ws_ptr=None), "workspace"), (dict(ws_bytes=ws - 1), "workspace"),
                         (dict(ws_ptr=5 * A + 8), "aligned"), (dict(out=A + 400), "overlaps the deltas"),
                         (dict(out=A + 100 * 4 * 7 + 396), "overlaps the deltas"), (dict(out=2 * A + 396), "server"),
                         (dict(out=2 * A - 396), "server"), (dict(out=5 * A), "workspace or a diagnostics"),
                         (dict(out=5 * A - 396), "workspace or a diagnostics"), (dict(out=4 * A), "diagnostics"),
                         (dict(out=4 * A + 6 * 4096 - 396), "diagnostics"), (dict(flags=_lib.SCALE), "flags"),
                         (dict(flags=_lib.UNALIGNED), "flags"), (dict(flags=_lib.ACCUMULATE), "flags"),
                         (dict(flags=_lib.HOST_TABLES), "flags"), (dict(L=2), "leaf table"),
                         (dict(tab=6 * A, L=65536), "leaf table"), (dict(tab=6 * A, L=2, max_n=101), "leaf table")]:
        assert dense(**kwargs) == -3, kwargs
        assert word in _err(), (kwargs, _err())

    def ptrs(dtype=_lib.F32, all_=A, group=2 * A, L=2, K=8, nblk=3, max_n=100, cos=4 * A, ws_ptr=5 * A, ws_bytes=None,
             flags=0):
        if ws_bytes is None:
            ws_bytes = lib.fjagg_fltrust_workspace_bytes(8, 2, 100)
        d = [4 * A + 4096 * i for i in range(1, 7)]
        return lib.fjagg_fltrust_ptrs(dtype, all_, group, L, K, nblk, max_n, cos, *d, ws_ptr, ws_bytes, flags, None)

    for kwargs, word in [(dict(dtype=_lib.BF16), "float32"), (dict(K=0), "clients"), (dict(K=4097), "4096"),
                         (dict(nblk=0), "plan"), (dict(L=0), "plan"), (dict(L=65536), "plan"),
                         (dict(max_n=(1 << 28) + 1), "1 GiB"), (dict(all_=None), "null"), (dict(group=None), "null"),
                         (dict(cos=None), "null"), (dict(ws_bytes=16), "workspace"), (dict(flags=_lib.SCALE), "flags"),
                         (dict(flags=_lib.NARROW), "flags")]:
        assert ptrs(**kwargs) == -3, kwargs
        assert word in _err(), (kwargs, _err())

    rows_ws = lib.fjagg_dotsq_rows_workspace_bytes(6, 100)
    assert rows_ws == 2 * 6 * 4 and lib.fjagg_dotsq_rows_workspace_bytes(6, 65537) == 2 * 6 * 2 * 4
    for args, word in [((_lib.BF16, A, 6, 100, 1, A, A, A, rows_ws, None), "float32"),
                       ((_lib.F32, A, 0, 100, 1, A, A, A, rows_ws, None), "grouping"),
                       ((_lib.F32, A, 6, 100, 4, A, A, A, rows_ws, None), "grouping"),
                       ((_lib.F32, A, 6, (1 << 28) + 1, 1, A, A, A, 1 << 40, None), "1 GiB"),
                       ((_lib.F32, A, 6, 100, 1, A, A, A, rows_ws - 1, None), "workspace"),
                       ((_lib.F32, None, 6, 100, 1, A, A, A, rows_ws, None), "null"),
                       ((_lib.F32, A, 6, 100, 1, A, None, A, rows_ws, None), "null")]:
        assert lib.fjagg_dotsq_rows(*args) == -3, args
        assert word in _err(), (args, _err())
    for args, word in [((_lib.F32, A, 100, 4097, 100, None, 1, 100, A, A, A, A, 1 << 30, 0, None), "4096"),
                       ((_lib.F32, A, 100, 8, 100, None, 1, 100, None, A, A, A, 1 << 30, 0, None), "null"),
                       ((_lib.F32, A, 100, 8, 100, None, 1, 100, A, A, A, A, 63, 0, None), "workspace"),
                       ((_lib.F32, A, 100, 8, 100, None, 1, 100, A, A, A, A, 1 << 30, _lib.UNALIGNED, None), "flags")]:
        assert lib.fjagg_dotsq_dense(*args) == -3, args
        assert word in _err(), (args, _err())
    sel = [A, A, A, 8] + [A] * 11 + [None]
    for change, word in [({3: 0}, "clients"), ({3: 4097}, "4096"), ({0: None}, "null"), ({7: None}, "null"),
                         ({14: None}, "null")]:
        args = list(sel)
        for i, v in change.items():
            args[i] = v
        assert lib.fjagg_fltrust_select(*args) == -3, change
        assert word in _err(), (change, _err())


def test_kernel_wrappers_check_before_the_library():
    x = torch.zeros(4, 10)
    g = torch.zeros(10)
    with pytest.raises(TypeError):
        kernels.fltrust_dense(x.double(), g)
    with pytest.raises(ValueError):
        kernels.fltrust_dense(x[:, ::2], g[:5])
    with pytest.raises(ValueError):
        kernels.fltrust_dense(torch.zeros(4097, 2), torch.zeros(2))
    with pytest.raises(ValueError):
        kernels.fltrust_dense(torch.zeros(0, 2), torch.zeros(2))
    with pytest.raises(ValueError):
        kernels.fltrust_dense(x, torch.zeros(9))
    with pytest.raises(TypeError):
        kernels.fltrust_dense(x, g.double())
    with pytest.raises(ValueError):
        kernels.fltrust_dense(x, g, out=torch.zeros(11))
    with pytest.raises(ValueError, match="server"):
        kernels.fltrust_dense(x, g, out=g)
    with pytest.raises(ValueError, match="deltas"):
        kernels.fltrust_dense(x, g, out=x[1])
    with pytest.raises(TypeError):
        kernels.fltrust_dense(x, g, leaf_table=torch.zeros(3, dtype=torch.int64), max_n=1)
    with pytest.raises(ValueError):
        kernels.fltrust_dense(x, g, leaf_table=torch.zeros(2, dtype=torch.int64), max_n=11)
    with pytest.raises(ValueError):  # all checked: what is left is that these are host tensors
        kernels.fltrust_dense(x, g)
    with pytest.raises(ValueError):
        kernels.dotsq_dense(x, torch.zeros(9))
    with pytest.raises(ValueError):
        kernels.dotsq_rows(torch.zeros(8, dtype=torch.int64), 3, 10)
    with pytest.raises(TypeError):
        kernels.dotsq_rows(torch.zeros(9, dtype=torch.int32), 3, 10)
    with pytest.raises(ValueError):
        kernels.dotsq_rows(torch.zeros(9, dtype=torch.int64), 3, 10, rows_per_group=2)
    with pytest.raises(TypeError):
        kernels.fltrust_select(torch.zeros(4), torch.zeros(5), torch.zeros(1))
    with pytest.raises(ValueError):
        kernels.fltrust_select(torch.zeros(4), torch.zeros(4), torch.zeros(2))
    with pytest.raises(ValueError):
        kernels.fltrust_select(torch.zeros(4097), torch.zeros(4097), torch.zeros(1))
    img = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError):
        kernels.fltrust_ptrs(img, img, 2, 4097, 1, 10)
    with pytest.raises(ValueError):
        kernels.fltrust_ptrs(img[:11], img, 2, 4, 1, 10)
    with pytest.raises(ValueError):
        kernels.fltrust_ptrs(img, img[:13], 2, 4, 1, 10)
    with pytest.raises(TypeError):
        kernels.fltrust_ptrs(img.int(), img, 2, 4, 1, 10)


def test_tree_and_aggregator_refusals():
    assert tree_util.tree_fltrust([], {"w": torch.zeros(2)}) is None
    with pytest.raises(ValueError, match="4096"):
        tree_util.tree_fltrust([{"w": torch.zeros(1)}] * 4097, {"w": torch.zeros(1)})
    agg = fedjax_amd.aggregators.fltrust_aggregator()
    state = agg.init()
    assert state.server_delta is None and state.trust == {} and state.factors == {}
    with pytest.raises(ValueError, match="server_delta"):
        agg.apply([("a", {"w": torch.zeros(2)}, 1.0)], state)
    with pytest.raises(ValueError, match="server_delta"):
        agg.apply([], state)
    ready = state.replace(server_delta={"w": torch.zeros(2)})
    assert ready.server_delta is not None and state.server_delta is None
    got, after = agg.apply([], ready)  # no clients: None, the state as it was
    assert got is None and after is ready
