"""The clipped fold with the server step in its epilogue (k_dense_clip_opt / k_ptrs_clip_opt
through fjagg_server_update_clip_dense / _ptrs, server.fused_clipped_mean_update and
server.fused_tree_clipped_mean_update; fedjax/algorithms/mime_lite.py:131-149, then :162-167)
against the numpy restatement in tests/clipped_update_ref.py bit for bit, against the library's
own two-step route (the clipped mean, then the fused step on it), and against the float64 rules.

Bitwise checks use the clip factors restated from the returned device norms, as
tests/test_gpu_clipped_mean.py's check_clipped_mean does; the norms themselves are held to
NORM_RTOL of a float64 norm. Bit patterns are compared with every NaN mapped to one pattern.
Every case that clips uses max_norm = the median float64 norm and asserts that some clients are
clipped and some are not (K = 1 cannot: it clips its only client at 0.75 of its norm).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, pytree, server, slab as slab_mod, tree_util as tu
from oracle import optax_rules_ref as rules
from tests import clipped_mean_ref as ref
from tests.clipped_update_ref import clipped_update_ref, inverse_total
from tests.test_clipped_update_ref import mime_lite_fixture
from tests.test_gpu_clipped_mean import (LEAF_NAMES, LEAF_P, LEAF_SHAPES, NORM_RTOL, assert_bits, client_trees,
                                         deltas, nbits, weight_sets)
from tests.test_server_rules_ref import HYPER, hyper_id, make_server, probe_state, rule_kwargs

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = F32(-1234.5)
ADAM = HYPER[3]
RULES = pytest.mark.parametrize("hi", range(len(HYPER)), ids=[hyper_id(h) for h in HYPER])


def to_dev(a, cuda):
    return torch.from_numpy(np.array(a, dtype=F32)).to(cuda)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def clip_norm(x):
    """The median float64 norm; for one client 0.75 of its norm."""
    n64 = ref.f64_norms(x)
    return float(np.median(n64)) if x.shape[0] > 1 else 0.75 * float(n64[0])


def restated_factors(got, x, C, what, mixed=True):
    """The factors restated from the returned norms, after holding the norms to NORM_RTOL of
    float64 and the flags to (c != 1)."""
    K = x.shape[0]
    norms = host(got.norms)
    assert norms.dtype == F32 and norms.shape == (K,)
    with np.errstate(all="ignore"):
        n64 = ref.f64_norms(x)
        fin = np.isfinite(n64)
        assert (np.abs(norms - n64)[fin] <= NORM_RTOL * n64[fin]).all(), what
        assert np.array_equal(nbits(norms[~fin]), nbits(n64[~fin].astype(F32))), what  # inf stays inf, NaN NaN
    c = ref.clip_factors_ref(norms, C)
    clipped = host(got.clipped)
    assert clipped.dtype == np.bool_ and (clipped == (c != 1)).all(), what
    if mixed:
        assert (clipped.any() and not clipped.all()) if K > 1 else clipped.all(), \
            f"{what}: the case must clip some clients and not others"
    return c


def check_clipped_norms(got, x, c, what):
    norms, cn, clipped = host(got.norms), host(got.clipped_norms), host(got.clipped)
    assert (nbits(cn)[~clipped] == nbits(norms)[~clipped]).all(), what  # verbatim where nothing was clipped
    with np.errstate(all="ignore"):
        p64 = ref.f64_norms(ref.clipped_products(x, c))
        ok = clipped & np.isfinite(p64)
        assert (np.abs(cn - p64)[ok] <= NORM_RTOL * p64[ok]).all(), what


def same_diagnostics(got, cm, what, clipped_norms=True):
    """``got`` (a ClippedUpdate) carries the bits of the ClippedMean ``cm`` of the same deltas."""
    assert torch.equal(got.norms.view(torch.int32), cm.norms.view(torch.int32)), f"{what}: norms"
    assert torch.equal(got.clipped, cm.clipped), f"{what}: clipped"
    if clipped_norms:
        assert torch.equal(got.clipped_norms.view(torch.int32), cm.clipped_norms.view(torch.int32)), \
            f"{what}: clipped norms"
    else:
        assert got.clipped_norms is None


def make_slab(x, cuda, template=None):
    K, P = x.shape
    sl = slab_mod.ClientDeltaSlab(template if template is not None else {"w": np.zeros(P, F32)}, K, device=cuda)
    assert sl.num_params == P
    sl.rows.copy_(torch.from_numpy(np.array(x)))
    return sl


def dev_state(m, v, count, cuda, wrap=lambda t: t):
    st = {"count": count}
    if m is not None:
        st["m"] = wrap(to_dev(m, cuda))
    if v is not None:
        st["v"] = wrap(to_dev(v, cuda))
    return st


# --------------------------------------------------------------- pytree helpers
CUTS = np.cumsum([0] + [int(np.prod(s)) for s in LEAF_SHAPES])


def tree_of(vec, cuda):
    return {n: to_dev(vec[CUTS[i]:CUTS[i + 1]], cuda).reshape(s) for i, (n, s) in enumerate(zip(LEAF_NAMES, LEAF_SHAPES))}


def flat_tree(tree):
    return np.concatenate([host(tree[n]).reshape(-1) for n in LEAF_NAMES])


@functools.lru_cache(maxsize=None)
def tree_case(K, seed, cuda):
    """(x [K, LEAF_P], the clients' device trees: leaf "d" 4 bytes off alignment), made once and never written."""
    x = deltas(K, LEAF_P, seed=seed)
    return x, client_trees(x, cuda)


# ----------------------------------- 1. slab route, two rounds, every rule, bitwise the reference
@RULES
def test_slab_two_rounds_every_rule(cuda, hi):
    h, K, P = HYPER[hi], 9, 1027  # 16-byte units, a 3-element tail, one tile
    opt = make_server(h)
    p, m, v = probe_state(h, P, seed=70 + hi)
    count = 0
    params, state = to_dev(p, cuda), dev_state(m, v, 0, cuda)
    for rnd in range(2):
        x = deltas(K, P, seed=20 + rnd)
        sl = make_slab(x, cuda)
        C, weights = clip_norm(x), weight_sets(K, K + rnd)["int" if rnd else "float"]
        mean_out = torch.full((P,), float(SENTINEL), device=cuda)
        before = state
        got = server.fused_clipped_mean_update(sl, weights, C, opt, params, state, mean_out=mean_out)
        assert isinstance(got, server.ClippedUpdate) and got.state is not before
        what = f"slab {hyper_id(h)} round {rnd + 1}"
        c = restated_factors(got, x, C, what)
        p, m, v, count, mean = clipped_update_ref(x, weights, c, opt, p, m, v, count)
        state = got.state
        assert state["count"] == count == rnd + 1
        assert_bits(params, p, what + " params")
        assert_bits(mean_out, mean, what + " mean_out")
        for key, want in (("m", m), ("v", v)):
            assert (key in state) == (want is not None)
            if want is not None:
                assert state[key] is before[key]  # updated in place
                assert_bits(state[key], want, f"{what} {key}")
        check_clipped_norms(got, x, c, what)
        same_diagnostics(got, sl.clipped_mean(weights, C), what)
        assert_bits(sl.rows, x, "the slab is not written")


# ------------------------------------------------------------------ 2. every dense shape, adam
def _dense_case(x, cuda, ld, what):
    """The raw dense launch over x with row stride ld, adam at count 3: with and without the
    clipped squares and with non-temporal loads, each bitwise the restatement; the squares are
    the clipped fold's own on the same deltas."""
    K, P = x.shape
    opt = make_server(ADAM)
    store = torch.full((K, ld), float("nan"), dtype=torch.float32, device=cuda)  # the padding is never read
    store[:, :P].copy_(torch.from_numpy(np.array(x)))
    xd = store[:, :P]
    assert xd.stride(0) == ld
    C = clip_norm(x)
    with np.errstate(all="ignore"):
        norms = np.sqrt((np.asarray(x, np.float64) ** 2).sum(axis=1)).astype(F32)
    c = ref.clip_factors_ref(norms, C)
    assert ((c != 1).any() and not (c != 1).all()) if K > 1 else (c != 1).all(), what
    weights = weight_sets(K, K + P % 97)["int"]
    w32 = np.array(weights, dtype=F32)
    scale = inverse_total(weights)
    p0, m0, v0 = probe_state(ADAM, P, seed=P % 89)
    p, m, v, _, mean = clipped_update_ref(x, weights, c, opt, p0, m0, v0, 2)
    wd, cd = to_dev(w32, cuda), to_dev(c, cuda)
    _, l2_want = kernels.clipped_sum_dense(xd, wd, cd, scale=float(scale), with_clipped_l2sq=True)
    for nt, with_l2 in ((False, True), (False, False), (True, True), (True, False)):
        tag = f"{what} nt={nt} l2={with_l2}"
        pd, md, vd = to_dev(p0, cuda), to_dev(m0, cuda), to_dev(v0, cuda)
        mo = torch.full((P,), float(SENTINEL), device=cuda)
        l2 = kernels.clipped_update_dense(xd, wd, cd, float(scale), opt.descriptor(3), pd, md, vd, mo,
                                          nontemporal=nt, with_clipped_l2sq=with_l2)
        assert_bits(pd, p, tag + " params")
        assert_bits(md, m, tag + " m")
        assert_bits(vd, v, tag + " v")
        assert_bits(mo, mean, tag + " mean")
        if with_l2:
            assert torch.equal(l2.view(torch.int32), l2_want.view(torch.int32)), tag + " clipped squares"
        else:
            assert l2 is None
        # without mean_out the mean is never stored and the step is the same
        pd2, md2, vd2 = to_dev(p0, cuda), to_dev(m0, cuda), to_dev(v0, cuda)
        kernels.clipped_update_dense(xd, wd, cd, float(scale), opt.descriptor(3), pd2, md2, vd2, None,
                                     nontemporal=nt, with_clipped_l2sq=with_l2)
        assert torch.equal(pd2.view(torch.int32), pd.view(torch.int32)), tag + " without mean_out"


@pytest.mark.parametrize("P", [1, 3, 4, 1027, 8197])
def test_dense_every_shape(cuda, P):
    for K in (1, 2, 9, 33):
        x = deltas(K, P, seed=4)
        # an aligned stride (16-byte units + tail) and an odd one (element units)
        for ld in ((P + 3) // 4 * 4 + 4, P + 1 + (P % 2)):
            _dense_case(x, cuda, ld, f"K={K} P={P} ld={ld}")


def test_dense_e8_u4_shape(cuda):
    """K = 33, P = 2**20 + 3: the smallest case where pick_variant returns 12 (E=8 x U=4)."""
    K, P = 33, (1 << 20) + 3
    g = torch.Generator().manual_seed(12)
    x = torch.randn(K, P, generator=g, dtype=torch.float32)
    x *= torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], dtype=torch.float32)[:, None]
    _dense_case(x.numpy(), cuda, (P + 3) // 4 * 4 + 4, f"K={K} P={P}")


# ------------------------------------------------- 3. pytree route, two rounds, every rule
@RULES
def test_pytree_two_rounds_every_rule(cuda, hi):
    h = HYPER[hi]
    opt = make_server(h)
    for K in (1, 5, 33, 130):
        p, m, v = probe_state(h, LEAF_P, seed=90 + hi)
        count = 0
        params = tree_of(p, cuda)
        state = dev_state(m, v, 0, cuda, wrap=lambda t: tree_of(host(t), cuda))
        for rnd in range(2):
            x, trees = tree_case(K, 30 + rnd, cuda)
            C, weights = clip_norm(x), weight_sets(K, 100 + K + rnd)["float" if rnd else "int"]
            pairs = list(zip(trees, weights))
            mean_out = tree_of(np.full(LEAF_P, SENTINEL, F32), cuda)
            with_norms = not (rnd == 1 and K == 5)  # one case without the clipped squares
            got = server.fused_tree_clipped_mean_update(pairs, C, opt, params, state, mean_out=mean_out,
                                                        with_clipped_norms=with_norms)
            what = f"pytree {hyper_id(h)} K={K} round {rnd + 1}"
            c = restated_factors(got, x, C, what)
            p, m, v, count, mean = clipped_update_ref(x, weights, c, opt, p, m, v, count)
            state = got.state
            assert state["count"] == count
            assert_bits(flat_tree(params), p, what + " params")
            assert_bits(flat_tree(mean_out), mean, what + " mean_out")
            for key, want in (("m", m), ("v", v)):
                assert (key in state) == (want is not None)
                if want is not None:
                    assert_bits(flat_tree(state[key]), want, f"{what} {key}")
            if with_norms:
                check_clipped_norms(got, x, c, what)
            same_diagnostics(got, tu.tree_clipped_mean(pairs, C), what, clipped_norms=with_norms)


def test_reference_fixture_through_the_pytree_route(cuda):
    """mime_lite_test.py:92-119 through fused_tree_clipped_mean_update: params 3.904, clipped
    norms 0.5 and 0.45000005 at the reference's tolerance, and the restated round's bits."""
    x, weights, C, lr, p0, want = mime_lite_fixture()
    trees = [{"w": to_dev(x[k, 0], cuda)} for k in range(2)]
    params = {"w": to_dev(p0[0], cuda)}
    opt = server.sgd(lr)
    got = server.fused_tree_clipped_mean_update(zip(trees, weights), C, opt, params, opt.init(params))
    assert got.state == {"count": 1}
    np.testing.assert_allclose(host(params["w"]), 3.904)
    np.testing.assert_allclose(host(got.clipped_norms), [0.5, 0.45000005])
    assert host(got.clipped).tolist() == [True, False]
    assert nbits(host(params["w"])) == nbits(want["params"])
    # the slab route: the same bits
    sl = make_slab(x, cuda)
    flat = to_dev(p0, cuda)
    got2 = server.fused_clipped_mean_update(sl, weights, C, opt, flat, opt.init(flat))
    assert nbits(host(flat))[0] == nbits(want["params"]) and got2.state == {"count": 1}
    assert torch.equal(got2.clipped_norms.view(torch.int32), got.clipped_norms.view(torch.int32))


# ------------------------------ 4. the fused route against the two-step route, every rule
@RULES
def test_slab_equals_clipped_mean_then_fused_step(cuda, hi):
    h, K, P = HYPER[hi], 9, 1027
    opt = make_server(h)
    p, m, v = probe_state(h, P, seed=50 + hi)
    template = {"u": np.zeros(27, F32), "w": np.zeros(P - 27, F32)}
    pa, pb = to_dev(p, cuda), to_dev(p, cuda)
    sa = dev_state(m, v, 0, cuda)
    for rnd in range(2):
        x = deltas(K, P, seed=40 + rnd)
        sl = make_slab(x, cuda, template)
        if rnd == 0:
            sb = dev_state(m, v, 0, cuda, wrap=sl.unflatten)
        C, weights = clip_norm(x), weight_sets(K, 7 + rnd)["float"]
        sa = server.fused_clipped_mean_update(sl, weights, C, opt, pa, sa).state
        cm = sl.clipped_mean(weights, C)
        sb = server.fused_tree_mean_update([(cm.mean, 1.0)], opt, sl.unflatten(pb), sb)
        assert sa["count"] == sb["count"] == rnd + 1
        assert_bits(pa, host(pb), f"params round {rnd + 1}")
        for key in ("m", "v"):
            if key in sa:
                wantv = torch.cat([t.reshape(-1) for t in pytree.leaves_of(sb[key])])
                assert_bits(sa[key], host(wantv), f"{key} round {rnd + 1}")


@RULES
def test_pytree_equals_clipped_mean_then_fused_step(cuda, hi):
    h, K = HYPER[hi], 5
    opt = make_server(h)
    p, m, v = probe_state(h, LEAF_P, seed=55 + hi)
    wrap = lambda t: tree_of(host(t), cuda)
    pa, pb = tree_of(p, cuda), tree_of(p, cuda)
    sa, sb = dev_state(m, v, 0, cuda, wrap=wrap), dev_state(m, v, 0, cuda, wrap=wrap)
    for rnd in range(2):
        x, trees = tree_case(K, 30 + rnd, cuda)
        C, weights = clip_norm(x), weight_sets(K, 17 + rnd)["int"]
        pairs = list(zip(trees, weights))
        sa = server.fused_tree_clipped_mean_update(pairs, C, opt, pa, sa).state
        cm = tu.tree_clipped_mean(pairs, C)
        sb = server.fused_tree_mean_update([(cm.mean, 1.0)], opt, pb, sb)
        assert sa["count"] == sb["count"] == rnd + 1
        assert_bits(flat_tree(pa), flat_tree(pb), f"params round {rnd + 1}")
        for key in ("m", "v"):
            if key in sa:
                assert_bits(flat_tree(sa[key]), flat_tree(sb[key]), f"{key} round {rnd + 1}")


# ------------------------------------------------------------------ 5. special values
def _special_cases():
    K, P = 9, 1027
    base = np.array(deltas(K, P, seed=8))
    C = clip_norm(base)
    ints = weight_sets(K, 3)["int"]
    inf_x = base.copy()
    inf_x[1, 5] = np.inf  # norm inf, factor 0, the product 0 * inf is NaN at that element alone
    nan_x = base.copy()
    nan_x[2, P // 2] = np.nan  # norm NaN, factor NaN: every element of the mean
    zero_x = base.copy()
    zero_x[3, :] = 0.0  # norm 0: max_norm / 0 = inf, factor 1
    return [("an inf element", inf_x, ints, C), ("a NaN element", nan_x, ints, C),
            ("an all-zero client", zero_x, ints, C), ("max_norm 0", base, ints, 0.0),
            ("max_norm 0 and an all-zero client", zero_x, ints, 0.0),  # 0 / 0: a NaN factor
            ("max_norm inf", base, ints, float("inf")), ("a zero total weight", base, [0] * K, C)]


@pytest.mark.parametrize("route", ["slab", "pytree"])
def test_special_values(cuda, route):
    opt = make_server(ADAM)
    for what, x, weights, C in _special_cases():
        K, P = x.shape
        p0, m0, v0 = probe_state(ADAM, P, seed=21)
        sl = make_slab(x, cuda)
        params = to_dev(p0, cuda)
        state = dev_state(m0, v0, 4, cuda)
        mean_out = torch.full((P,), float(SENTINEL), device=cuda)
        if route == "slab":
            got = server.fused_clipped_mean_update(sl, weights, C, opt, params, state, mean_out=mean_out)
            cm = sl.clipped_mean(weights, C)
        else:
            pairs = [(sl.client(k), w) for k, w in enumerate(weights)]
            wrap = lambda t: {"w": t}
            got = server.fused_tree_clipped_mean_update(pairs, C, opt, wrap(params), {k_: (wrap(v_) if k_ != "count" else v_)
                                                                                  for k_, v_ in state.items()},
                                                        mean_out=wrap(mean_out))
            cm = tu.tree_clipped_mean(pairs, C)
        tag = f"{route}: {what}"
        c = restated_factors(got, x, C, tag, mixed=False)
        p, m, v, count, mean = clipped_update_ref(x, weights, c, opt, p0, m0, v0, 4)
        assert got.state["count"] == count == 5
        assert_bits(params, p, tag + " params")
        assert_bits(state["m"], m, tag + " m")
        assert_bits(state["v"], v, tag + " v")
        assert_bits(mean_out, mean, tag + " mean")
        same_diagnostics(got, cm, tag)
        ch, nh = host(got.clipped), host(got.norms)
        if what == "an inf element":
            assert np.isinf(nh[1]) and c[1] == 0 and np.isnan(mean[5]) and np.isfinite(np.delete(mean, 5)).all()
        elif what == "a NaN element":
            assert np.isnan(nh[2]) and np.isnan(c[2]) and ch[2] and np.isnan(mean).all()
        elif what == "an all-zero client":
            assert nh[3] == 0 and c[3] == 1 and not ch[3] and np.isfinite(mean).all()
        elif what == "max_norm 0":
            assert (c == 0).all() and ch.all() and (mean == 0).all()
        elif what == "max_norm 0 and an all-zero client":
            assert np.isnan(c[3]) and np.isnan(mean).all()
        elif what == "max_norm inf":
            assert (c == 1).all() and not ch.any()
            assert torch.equal(got.norms.view(torch.int32), got.clipped_norms.view(torch.int32))
        else:
            assert (mean == 0).all() and ch.any() and not ch.all()  # scale 0: a zero mean still steps adam's moments


# ------------------------------------------------------------------ 6. the float64 rules
@pytest.mark.parametrize("route", ["slab", "pytree"])
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_one_round_against_float64_rules(cuda, h, route):
    """One round per rule held to oracle/optax_rules_ref.step under that module's own bound, at
    the counts 1, 7 and 1000; the clipped mean given to the rules is the restated one."""
    opt = make_server(h)
    K = 9
    n = 1027 if route == "slab" else LEAF_P
    x = (np.array(deltas(K, n, seed=9)) * F32(0.02)).astype(F32)  # the probe gradients' magnitude
    C, weights = clip_norm(x), weight_sets(K, 5)["float"]
    sl = make_slab(x, cuda) if route == "slab" else None
    trees = client_trees(x, cuda) if route == "pytree" else None
    for t0 in (0, 6, 999):
        ps, ms, vs = probe_state(h, n, seed=60 + t0 % 7)
        if route == "slab":
            params, state = to_dev(ps, cuda), dev_state(ms, vs, t0, cuda)
            got = server.fused_clipped_mean_update(sl, weights, C, opt, params, state)
            flat = host
        else:
            params = tree_of(ps, cuda)
            state = dev_state(ms, vs, t0, cuda, wrap=lambda t: tree_of(host(t), cuda))
            got = server.fused_tree_clipped_mean_update(list(zip(trees, weights)), C, opt, params, state)
            flat = flat_tree
        c = restated_factors(got, x, C, f"{route} t={t0 + 1}")
        mean = ref.clipped_fold_ref(x, np.array([F32(w) for w in weights], F32), c, inverse_total(weights))
        assert got.state["count"] == t0 + 1
        want = rules.step(h["kind"], t0 + 1, mean, ps, ms, vs, **rule_kwargs(h))
        have = {"p": flat(params)}
        have.update({k_: flat(got.state[k_]) for k_ in ("m", "v") if k_ in want})
        for key, (r, bound) in want.items():
            ok = rules.within(have[key], r, bound)
            worst = float(np.max(np.abs(have[key].astype(np.float64) - r) / np.maximum(bound, 1e-300)))
            print(f"{route} {hyper_id(h)} t={t0 + 1} {key}: max |gpu - ref| / bound = {worst:.3g}")
            assert ok.all(), (route, t0, key, int((~ok).sum()), worst)


# ------------------------------------------------------- 7. frozen leaves and adafactor
FROZEN_SHAPES = {"m0": {"a": (3,), "b": (64,)}, "m1": {"c": (13, 79), "d": (5,)}}
FROZEN_P = 3 + 64 + 13 * 79 + 5


def test_frozen_leaves_both_routes(cuda):
    """ignore_grads_haiku: the clip norm covers the frozen leaves, the step does not. Frozen
    params and state are untouched, their mean_out is filled, the trainable leaves are bitwise
    the reference, and the diagnostics are the clipped mean's."""
    K = 9
    opt0 = make_server(ADAM)
    opt = server.ignore_grads_haiku(opt0, [("m0", "b"), ("m1", "d")])
    frozen = np.zeros(FROZEN_P, dtype=bool)
    frozen[3:67] = True
    frozen[-5:] = True
    template = {mk: {k_: np.zeros(s, F32) for k_, s in sub.items()} for mk, sub in FROZEN_SHAPES.items()}
    p0, m0, v0 = probe_state(ADAM, FROZEN_P, seed=33)
    x = deltas(K, FROZEN_P, seed=10)
    sl = make_slab(x, cuda, template)
    C, weights = clip_norm(x), weight_sets(K, 2)["int"]
    cm = sl.clipped_mean(weights, C)
    for route in ("slab", "pytree"):
        params, state = to_dev(p0, cuda), dev_state(m0, v0, 0, cuda)
        mean_out = torch.full((FROZEN_P,), float(SENTINEL), device=cuda)
        if route == "slab":
            got = server.fused_clipped_mean_update(sl, weights, C, opt, params, state, mean_out=mean_out)
            assert got.state["m"] is state["m"] and got.state["v"] is state["v"]
        else:
            tstate = {"count": 0, "m": sl.unflatten(state["m"]), "v": sl.unflatten(state["v"])}
            pairs = [(sl.client(k), w) for k, w in enumerate(weights)]
            got = server.fused_tree_clipped_mean_update(pairs, C, opt, sl.unflatten(params), tstate,
                                                        mean_out=sl.unflatten(mean_out))
            cm = tu.tree_clipped_mean(pairs, C)  # the clipped squares' order is the route's own
        c = restated_factors(got, x, C, route)
        p, m, v, count, mean = clipped_update_ref(x, weights, c, opt0, p0, m0, v0, 0)
        assert got.state["count"] == 1  # the count still advances
        for name, have, want, init in (("params", params, p, p0), ("m", state["m"], m, m0), ("v", state["v"], v, v0)):
            have = host(have)
            assert_bits(have[frozen], init[frozen], f"{route} {name}: a frozen leaf moved")
            assert_bits(have[~frozen], want[~frozen], f"{route} {name}")
        assert_bits(mean_out, mean, f"{route} mean_out, frozen leaves included")
        same_diagnostics(got, cm, route)


def test_adafactor_falls_back_to_clipped_mean_then_apply(cuda):
    K = 9
    opt = server.adafactor(0.01, min_dim_size_to_factor=8)
    shapes = {"w": (16, 12), "b": (12,)}
    n = 16 * 12 + 12
    x = deltas(K, n, seed=11)
    sl = make_slab(x, cuda, {k_: np.zeros(s, F32) for k_, s in shapes.items()})
    C, weights = clip_norm(x), weight_sets(K, 4)["float"]
    p0 = np.random.RandomState(9).uniform(-1, 1, n).astype(F32)
    pa, pb, pc = to_dev(p0, cuda), to_dev(p0, cuda), to_dev(p0, cuda)
    cm = sl.clipped_mean(weights, C)
    sb = opt.apply(cm.mean, opt.init(sl.unflatten(pb)), sl.unflatten(pb))[0]
    got = server.fused_clipped_mean_update(sl, weights, C, opt, pa, opt.init(sl.unflatten(pa)))
    assert got.state["count"] == sb["count"] == 1
    assert_bits(pa, host(pb), "slab route")
    assert not np.array_equal(host(pa), p0)
    same_diagnostics(got, cm, "adafactor slab")
    gotc = server.fused_tree_clipped_mean_update([(sl.client(k), w) for k, w in enumerate(weights)], C, opt,
                                                 sl.unflatten(pc), opt.init(sl.unflatten(pc)),
                                                 with_clipped_norms=False)
    assert gotc.state["count"] == 1 and gotc.clipped_norms is None
    assert_bits(pc, host(pb), "pytree route")


# ------------------------------------------------------------------------ 8. refusals
def test_python_refusals(cuda):
    K, P = 9, 1027
    opt = make_server(ADAM)
    x = deltas(K, P, seed=2)
    sl = make_slab(x, cuda)
    weights = weight_sets(K, K)["int"]
    p0, m0, v0 = probe_state(ADAM, P, seed=1)
    sentinel = torch.full((P,), float(SENTINEL), device=cuda)
    good_s = lambda: dev_state(m0, v0, 0, cuda)

    def call(**kw):
        return server.fused_clipped_mean_update(kw.get("slab", sl), kw.get("weights", weights), 1.0, kw.get("opt", opt),
                                                kw.get("params", sentinel), kw.get("state") or good_s(),
                                                mean_out=kw.get("mean_out"))

    with pytest.raises(TypeError):  # bf16 deltas
        call(slab=slab_mod.ClientDeltaSlab({"w": np.zeros(P, F32)}, K, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(ValueError, match="4096"):
        big = slab_mod.ClientDeltaSlab({"w": np.zeros(4, F32)}, 4097, device=cuda)
        server.fused_clipped_mean_update(big, [1] * 4097, 1.0, opt, torch.zeros(4, device=cuda),
                                         opt.init(torch.zeros(4, device=cuda)))
    with pytest.raises(ValueError):  # params of another dtype
        call(params=sentinel.double())
    with pytest.raises(ValueError):  # not contiguous
        call(params=torch.zeros(P, 2, device=cuda)[:, 0])
    with pytest.raises(ValueError):  # the wrong size
        call(params=torch.zeros(P + 1, device=cuda))
    with pytest.raises(ValueError):  # host params
        call(params=torch.zeros(P))
    with pytest.raises(ValueError):
        call(weights=weights[:-1])
    with pytest.raises(ValueError):
        call(mean_out=torch.zeros(P + 1, device=cuda))
    bad = good_s()
    del bad["v"]
    with pytest.raises(ValueError, match="'v'"):  # _require_state
        call(state=bad)
    bad = good_s()
    bad["m"] = bad["m"][:-1]
    with pytest.raises(ValueError):
        call(state=bad)
    # the pytree route
    xt, trees = tree_case(5, 30, cuda)
    pt0, mt0, vt0 = probe_state(ADAM, LEAF_P, seed=1)
    tparams = tree_of(np.full(LEAF_P, SENTINEL, F32), cuda)
    tstate = lambda: dev_state(mt0, vt0, 0, cuda, wrap=lambda t: tree_of(host(t), cuda))
    w5 = weight_sets(5, 5)["int"]
    with pytest.raises(ValueError, match="no clients to aggregate"):
        server.fused_tree_clipped_mean_update([], 1.0, opt, tparams, tstate())
    with pytest.raises(TypeError):
        server.fused_tree_clipped_mean_update([({k_: v_.bfloat16() for k_, v_ in t.items()}, 1.0) for t in trees],
                                              1.0, opt, tparams, tstate())
    with pytest.raises(TypeError):
        server.fused_tree_clipped_mean_update([({k_: v_.int() for k_, v_ in t.items()}, 1) for t in trees],
                                              1.0, opt, tparams, tstate())
    with pytest.raises(ValueError, match="4096"):
        one = {"w": torch.zeros(4, device=cuda)}
        server.fused_tree_clipped_mean_update([(one, 1)] * 4097, 1.0, opt, {"w": torch.zeros(4, device=cuda)},
                                              opt.init({"w": torch.zeros(4, device=cuda)}))
    with pytest.raises(ValueError):
        server.fused_tree_clipped_mean_update(list(zip(trees, w5)), 1.0, opt, dict(tparams, e=tparams["e"].double()),
                                              tstate())
    with pytest.raises(ValueError):
        server.fused_tree_clipped_mean_update(list(zip(trees, w5)), 1.0, opt, tparams, tstate(),
                                              mean_out=dict(tparams, f=tparams["f"][:-1]))
    bads = tstate()
    del bads["m"]
    with pytest.raises(ValueError, match="'m'"):
        server.fused_tree_clipped_mean_update(list(zip(trees, w5)), 1.0, opt, tparams, bads)
    # not capturable: the weights and the descriptor go up with every call
    g, st, ready = torch.cuda.CUDAGraph(), torch.cuda.Stream(), good_s()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g, stream=st):
                call(state=ready)
    torch.cuda.synchronize()
    assert (sentinel == float(SENTINEL)).all(), "a refused call wrote params"
    assert (flat_tree(tparams) == SENTINEL).all(), "a refused call wrote the params tree"


def test_raw_entry_refusals(cuda):
    """Every FJAGG_EINVAL / FJAGG_EUNSUPPORTED of the two entries on real buffers, with sentinel
    params unchanged; the same arguments, accepted, do step."""
    lib = _lib.load()
    EINVAL, EUNSUP = -1, kernels._EUNSUPPORTED
    K, P, L = 4, 64, 1
    x = torch.zeros(K, P, device=cuda)
    w, c = torch.ones(K, device=cuda), torch.full((K,), 0.5, device=cuda)
    state = torch.full((4, P), float(SENTINEL), device=cuda)  # params | m | v | mean
    l2 = torch.full((K,), float(SENTINEL), device=cuda)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    opt = make_server(ADAM)
    adam = opt.descriptor(1)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    st = np.array([state[i].data_ptr() for i in (1, 2, 3)], dtype=np.int64)
    w_words = np.zeros((K + 1) // 2, dtype=np.int64)
    w_words.view(np.float32)[:K] = 1.0
    blocks = np.array([0, P // 4], dtype=np.int64)
    image_h = np.concatenate([[x[k].data_ptr() for k in range(K)], [state[0].data_ptr()], [P], blocks, w_words, st])
    image = torch.from_numpy(image_h.astype(np.int64)).to(cuda)
    w_ptr = image.data_ptr() + 8 * (K * L + 2 * L + blocks.size)
    st_ptr = w_ptr + 8 * w_words.size

    def dense(in_dtype=_lib.F32, xp=x.data_ptr(), ld=P, Kv=K, Pv=P, wp=w.data_ptr(), cp=c.data_ptr(), desc=adam,
              pp=state[0].data_ptr(), mp=state[1].data_ptr(), vp=state[2].data_ptr(), l2p=l2.data_ptr(), flags=0,
              wsp=ws.data_ptr(), wsb=ws.numel()):
        return lib.fjagg_server_update_clip_dense(in_dtype, xp, ld, Kv, Pv, wp, cp, 1.0,
                                                  None if desc is None else ctypes.byref(desc), pp, mp, vp,
                                                  state[3].data_ptr(), l2p, flags, wsp, wsb, stream)

    def ptrs(in_dtype=_lib.F32, ip=image.data_ptr(), Lv=L, Kv=K, nblk=1, wp=w_ptr, cp=c.data_ptr(), desc=adam,
             sp=st_ptr, l2p=l2.data_ptr(), flags=0, wsp=ws.data_ptr(), wsb=ws.numel()):
        return lib.fjagg_server_update_clip_ptrs(in_dtype, ip, Lv, Kv, nblk, wp, cp, 1.0,
                                                 None if desc is None else ctypes.byref(desc), sp, l2p, flags, wsp,
                                                 wsb, stream)

    bad7, bad0 = opt.descriptor(1), opt.descriptor(1)
    bad7.kind, bad0.kind = 7, 0
    both = [("bf16", dict(in_dtype=_lib.BF16), EUNSUP), ("FJAGG_NARROW", dict(flags=_lib.NARROW), EUNSUP),
            ("FJAGG_HOST_TABLES", dict(flags=_lib.HOST_TABLES), EUNSUP),
            ("FJAGG_ZEROED_WS", dict(flags=_lib.ZEROED_WS), EUNSUP), ("a variant byte", dict(flags=12 << 8), EUNSUP),
            ("FJAGG_ACCUMULATE", dict(flags=_lib.ACCUMULATE), EUNSUP), ("FJAGG_SCALE", dict(flags=_lib.SCALE), EUNSUP),
            ("kind 7", dict(desc=bad7), EINVAL), ("kind 0", dict(desc=bad0), EINVAL),
            ("no descriptor", dict(desc=None), EINVAL), ("null w", dict(wp=None), EINVAL),
            ("null c", dict(cp=None), EINVAL), ("K = 0", dict(Kv=0), EINVAL), ("K > 4096 with norms", dict(Kv=4097), EUNSUP),
            ("norms without a workspace", dict(wsp=None), EINVAL), ("a small workspace", dict(wsb=8), EINVAL)]
    for what, kw, want in both:
        for name, entry in (("dense", dense), ("ptrs", ptrs)):
            rc = entry(**kw)
            assert rc == want, (name, what, rc, lib.fjagg_last_error())
    for what, rc, want in [
        ("FJAGG_UNALIGNED on the dense entry", dense(flags=_lib.UNALIGNED), EUNSUP),
        ("null x", dense(xp=None), EINVAL), ("null params", dense(pp=None), EINVAL),
        ("null m under adam", dense(mp=None), EINVAL), ("null v under adam", dense(vp=None), EINVAL),
        ("P = 0", dense(Pv=0), EINVAL), ("ld < P", dense(ld=P - 1), EINVAL),
        ("rows over 1 GiB", dense(Pv=(1 << 28) + 1, ld=(1 << 28) + 4), EUNSUP),
        ("null image", ptrs(ip=None), EINVAL), ("null state table", ptrs(sp=None), EINVAL),
        ("L = 0", ptrs(Lv=0), EINVAL), ("nblk = 0", ptrs(nblk=0), EINVAL),
    ]:
        assert rc == want, (what, rc, lib.fjagg_last_error())
    torch.cuda.synchronize()
    assert (state == float(SENTINEL)).all() and (l2 == float(SENTINEL)).all(), "a refused call wrote"
    # accepted: zero deltas, so every launch multiplies m by adam's b1 once more and leaves l2 = 0
    ublocks = kernels.ptrs_plan(_lib.F32, np.array([P], np.int64), True)  # element units over the whole launch
    uimage_h = np.concatenate([image_h[:K * L + 2 * L], ublocks, w_words, st]).astype(np.int64)
    uimage = torch.from_numpy(uimage_h).to(cuda)
    uw_ptr = uimage.data_ptr() + 8 * (K * L + 2 * L + ublocks.size)
    m = host(state[1]).copy()
    launches = [dense, lambda: dense(flags=_lib.NONTEMPORAL), lambda: dense(l2p=None, wsp=None, wsb=0), ptrs,
                lambda: ptrs(flags=_lib.NONTEMPORAL), lambda: ptrs(l2p=None, wsp=None, wsb=0),
                lambda: ptrs(flags=_lib.UNALIGNED, ip=uimage.data_ptr(), wp=uw_ptr, sp=uw_ptr + 8 * w_words.size,
                             nblk=ublocks.size // 2)]
    for i, launch in enumerate(launches):
        assert launch() == 0, (i, lib.fjagg_last_error())
        m = (F32(0.1) * F32(0) + F32(0.9) * m).astype(F32)
        assert_bits(state[1], m, f"accepted launch {i}")
    assert (l2 == 0).all() and (state[3] == 0).all()


# -------------------------------------------------------- 9. no host round trip
def test_no_host_synchronisation(cuda):
    K, P = 9, 1027
    opt = make_server(ADAM)
    x = deltas(K, P, seed=2)
    sl = make_slab(x, cuda)
    weights = weight_sets(K, K)["int"]
    C = clip_norm(x)
    p0, m0, v0 = probe_state(ADAM, P, seed=3)
    xt, trees = tree_case(5, 30, cuda)
    pt0, mt0, vt0 = probe_state(ADAM, LEAF_P, seed=4)
    Ct, wt = clip_norm(xt), weight_sets(5, 5)["int"]
    wrap = lambda t: tree_of(host(t), cuda)
    # first calls: library load, kernel attributes
    server.fused_clipped_mean_update(sl, weights, C, opt, to_dev(p0, cuda), dev_state(m0, v0, 0, cuda))
    server.fused_tree_clipped_mean_update(list(zip(trees, wt)), Ct, opt, tree_of(pt0, cuda),
                                          dev_state(mt0, vt0, 0, cuda, wrap=wrap))
    params, state = to_dev(p0, cuda), dev_state(m0, v0, 0, cuda)
    tparams, tstate = tree_of(pt0, cuda), dev_state(mt0, vt0, 0, cuda, wrap=wrap)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = server.fused_clipped_mean_update(sl, weights, C, opt, params, state)
        gott = server.fused_tree_clipped_mean_update(list(zip(trees, wt)), Ct, opt, tparams, tstate)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    c = restated_factors(got, x, C, "slab under sync debug mode")
    assert_bits(params, clipped_update_ref(x, weights, c, opt, p0, m0, v0, 0)[0], "slab under sync debug mode")
    ct = restated_factors(gott, xt, Ct, "pytree under sync debug mode")
    assert_bits(flat_tree(tparams), clipped_update_ref(xt, wt, ct, opt, pt0, mt0, vt0, 0)[0], "pytree")
