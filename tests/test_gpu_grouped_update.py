"""The grouped fold with each cluster's server step in its epilogue (k_dense_group_opt /
k_ptrs_group_opt through fjagg_server_update_group_dense / _ptrs, server.fused_grouped_mean_update
and server.fused_tree_grouped_mean_update; fedjax/algorithms/hyp_cluster.py:107-128) against the
numpy restatement in tests/grouped_update_ref.py, bit for bit, against the library's own
two-step route (grouped mean, then one fused step per cluster), and against the float64 rules.

Bit patterns are compared with every NaN mapped to one pattern (grouped_mean_ref.bits).
"""
import functools

import numpy as np
import pytest
import torch

from fedjax_amd import _lib, kernels, pytree, server, slab as slab_mod, tree_util as tu
from oracle import optax_rules_ref as rules
from tests import grouped_mean_ref as gref
from tests.grouped_update_ref import grouped_update_ref
from tests.test_server_rules_ref import HYPER, hyper_id, make_server, probe_state, rule_kwargs

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = F32(-1234.5)
ADAM, NESTEROV = HYPER[3], HYPER[2]
K, G, P = 13, 5, 1027
LEAVES = [("a", 1), ("b", 3), ("c", 64), ("d", 1027), ("e", 4100)]  # flatten order
CUTS = np.cumsum([0] + [n for _, n in LEAVES])
PT = int(CUTS[-1])


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return gref.bits(a).reshape(-1)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ the two rounds
@functools.lru_cache(maxsize=None)
def rounds():
    """Two rounds of (ids, weights). Round 1: two clients in no group, group 4 with a single
    member, group 3 empty (grouped_mean_ref.seeded_ids) and group 1 with a zero total, so the
    counts diverge: clusters 0, 2 and 4 step, 1 and 3 do not. Round 2: every cluster steps."""
    ids1 = gref.seeded_ids(K, G, seed=4)
    assert (ids1 == -1).sum() == 2 and (ids1 == 4).sum() == 1 and (ids1 == 3).sum() == 0
    rng = np.random.RandomState(3)
    w1 = [float(v) for v in rng.uniform(0.5, 3.0, K)]
    m1 = np.flatnonzero(ids1 == 1)
    assert m1.size >= 2 and (ids1 == 0).sum() >= 3 and (ids1 == 2).sum() >= 1
    for k in m1[:-1]:
        w1[k] = 1.0
    w1[m1[-1]] = -float(m1.size - 1)  # group 1: members, total exactly 0
    ids2 = ids1.copy()
    ids2[np.flatnonzero(ids1 == 0)[:2]] = 3  # the empty cluster gets members
    w2 = [int(v) for v in rng.randint(1, 50, K)]
    assert gref.group_totals(w1, ids1, G)[1] == 0 and all(W > 0 for W in gref.group_totals(w2, ids2, G))
    return (ids1, w1), (ids2, w2)


@functools.lru_cache(maxsize=None)
def deltas(n, seed):
    rs = np.random.RandomState(100 + seed)
    x = (rs.standard_normal((K, n)) * 0.02).astype(F32)
    x.setflags(write=False)
    return x


def initial(h, n):
    """Per cluster a chosen state (tests.test_server_rules_ref.probe_state), counts 0."""
    ps, ms, vs = zip(*[probe_state(h, n, seed=40 + g) for g in range(G)])
    return list(ps), list(ms), list(vs), [0] * G


@functools.lru_cache(maxsize=None)
def expected(hi, n):
    """The restatement's two rounds for rule HYPER[hi] on K x n deltas: computed once, shared, and
    never written to."""
    h = HYPER[hi]
    opt = make_server(h)
    p, m, v, c = initial(h, n)
    out = []
    for rnd, (ids, w) in enumerate(rounds()):
        r = grouped_update_ref(deltas(n, rnd), w, ids, G, opt, p, m, v, c)
        p, m, v, c = r["params"], r["m"], r["v"], r["counts"]
        out.append(r)
    assert out[0]["updated"] == [True, False, True, False, True] and out[1]["counts"] == [2, 1, 2, 1, 2]
    return out


def to_dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)


def make_states(opt, params, ms, vs, counts, cuda, wrap=lambda t: t):
    states = []
    for g in range(G):
        st = {"count": counts[g]}
        if ms[g] is not None:
            st["m"] = wrap(to_dev(ms[g], cuda))
        if vs[g] is not None:
            st["v"] = wrap(to_dev(vs[g], cuda))
        states.append(st)
    return states


def fill_slab(s, x):
    s.storage[:, : s.num_params].copy_(torch.from_numpy(np.array(x)))


# ------------------------------------------- 1. bitwise against the restatement, two rounds
def check_round(r, flat_p, flat_m, flat_v, mean_out, states, updated, what):
    """``flat_*(g)`` give cluster g's values as one float32 host vector (None if absent)."""
    assert updated == r["updated"], what
    assert [s["count"] for s in states] == r["counts"], what
    for g in range(G):
        assert same(flat_p(g), r["params"][g]), f"{what}: params of cluster {g}"
        for name, got, want in (("m", flat_m(g), r["m"][g]), ("v", flat_v(g), r["v"][g])):
            assert (got is None) == (want is None)
            if want is not None:
                assert same(got, want), f"{what}: {name} of cluster {g}"
        if r["means"][g] is None:
            assert (mean_out(g) == SENTINEL).all(), f"{what}: cluster {g} took no step but its mean row was written"
        else:
            assert same(mean_out(g), r["means"][g]), f"{what}: mean of cluster {g}"


@pytest.mark.parametrize("hi", range(len(HYPER)), ids=[hyper_id(h) for h in HYPER])
def test_dense_two_rounds_bitwise(cuda, hi):
    h = HYPER[hi]
    opt = make_server(h)
    want = expected(hi, P)
    s = slab_mod.ClientDeltaSlab({"w": np.zeros(P, F32)}, K, device=cuda)
    p0, m0, v0, c0 = initial(h, P)
    params = to_dev(np.stack(p0), cuda)
    states = make_states(opt, p0, m0, v0, c0, cuda)
    host = lambda t: t.detach().cpu().numpy()
    for rnd, (ids, w) in enumerate(rounds()):
        fill_slab(s, deltas(P, rnd))
        mean_out = torch.full((G, P), float(SENTINEL), device=cuda)
        before = states
        states, updated = server.fused_grouped_mean_update(s, w, ids, G, opt, params, states, mean_out=mean_out)
        assert all((a is b) != u for a, b, u in zip(states, before, updated))  # no step: the state itself
        mo = host(mean_out)
        check_round(want[rnd], lambda g: host(params[g]), lambda g: host(states[g]["m"]) if "m" in states[g] else None,
                    lambda g: host(states[g]["v"]) if "v" in states[g] else None, lambda g: mo[g], states, updated,
                    f"dense {hyper_id(h)} round {rnd + 1}")


def tree_of(vec, cuda, misalign=()):
    """{name: leaf} views of the host vector ``vec`` [PT] on the device; the leaves named in
    ``misalign`` sit 4 bytes off 16-byte alignment (a view at element 1 of their buffer)."""
    out = {}
    for i, (name, n) in enumerate(LEAVES):
        val = to_dev(vec[CUTS[i]:CUTS[i + 1]], cuda)
        if name in misalign:
            buf = torch.empty(n + 1, device=cuda)
            leaf = buf[1:]
            assert leaf.data_ptr() % 16 == 4
            leaf.copy_(val)
            val = leaf
        out[name] = val
    return out


def flat_tree(tree):
    return np.concatenate([tree[name].detach().cpu().numpy().reshape(-1) for name, _ in LEAVES])


def tree_clients(x, cuda):
    return [tree_of(x[k], cuda, misalign=("d",)) for k in range(K)]  # leaf d: element units


def tree_setup(h, opt, cuda):
    p0, m0, v0, c0 = initial(h, PT)
    # cluster 2's params leaf c is misaligned too: a leaf is unaligned when ANY pointer to it is
    params = [tree_of(p0[g], cuda, misalign=("c",) if g == 2 else ()) for g in range(G)]
    states = make_states(opt, p0, m0, v0, c0, cuda, wrap=lambda t: tree_of(t.cpu().numpy(), cuda))
    return params, states


@pytest.mark.parametrize("hi", range(len(HYPER)), ids=[hyper_id(h) for h in HYPER])
def test_pytree_two_rounds_bitwise(cuda, hi):
    h = HYPER[hi]
    opt = make_server(h)
    want = expected(hi, PT)
    assert pytree.flatten({n: 0 for n, _ in LEAVES})[1].num_leaves == len(LEAVES)
    params, states = tree_setup(h, opt, cuda)
    for rnd, (ids, w) in enumerate(rounds()):
        clients = tree_clients(deltas(PT, rnd), cuda)
        mean_out = [tree_of(np.full(PT, SENTINEL, F32), cuda) for _ in range(G)]
        states, updated = server.fused_tree_grouped_mean_update(list(zip(clients, w)), ids, opt, params, states,
                                                                mean_out=mean_out)
        check_round(want[rnd], lambda g: flat_tree(params[g]),
                    lambda g: flat_tree(states[g]["m"]) if "m" in states[g] else None,
                    lambda g: flat_tree(states[g]["v"]) if "v" in states[g] else None,
                    lambda g: flat_tree(mean_out[g]), states, updated, f"pytree {hyper_id(h)} round {rnd + 1}")


# ----------------------- 2. bitwise against the library's two-step route (the parent's route)
def two_step(means, opt, params_trees, states):
    """The route before this kernel: for each cluster with a mean, the fused step on a one-client
    mean of weight 1 (the identity)."""
    new = list(states)
    for g, mean in enumerate(means):
        if mean is not None:
            new[g] = server.fused_tree_mean_update([(mean, 1.0)], opt, params_trees[g], states[g])
    return new


@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_dense_equals_grouped_mean_then_fused_steps(cuda, h):
    opt = make_server(h)
    s = slab_mod.ClientDeltaSlab({"u": np.zeros(27, F32), "w": np.zeros(P - 27, F32)}, K, device=cuda)
    p0, m0, v0, c0 = initial(h, P)
    pa, pb = to_dev(np.stack(p0), cuda), to_dev(np.stack(p0), cuda)
    sa = make_states(opt, p0, m0, v0, c0, cuda)
    sb = make_states(opt, p0, m0, v0, c0, cuda, wrap=s.unflatten)
    for rnd, (ids, w) in enumerate(rounds()):
        fill_slab(s, deltas(P, rnd))
        sa, updated = server.fused_grouped_mean_update(s, w, ids, G, opt, pa, sa)
        means = s.grouped_mean(w, ids, G)
        assert updated == [mean is not None for mean in means]
        sb = two_step(means, opt, [s.unflatten(pb[g]) for g in range(G)], sb)
        assert same(pa, pb), rnd
        for g in range(G):
            assert sa[g]["count"] == sb[g]["count"]
            for key in ("m", "v"):
                if key in sa[g]:
                    got = sa[g][key]
                    wantv = torch.cat([t.reshape(-1) for t in pytree.leaves_of(sb[g][key])])
                    assert same(got, wantv), (rnd, g, key)


@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_pytree_equals_grouped_mean_then_fused_steps(cuda, h):
    opt = make_server(h)
    pa, sa = tree_setup(h, opt, cuda)
    pb, sb = tree_setup(h, opt, cuda)
    for rnd, (ids, w) in enumerate(rounds()):
        pairs = list(zip(tree_clients(deltas(PT, rnd), cuda), w))
        sa, updated = server.fused_tree_grouped_mean_update(pairs, ids, opt, pa, sa)
        means = tu.tree_grouped_mean(pairs, ids, G)
        assert updated == [mean is not None for mean in means]
        sb = two_step(means, opt, pb, sb)
        for g in range(G):
            assert sa[g]["count"] == sb[g]["count"]
            assert same(flat_tree(pa[g]), flat_tree(pb[g])), (rnd, g)
            for key in ("m", "v"):
                if key in sa[g]:
                    assert same(flat_tree(sa[g][key]), flat_tree(sb[g][key])), (rnd, g, key)


# --------------------------------------------------------------- 3. every dense shape
def _dense_launch(xd, w, ids, Gn, opt, counts, p, m, v, nt):
    """One raw launch of kernels.grouped_update_dense on clones of p, m, v [Gn, n]."""
    totals = gref.group_totals([float(t) for t in w], ids, Gn)
    scales = np.array([F32(1.0 / W) for W in totals], F32)
    tables = kernels.GroupTables(w, ids, Gn, scales)
    p, m, v = p.clone(), m.clone(), v.clone()
    mean = torch.full_like(p, float(SENTINEL))
    addrs = np.array([[t[g].data_ptr() for t in (p, m, v, mean)] for g in range(Gn)], dtype=np.int64)
    up = kernels.GroupUpdateTables(tables, [opt.descriptor(c + 1) for c in counts], addrs.reshape(1, -1))
    up.upload(xd.device)
    shape = kernels.grouped_update_dense_shape(xd, tables)
    kernels.grouped_update_dense(xd, up, 0, nontemporal=nt)
    return shape, p, m, v, mean


# the sizes of tests/test_gpu_grouped_mean.py's regime test (E=4 x U=4; E=8 x U=4 burst: 128 tiles x
# 3 groups < 2 x 256 CUs; E=8 x U=4 interleaved) and a small one (E=1 x U=8 over 16-byte units)
@pytest.mark.parametrize("n,shape", [(20_483, 2), (600_003, 5), (1_048_579, 12), (1_500_003, 12)])
def test_dense_every_shape(cuda, n, shape):
    Kn, Gn = 40, 3
    ld = (n + 3) // 4 * 4 + 4
    gen = torch.Generator(device=cuda).manual_seed(n)
    xd = (torch.randn(Kn, ld, device=cuda, generator=gen) * 0.02)[:, :n]
    odd = torch.empty(Kn, n + 1 + (n % 2), device=cuda)[:, :n]  # an odd row stride: element units
    odd.copy_(xd)
    ids = gref.seeded_ids(Kn, Gn, seed=n, force_edges=False)
    assert np.bincount(ids, minlength=Gn).min() >= 8
    w = np.random.RandomState(n).uniform(0.1, 3.0, Kn).astype(F32)
    opt = make_server(ADAM)
    counts = [0, 1, 6]
    ps, ms, vs = zip(*[probe_state(ADAM, n, seed=g) for g in range(Gn)])
    p, m, v = (to_dev(np.stack(a), cuda) for a in (ps, ms, vs))
    got = _dense_launch(xd, w, ids, Gn, opt, counts, p, m, v, nt=True)
    ref = _dense_launch(odd, w, ids, Gn, opt, counts, p, m, v, nt=False)
    assert got[0] == shape and ref[0] == 0
    for a, b, what in zip(got[1:], ref[1:], ("params", "m", "v", "mean")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: the shapes disagree"
    # and sampled columns (the last 16 included) against the restatement
    cols = np.unique(np.concatenate([np.random.RandomState(n).randint(0, n, 2048), np.arange(n - 16, n)]))
    cd = torch.from_numpy(cols).to(cuda)
    r = grouped_update_ref(xd[:, cd].cpu().numpy(), [float(t) for t in w], ids, Gn, opt,
                           [a[cols] for a in ps], [a[cols] for a in ms], [a[cols] for a in vs], counts)
    for g in range(Gn):
        for a, key in zip(got[1:], ("params", "m", "v", "means")):
            assert same(a[g, cd], r[key][g]), (g, key)


# ------------------------------------------------------------------ 4. special values
def test_special_values_stay_in_their_group(cuda):
    opt = make_server(ADAM)
    ids, w = rounds()[1]  # every cluster has members and a positive total
    ids, w = ids.copy(), [float(t) for t in w]
    free = np.flatnonzero(ids == -1)
    a_member, b_member = np.flatnonzero(ids == 0)[0], np.flatnonzero(ids == 2)[0]
    x = np.array(deltas(P, 5))
    s = slab_mod.ClientDeltaSlab({"w": np.zeros(P, F32)}, K, device=cuda)
    p0, m0, v0, c0 = initial(ADAM, P)
    c0 = [0, 1, 2, 0, 1]

    def run(xx, ww):
        fill_slab(s, xx)
        params = to_dev(np.stack(p0), cuda)
        states = make_states(opt, p0, m0, v0, c0, cuda)
        mean_out = torch.full((G, P), float(SENTINEL), device=cuda)
        states, updated = server.fused_grouped_mean_update(s, ww, ids, G, opt, params, states, mean_out=mean_out)
        return params.cpu().numpy(), states, updated, mean_out.cpu().numpy()

    clean = run(x, w)
    y, wy = x.copy(), list(w)
    y[a_member, 0::4], y[a_member, 1::4], y[a_member, 2::4] = np.inf, np.nan, -0.0  # cluster 0's member
    y[free[0], :] = np.nan  # a client in no group
    y[free[1], ::2] = -np.inf
    wy[b_member] = float("nan")  # cluster 2's total is NaN: no mean, no step
    got = run(y, wy)
    r = grouped_update_ref(y, wy, ids, G, opt, p0, m0, v0, c0)
    assert got[2] == r["updated"] == [True, True, False, True, True]
    for g in range(G):
        assert same(got[0][g], r["params"][g]), g
        assert got[1][g]["count"] == r["counts"][g]
        assert same(got[1][g]["m"], r["m"][g]) and same(got[1][g]["v"], r["v"][g]), g
        if g in (1, 3, 4):  # never saw the special clients' values
            assert same(got[0][g], clean[0][g]) and same(got[3][g], clean[3][g]), g
            assert np.isfinite(got[0][g]).all()
    assert np.isnan(got[0][0]).any() and (got[3][2] == SENTINEL).all()
    assert same(got[0][2], p0[2])  # the NaN-total cluster kept its params


# ------------------------------------------------------------------ 5. the float64 rules
@pytest.mark.parametrize("route", ["dense", "pytree"])
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_one_round_against_float64_rules(cuda, h, route):
    """One round per rule held to oracle/optax_rules_ref.step under that module's own bound; the
    clusters step at counts 1, 2, 7, 1000 and 100000 in the same launch."""
    opt = make_server(h)
    n = P if route == "dense" else PT
    ids, w = rounds()[1]
    x = deltas(n, 7)
    counts = [0, 1, 6, 999, 99999]
    ps, ms, vs = zip(*[probe_state(h, n, seed=60 + g) for g in range(G)])
    means = gref.grouped_mean_ref(x, w, ids, G)
    if route == "dense":
        s = slab_mod.ClientDeltaSlab({"w": np.zeros(n, F32)}, K, device=cuda)
        fill_slab(s, x)
        params = to_dev(np.stack(ps), cuda)
        states = make_states(opt, ps, ms, vs, counts, cuda)
        states, _ = server.fused_grouped_mean_update(s, w, ids, G, opt, params, states)
        flat = lambda t: t.detach().cpu().numpy()
        got_p = [flat(params[g]) for g in range(G)]
    else:
        params = [tree_of(ps[g], cuda) for g in range(G)]
        states = make_states(opt, ps, ms, vs, counts, cuda, wrap=lambda t: tree_of(t.cpu().numpy(), cuda))
        states, _ = server.fused_tree_grouped_mean_update(list(zip(tree_clients(x, cuda), w)), ids, opt, params,
                                                          states)
        flat = flat_tree
        got_p = [flat(params[g]) for g in range(G)]
    for g in range(G):
        t = counts[g] + 1
        assert states[g]["count"] == t
        want = rules.step(h["kind"], t, means[g], ps[g], ms[g], vs[g], **rule_kwargs(h))
        got = {"p": got_p[g]}
        got.update({k: flat(states[g][k]) for k in ("m", "v") if k in want})
        for key, (r, bound) in want.items():
            ok = rules.within(got[key], r, bound)
            worst = float(np.max(np.abs(got[key].astype(np.float64) - r) / np.maximum(bound, 1e-300)))
            print(f"{route} {hyper_id(h)} cluster {g} t={t} {key}: max |gpu - ref| / bound = {worst:.3g}")
            assert ok.all(), (route, g, key, int((~ok).sum()), worst)


# ------------------------------------------------------------------------ 6. refusals
def test_python_refusals(cuda):
    opt = make_server(ADAM)
    s = slab_mod.ClientDeltaSlab({"w": np.zeros(P, F32)}, K, device=cuda)
    ids, w = rounds()[1]
    p0, m0, v0, c0 = initial(ADAM, P)
    good_p = lambda: to_dev(np.stack(p0), cuda)
    good_s = lambda: make_states(opt, p0, m0, v0, c0, cuda)

    def call(**kw):
        params = kw["params"] if "params" in kw else good_p()
        states = kw["states"] if "states" in kw else good_s()
        return server.fused_grouped_mean_update(kw.get("slab", s), w, kw.get("ids", ids), G, opt, params, states,
                                                mean_out=kw.get("mean_out"))

    sentinel = torch.full((G, P), float(SENTINEL), device=cuda)
    with pytest.raises(TypeError):  # bf16 deltas
        call(slab=slab_mod.ClientDeltaSlab({"w": np.zeros(P, F32)}, K, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(ValueError):  # params of another dtype
        call(params=good_p().double())
    with pytest.raises(ValueError):  # not contiguous
        call(params=torch.zeros(P, G, device=cuda).t())
    with pytest.raises(ValueError):  # the wrong shape
        call(params=torch.zeros(G, P + 1, device=cuda))
    with pytest.raises(ValueError):  # host params
        call(params=torch.zeros(G, P))
    with pytest.raises(ValueError):  # too few states
        call(states=good_s()[:-1])
    bad = good_s()
    del bad[0]["v"]
    with pytest.raises(ValueError, match="'v'"):  # _require_state, per updated cluster
        call(states=bad, params=sentinel)
    bad = good_s()
    bad[4]["m"] = bad[4]["m"][:-1]
    with pytest.raises(ValueError):
        call(states=bad, params=sentinel)
    with pytest.raises(ValueError):
        call(ids=[0] * (K - 1))
    with pytest.raises(ValueError):
        call(ids=[G] * K)
    with pytest.raises(ValueError):
        call(mean_out=torch.zeros(G, P + 1, device=cuda), params=sentinel)
    assert (sentinel == float(SENTINEL)).all(), "a refused call wrote params"
    # the pytree route
    params, states = tree_setup(ADAM, opt, cuda)
    clients = tree_clients(deltas(PT, 0), cuda)
    with pytest.raises(TypeError):
        server.fused_tree_grouped_mean_update([({k_: v_.bfloat16() for k_, v_ in c.items()}, 1.0) for c in clients],
                                              ids, opt, params, states)
    with pytest.raises(TypeError):
        server.fused_tree_grouped_mean_update([({k_: v_.int() for k_, v_ in c.items()}, 1) for c in clients],
                                              ids, opt, params, states)
    with pytest.raises(ValueError):
        server.fused_tree_grouped_mean_update(list(zip(clients, w)), ids, opt, params[:-1], states)
    badp = list(params)
    badp[1] = dict(badp[1], e=badp[1]["e"].double())
    with pytest.raises(ValueError):
        server.fused_tree_grouped_mean_update(list(zip(clients, w)), ids, opt, badp, states)
    bads = [dict(st) for st in states]
    del bads[3]["m"]
    with pytest.raises(ValueError, match="'m'"):
        server.fused_tree_grouped_mean_update(list(zip(clients, w)), ids, opt, params, bads)
    # not capturable: the tables go up with every call
    g, st, ready = torch.cuda.CUDAGraph(), torch.cuda.Stream(), good_s()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with pytest.raises(RuntimeError, match="not capturable"):
            with torch.cuda.graph(g, stream=st):
                call(params=sentinel, states=ready)
    torch.cuda.synchronize()
    assert (sentinel == float(SENTINEL)).all()


def test_raw_entry_refusals(cuda):
    """Every FJAGG_EINVAL / FJAGG_EUNSUPPORTED of the two entries, with sentinel params unchanged."""
    lib = _lib.load()
    EINVAL, EUNSUP = -1, kernels._EUNSUPPORTED
    n, Kn, Gn, L = 64, 4, 2, 1
    x = torch.zeros(Kn, n, device=cuda)
    ids = np.array([0, 1, 0, -1])
    w = np.ones(Kn, F32)
    opt = make_server(ADAM)
    state = torch.full((4, Gn, n), float(SENTINEL), device=cuda)  # params | m | v | mean
    addrs = np.array([[state[i, g].data_ptr() for i in range(4)] for g in range(Gn)], dtype=np.int64)

    def dense(flags=_lib.SCALE, dtype=_lib.F32, descs=None, addr=addrs, seg=None, order=None, Gv=Gn):
        t = kernels.GroupTables(w, ids, Gn, np.ones(Gn, F32))
        up = kernels.GroupUpdateTables(t, descs or [opt.descriptor(1)] * Gn, addr.reshape(1, -1)).upload(cuda)
        order_p, seg_p, gorder_p, wperm_p, gscale_p = t.ptrs()
        seg_h = t.seg if seg is None else np.array(seg, np.int32)
        order_h = t.order if order is None else np.array(order, np.int32)
        host = np.ascontiguousarray(addr)
        return lib.fjagg_server_update_group_dense(
            dtype, x.data_ptr(), n, Kn, n, t.M, Gv, order_p, seg_p, wperm_p, gscale_p, gorder_p, order_h.ctypes.data,
            seg_h.ctypes.data, up.opts_ptr(), up.addrs_ptr(0), up.opts.ctypes.data, host.ctypes.data, flags, None)

    def zeroed(g, i):
        a = addrs.copy()
        a[g, i] = 0
        return a

    bad_kind = opt.descriptor(1)
    bad_kind.kind = 7
    zero_kind = opt.descriptor(1)
    zero_kind.kind = 0
    for what, rc, want in [
        ("no FJAGG_SCALE", dense(flags=0), EINVAL),
        ("FJAGG_ACCUMULATE", dense(flags=_lib.SCALE | _lib.ACCUMULATE), EUNSUP),
        ("FJAGG_NARROW", dense(flags=_lib.SCALE | _lib.NARROW), EUNSUP),
        ("FJAGG_HOST_TABLES", dense(flags=_lib.SCALE | _lib.HOST_TABLES), EUNSUP),
        ("FJAGG_UNALIGNED on the dense entry", dense(flags=_lib.SCALE | _lib.UNALIGNED), EUNSUP),
        ("bf16", dense(dtype=_lib.BF16), EUNSUP),
        ("kind 7", dense(descs=[opt.descriptor(1), bad_kind]), EINVAL),
        ("kind 0", dense(descs=[zero_kind, opt.descriptor(1)]), EINVAL),
        ("params 0", dense(addr=zeroed(1, 0)), EINVAL),
        ("m 0 under adam", dense(addr=zeroed(0, 1)), EINVAL),
        ("v 0 under adam", dense(addr=zeroed(1, 2)), EINVAL),
        ("seg[0] != 0", dense(seg=[1, 2, 3]), EINVAL),
        ("seg not monotone", dense(seg=[0, 3, 2]), EINVAL),
        ("seg[G] != M", dense(seg=[0, 2, 4]), EINVAL),
        ("order outside [0, K)", dense(order=[0, 2, 4]), EINVAL),
        ("G = 0", dense(Gv=0), EINVAL),
    ]:
        assert rc == want, (what, rc, lib.fjagg_last_error())
    # the pytree entry: the same image as the Python route builds, by hand
    t = kernels.GroupTables(w, ids, Gn, np.ones(Gn, F32))
    leaf_n = np.array([n], np.int64)
    in_ptrs = np.array([[x[k].data_ptr()] for k in t.order], dtype=np.int64)
    out_ptrs = addrs[:, :1].copy()
    st = np.ascontiguousarray(addrs[:, 1:].reshape(Gn, 3, L))
    blocks, _ = tu._leaf_plan(_lib.F32, leaf_n, in_ptrs, out_ptrs, st.reshape(3 * Gn, L), cuda)

    def ptrs(flags=_lib.SCALE, dtype=_lib.F32, descs=None, params_h=out_ptrs, st_h=st, seg=None, nblk=None,
             blocks=blocks):
        opts = kernels.pack_server_opts(descs or [opt.descriptor(1)] * Gn)
        t32 = np.concatenate([t.host[t.M:], opts])
        words = np.zeros((t32.size + 1) // 2, dtype=np.int64)
        words.view(np.int32)[: t32.size] = t32
        image = np.concatenate([in_ptrs.ravel(), out_ptrs.ravel(), leaf_n, blocks, words, st.ravel()])
        dev = _lib.upload(torch.from_numpy(image), cuda)
        seg_p = dev.data_ptr() + 8 * (in_ptrs.size + out_ptrs.size + L + blocks.size)
        seg_h = t.seg if seg is None else np.array(seg, np.int32)
        params_h, st_h = np.ascontiguousarray(params_h), np.ascontiguousarray(st_h)
        return lib.fjagg_server_update_group_ptrs(
            dtype, dev.data_ptr(), L, Kn, t.M, Gn, blocks.size // 2 if nblk is None else nblk, seg_p,
            seg_p + 4 * (2 * Gn + 1), seg_p + 4 * (2 * Gn + 1 + t.M), seg_p + 4 * (Gn + 1), seg_h.ctypes.data,
            seg_p + 4 * (3 * Gn + 1 + t.M), seg_p + 8 * words.size, opts.ctypes.data, st_h.ctypes.data,
            params_h.ctypes.data, leaf_n.ctypes.data, flags, None)

    zp = out_ptrs.copy()
    zp[0, 0] = 0
    zm, zv = st.copy(), st.copy()
    zm[1, 0, 0] = 0
    zv[0, 1, 0] = 0
    for what, rc, want in [
        ("no FJAGG_SCALE", ptrs(flags=0), EINVAL),
        ("FJAGG_ACCUMULATE", ptrs(flags=_lib.SCALE | _lib.ACCUMULATE), EUNSUP),
        ("FJAGG_NARROW", ptrs(flags=_lib.SCALE | _lib.NARROW), EUNSUP),
        ("bf16", ptrs(dtype=_lib.BF16), EUNSUP),
        ("kind 7", ptrs(descs=[bad_kind, opt.descriptor(1)]), EINVAL),
        ("params 0", ptrs(params_h=zp), EINVAL),
        ("m 0 under adam", ptrs(st_h=zm), EINVAL),
        ("v 0 under adam", ptrs(st_h=zv), EINVAL),
        ("seg[G] != M", ptrs(seg=[0, 1, 2]), EINVAL),
        ("nblk 0", ptrs(nblk=0), EINVAL),
    ]:
        assert rc == want, (what, rc, lib.fjagg_last_error())
    torch.cuda.synchronize()
    assert (state == float(SENTINEL)).all(), "a refused call wrote through the state addresses"
    # and the same arguments, accepted, do step (the refusals above were not vacuous): zero deltas,
    # so every accepted launch multiplies m by adam's b1 once more, in both clusters
    m_of = lambda: state[1].cpu().numpy().copy()
    m = m_of()
    launches = [dense, lambda: dense(flags=_lib.SCALE | _lib.NONTEMPORAL), ptrs,
                lambda: ptrs(flags=_lib.SCALE | _lib.NONTEMPORAL),
                # single-element units over the whole launch: a plan made for them
                lambda: ptrs(flags=_lib.SCALE | _lib.UNALIGNED, blocks=kernels.ptrs_plan(_lib.F32, leaf_n, True)),
                lambda: ptrs(flags=_lib.SCALE | _lib.UNALIGNED | _lib.NONTEMPORAL,
                             blocks=kernels.ptrs_plan(_lib.F32, leaf_n, True))]
    for i, launch in enumerate(launches):
        assert launch() == 0, (i, lib.fjagg_last_error())
        m = (F32(0.1) * F32(0) + F32(0.9) * m).astype(F32)
        assert same(m_of(), m), f"accepted launch {i}"


# ------------------------------------------------------- 7. frozen leaves and adafactor
def test_frozen_leaves_both_routes(cuda):
    """ignore_grads_haiku: the frozen leaves' params and state are untouched in every cluster and
    the trainable leaves are bitwise those of test 1 (the same rounds, states and deltas)."""
    hi = 3
    h = HYPER[hi]
    opt = server.ignore_grads_haiku(make_server(h), [("m1", "b"), ("m2", "d")])
    want = expected(hi, PT)
    nest = lambda tr: {"m0": {"a": tr["a"]}, "m1": {"b": tr["b"], "c": tr["c"]}, "m2": {"d": tr["d"], "e": tr["e"]}}
    unnest = lambda tr: {k_: v_ for sub in tr.values() for k_, v_ in sub.items()}
    frozen = np.zeros(PT, dtype=bool)
    for i in (1, 3):
        frozen[CUTS[i]:CUTS[i + 1]] = True
    p0, m0, v0, c0 = initial(h, PT)
    # pytree route
    params, states = tree_setup(h, opt, cuda)
    params = [nest(p) for p in params]
    states = [dict(st, m=nest(st["m"]), v=nest(st["v"])) for st in states]
    # slab route: the same template, flat
    s = slab_mod.ClientDeltaSlab(nest({n_: np.zeros(k_, F32) for n_, k_ in LEAVES}), K, device=cuda)
    assert [int(v_) for v_ in s.sizes] == [n_ for _, n_ in LEAVES]
    dparams = to_dev(np.stack(p0), cuda)
    dstates = make_states(opt, p0, m0, v0, c0, cuda)
    for rnd, (ids, w) in enumerate(rounds()):
        x = deltas(PT, rnd)
        mean_out = [nest(tree_of(np.full(PT, SENTINEL, F32), cuda)) for _ in range(G)]
        states, updated = server.fused_tree_grouped_mean_update(
            [(nest(c), wk) for c, wk in zip(tree_clients(x, cuda), w)], ids, opt, params, states, mean_out=mean_out)
        fill_slab(s, x)
        dmean = torch.full((G, PT), float(SENTINEL), device=cuda)
        dstates, dupdated = server.fused_grouped_mean_update(s, w, ids, G, opt, dparams, dstates, mean_out=dmean)
        r = want[rnd]
        assert updated == dupdated == r["updated"]
        for g in range(G):
            assert states[g]["count"] == dstates[g]["count"] == r["counts"][g]  # the count still advances
            for what, tree_v, flat_v, ref_v, init_v in (
                    ("params", flat_tree(unnest(params[g])), dparams[g].cpu().numpy(), r["params"][g], p0[g]),
                    ("m", flat_tree(unnest(states[g]["m"])), dstates[g]["m"].cpu().numpy(), r["m"][g], m0[g]),
                    ("v", flat_tree(unnest(states[g]["v"])), dstates[g]["v"].cpu().numpy(), r["v"][g], v0[g])):
                for route, got in (("pytree", tree_v), ("slab", flat_v)):
                    assert same(got[frozen], init_v[frozen]), f"{route} {what} of cluster {g}: a frozen leaf moved"
                    assert same(got[~frozen], ref_v[~frozen]), f"{route} {what} of cluster {g} round {rnd + 1}"
            if r["means"][g] is not None:  # the mean of frozen leaves too
                assert same(flat_tree(unnest(mean_out[g])), r["means"][g]) and same(dmean[g], r["means"][g]), g
            else:
                assert (dmean[g] == float(SENTINEL)).all() and (flat_tree(unnest(mean_out[g])) == SENTINEL).all()


def test_adafactor_falls_back_to_grouped_mean_then_apply(cuda):
    opt = server.adafactor(0.01, min_dim_size_to_factor=8)
    shapes = {"w": (16, 12), "b": (12,)}
    n = 16 * 12 + 12
    ids, w = rounds()[0]
    rs = np.random.RandomState(9)
    x = (rs.standard_normal((K, n)) * 0.02).astype(F32)
    p0 = (rs.uniform(-1, 1, (G, n))).astype(F32)
    s = slab_mod.ClientDeltaSlab({k_: np.zeros(v_, F32) for k_, v_ in shapes.items()}, K, device=cuda)
    fill_slab(s, x)
    pa, pb = to_dev(p0, cuda), to_dev(p0, cuda)
    sa = [opt.init(s.unflatten(pa[g])) for g in range(G)]
    sb = [opt.init(s.unflatten(pb[g])) for g in range(G)]
    new, updated = server.fused_grouped_mean_update(s, w, ids, G, opt, pa, sa)
    means = s.grouped_mean(w, ids, G)
    assert updated == [mean is not None for mean in means] == [True, False, True, False, True]
    for g, mean in enumerate(means):
        if mean is not None:
            sb[g] = opt.apply(mean, sb[g], s.unflatten(pb[g]))[0]
        assert new[g]["count"] == sb[g]["count"] == int(updated[g])
        assert (new[g] is sa[g]) == (not updated[g])
    assert same(pa, pb) and same(pa[1], p0[1]) and not same(pa[0], p0[0])
    # the pytree route
    trees = [s.client(k) for k in range(K)]
    pc = to_dev(p0, cuda)
    sc = [opt.init(s.unflatten(pc[g])) for g in range(G)]
    newc, updc = server.fused_tree_grouped_mean_update(list(zip(trees, w)), ids, opt,
                                                       [s.unflatten(pc[g]) for g in range(G)], sc)
    assert updc == updated and [st["count"] for st in newc] == [st["count"] for st in new]
    assert same(pc, pb)
