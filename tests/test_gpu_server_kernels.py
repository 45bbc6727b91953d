"""The fused server step's kernels (k_dense_opt / k_ptrs_opt, fedjax_amd/csrc/fjagg.hip)
against expectations that do not come from the code under test.

* Formula probes: one step from a chosen state at counts 1 .. 100000, both paths, against
  the float64 reference of the rules (oracle/optax_rules_ref.py) under its own bound. The
  reference sees only the public hyperparameters and the oracle's mean.
* Every epilogue instantiation, bitwise: the oracle mean (oracle/fold_ref.c), the numpy
  restatement ``_np_server_step`` and constants computed in tests/test_server_rules_ref.py
  from the hyperparameters (never ``descriptor()``). Each case's id names the kernel
  instantiation it reaches: ``V`` elements per unit, ``E`` units per lane, ``U`` clients
  in flight, ``NT`` nontemporal loads.
* Special values (NaN, infinities, signed zeros, subnormals, overflowing and underflowing
  squares) through the epilogue of both paths.
"""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import server
from oracle import optax_rules_ref as rules
from oracle import tree_util_ref as ref
from tests.coracle import bf16_to_f32
from tests.test_gpu_parity import _np_server_step, bits, host
from tests.test_server_rules_ref import (COUNTS, HYPER, consts, hyper_id, make_server, needs, probe_state,
                                         rule_kwargs)

pytestmark = pytest.mark.gpu
f32 = np.float32
ADAM, NESTEROV = HYPER[3], HYPER[2]


def _weights(K, seed):
    return [int(w) for w in ref.fedavg_weights(K, seed=seed + 100)]


_MEANS = {}


def oracle_rows(coracle, K, P, bf16, seed, amp=0.01):
    """The synthetic client rows as float32 on the host (bf16: the rounded values, widened)."""
    if bf16:
        return np.ascontiguousarray(bf16_to_f32(coracle.synth_bf16(K, P, seed=seed, amp=amp)))
    return coracle.synth_f32(K, P, seed=seed, amp=amp)


def oracle_mean(coracle, K, P, bf16, seed, amp=0.01):
    """The oracle's float32 fold of the synthetic slab (seed) with the weights of the same
    seed, times f32(1 / W). Computed once per shape and shared; callers do not write to it."""
    key = (K, P, bf16, seed, amp)
    if key not in _MEANS:
        wi = _weights(K, seed)
        g = coracle.wsum_f32(oracle_rows(coracle, K, P, bf16, seed, amp), f32(wi), scale=ref.mean_scale(wi))
        g.setflags(write=False)
        _MEANS[key] = g
    return _MEANS[key]


def same(a, b):
    """Equal bits (the sign of zero included), or NaN on both sides."""
    a, b = np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def _set_state(state, m, v, count):
    state["count"] = count
    for key, val in (("m", m), ("v", v)):
        if key in state:
            assert val is not None
            state[key].copy_(torch.from_numpy(val))
    return state


def _np_step(h, t, g, p, m, v):
    """_np_server_step with this suite's own constants; absent moments stay None."""
    with np.errstate(all="ignore"):
        p2, m2, v2 = _np_server_step(make_server(h), consts(h, t), g, p, m, v)
    has_m, has_v = needs(h)
    return p2, (m2 if has_m else None), (v2 if has_v else None)


# ------------------------------------------------------------------ formula probes
PROBE_LEAVES = {"a": (7,), "b": (1009,), "c": (3, 5)}
PROBE_K, PROBE_P = 3, 1031


def _probe_expect(coracle, h, t, zero_params):
    g = oracle_mean(coracle, PROBE_K, PROBE_P, False, seed=300 + t % 97, amp=0.02)
    p, m, v = probe_state(h, PROBE_P, seed=t % 97, zero_params=zero_params)
    return g, p, m, v, rules.step(h["kind"], t, g, p, m, v, **rule_kwargs(h))


def _check_bound(got, want, what):
    for key, (r, bound) in want.items():
        ok = rules.within(got[key], r, bound)
        worst = float(np.max(np.abs(got[key].astype(np.float64) - r) / np.maximum(bound, 1e-300)))
        print(f"{what} {key}: max |gpu - ref| / bound = {worst:.3g}")
        assert ok.all(), (what, key, int((~ok).sum()), worst)


@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_probe_dense_against_float64_rules(h, t, cuda, coracle):
    """fused_mean_update (k_dense_opt<f32, V=4, E=1, U=8>), one step with incremented
    count t: p', m', v' within twice the reference's bound; mean_out bitwise the oracle's."""
    opt = make_server(h)
    slab = fedjax_amd.ClientDeltaSlab({k: np.zeros(s, f32) for k, s in PROBE_LEAVES.items()}, PROBE_K, device=cuda)
    slab.fill_synthetic(seed=300 + t % 97, amp=0.02)
    wi = _weights(PROBE_K, 300 + t % 97)
    for zero_params in (True, False):
        g, p, m, v, want = _probe_expect(coracle, h, t, zero_params)
        params = torch.from_numpy(p.copy()).to(cuda)
        state = _set_state(opt.init(params), m, v, t - 1)
        mean_out = torch.empty(PROBE_P, device=cuda)
        state = server.fused_mean_update(slab, wi, opt, params, state, mean_out=mean_out)
        assert state["count"] == t
        assert np.array_equal(bits(host(mean_out)), bits(g))
        got = {"p": host(params)}
        got.update({k: host(state[k]) for k in ("m", "v") if k in want})
        _check_bound(got, want, f"dense {hyper_id(h)} t={t} p0={zero_params}")


@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_probe_pytree_against_float64_rules(h, t, cuda, coracle):
    """fused_tree_mean_update (k_ptrs_opt<f32, V=4>; leaves of 7, 1009 and (3, 5)): the
    same probes, leaf by leaf."""
    opt = make_server(h)
    seed = 300 + t % 97
    x = torch.from_numpy(coracle.synth_f32(PROBE_K, PROBE_P, seed=seed, amp=0.02)).to(cuda)
    wi = _weights(PROBE_K, seed)
    cuts = np.cumsum([0] + [int(np.prod(s)) for s in PROBE_LEAVES.values()])
    tree = lambda vec: {k: vec[cuts[i]:cuts[i + 1]].clone().view(s) for i, (k, s) in enumerate(PROBE_LEAVES.items())}
    flat = lambda tr: np.concatenate([host(tr[k]).reshape(-1) for k in PROBE_LEAVES])
    clients = [tree(x[k]) for k in range(PROBE_K)]
    for zero_params in (True, False):
        g, p, m, v, want = _probe_expect(coracle, h, t, zero_params)
        params = tree(torch.from_numpy(p.copy()).to(cuda))
        state = opt.init(params)
        state["count"] = t - 1
        for key, val in (("m", m), ("v", v)):
            if key in state:
                state[key] = tree(torch.from_numpy(val).to(cuda))
        mean_out = {k: torch.empty_like(q) for k, q in params.items()}
        state = server.fused_tree_mean_update(list(zip(clients, wi)), opt, params, state, mean_out=mean_out)
        assert state["count"] == t
        assert np.array_equal(bits(flat(mean_out)), bits(g))
        got = {"p": flat(params)}
        got.update({k: flat(state[k]) for k in ("m", "v") if k in want})
        _check_bound(got, want, f"pytree {hyper_id(h)} t={t} p0={zero_params}")


# ------------------------------------------------------- every dense instantiation
def _run_dense(cuda, coracle, h, K, P, bf16, nt, frozen_head=0, steps=2, seed=400):
    """``steps`` rounds of fused_mean_update on a K x P slab from a random state; p, m, v and
    mean_out whole, bitwise. ``frozen_head``: the first leaf has that many elements and is
    frozen (ignore_grads_haiku), so the kernel runs on the columns after it."""
    opt = make_server(h)
    if frozen_head:
        template = {"a": {"w": np.zeros(frozen_head, f32)}, "b": {"w": np.zeros(P - frozen_head, f32)}}
        opt = server.ignore_grads_haiku(opt, [("a", "w")])
    else:
        template = {"w": np.zeros(P, f32)}
    slab = fedjax_amd.ClientDeltaSlab(template, K, dtype=torch.bfloat16 if bf16 else torch.float32, device=cuda)
    p, m, v = probe_state(h, P, seed=seed)
    params = torch.from_numpy(p.copy()).to(cuda)
    state = _set_state(opt.init(params), m, v, 0)
    lo = frozen_head
    p0, m0, v0 = p.copy(), None if m is None else m.copy(), None if v is None else v.copy()
    for rnd in range(steps):
        slab.fill_synthetic(seed=seed + rnd)
        wi = _weights(K, seed + rnd)
        g = oracle_mean(coracle, K, P, bf16, seed + rnd)
        mean_out = torch.empty(P, device=cuda)
        state = server.fused_mean_update(slab, wi, opt, params, state, mean_out=mean_out, nontemporal=nt)
        assert state["count"] == rnd + 1
        assert np.array_equal(bits(host(mean_out)), bits(g)), rnd
        sl = lambda a: None if a is None else a[lo:]
        p2, m2, v2 = _np_step(h, rnd + 1, g[lo:], p[lo:], sl(m), sl(v))
        p[lo:] = p2
        if m is not None:
            m[lo:] = m2
        if v is not None:
            v[lo:] = v2
        assert np.array_equal(bits(host(params)), bits(p)), rnd
        if m is not None:
            assert np.array_equal(bits(host(state["m"])), bits(m)), rnd
        if v is not None:
            assert np.array_equal(bits(host(state["v"])), bits(v)), rnd
    if lo:  # the frozen leaf's params and moments never moved
        assert np.array_equal(bits(p[:lo]), bits(p0[:lo]))
        assert m is None or np.array_equal(bits(m[:lo]), bits(m0[:lo]))
        assert v is None or np.array_equal(bits(v[:lo]), bits(v0[:lo]))
    del slab, params, state
    torch.cuda.empty_cache()


NT = pytest.mark.parametrize("nt", [False, True], ids=["T", "NT"])


@NT
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_dense_a_f32_V4_E8_U4(h, nt, cuda, coracle):
    """(a) k_dense_opt<f32, V=4, E=8, U=4, nt>: K = 32, P = 1 Mi + 4000 + 3 = 263144 units
    (what pick_variant chooses from 262144 units and 32 clients), a tail of 3 in block 0, a
    partial last group; every rule."""
    _run_dense(cuda, coracle, h, 32, 1_048_576 + 4000 + 3, False, nt, seed=410)


@NT
@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_dense_b_bf16_V8_E1_U8(h, nt, cuda, coracle):
    """(b) k_dense_opt<bf16, V=8, E=1, U=8, nt>: K = 5, P = 2405 (300 units, tail 5)."""
    _run_dense(cuda, coracle, h, 5, 2405, True, nt, seed=420)


@NT
@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_dense_c_bf16_V8_E8_U4(h, nt, cuda, coracle):
    """(c) k_dense_opt<bf16, V=8, E=8, U=4, nt>: K = 32, P = 2 Mi + 8000 + 5 (263144 units,
    tail 5)."""
    _run_dense(cuda, coracle, h, 32, 2_097_152 + 8000 + 5, True, nt, seed=430)


@NT
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_dense_d_V1_E1_U8_unaligned_run(h, bf16, nt, cuda, coracle):
    """(d) k_dense_opt<in, V=1, E=1, U=8, nt>: a frozen first leaf of 3 elements puts the
    trainable run 12 (f32) or 6 (bf16) bytes off 16-byte alignment, 2405 elements over
    several workgroups; the frozen leaf keeps its params and moments, mean_out is whole."""
    _run_dense(cuda, coracle, h, 5, 3 + 2405, bf16, nt, frozen_head=3, seed=440)


@NT
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_dense_d_V1_E1_U8_below_one_vector(h, bf16, P, nt, cuda, coracle):
    """(d) k_dense_opt<in, V=1, E=1, U=8, nt>: P below one 16-byte unit."""
    _run_dense(cuda, coracle, h, 5, P, bf16, nt, seed=450)


@pytest.mark.parametrize("K", [1, 8, 33])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32-V4", "bf16-V8"])
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_dense_f_E1_U8_client_counts(h, bf16, K, cuda, coracle):
    """(f) k_dense_opt<in, V, E=1, U=8>: K = 1 (no loop), 8 (one full group of U) and 33
    (four groups and a remainder) at P = 2405; every rule."""
    _run_dense(cuda, coracle, h, K, 2405, bf16, False, seed=460 + K)


# ------------------------------------------------------ every pytree instantiation
TREE_LEAVES = [("a", (0,)), ("b", (1,)), ("c", ()), ("d", (300_000,)), ("e", (3, 5)), ("f", (1009,))]
TREE_CASES = {
    "bf16-V8-aligned": (True, {}),
    "bf16-V1-offset-2B": (True, {k: 1 for k, _ in TREE_LEAVES}),
    "bf16-V1-offset-8B": (True, {k: 4 for k, _ in TREE_LEAVES}),
    "f32-V4-and-V1-mixed": (False, {"f": 1, "e": 1}),  # d (300000), a, b, c aligned; e, f 4 bytes off
}


@pytest.mark.parametrize("nt", [None, False, True], ids=["native", "python", "python-NT"])
@pytest.mark.parametrize("case", list(TREE_CASES))
@pytest.mark.parametrize("h", [ADAM, NESTEROV], ids=hyper_id)
def test_pytree_instantiations_bitwise(h, case, nt, cuda, coracle):
    """k_ptrs_opt<in, V, nt> (V = 8 bf16 / 4 f32 for leaves whose pointers are all 16-byte
    aligned, element units otherwise; the choice is per leaf): leaves of 0 and 1 elements,
    a 0-d leaf, 300000 elements (several workgroups of E=8 groups and a partial one), (3, 5)
    and 1009 (E=1 walk, tail block). ``native`` is the one-call path (fjhost.server_pairs),
    the others the Python path with the cache policy given."""
    bf16, mis = TREE_CASES[case]
    K, seed = 5, 500
    pos, o = {}, 0
    for name, shape in TREE_LEAVES:  # every leaf starts 32 bytes aligned, plus its misalignment
        o = (o + 7) // 8 * 8 + mis.get(name, 0)
        pos[name] = o
        o += int(np.prod(shape))
    ld = (o + 8 + 7) // 8 * 8
    opt = make_server(h)
    p_all, m_all, v_all = probe_state(h, ld, seed=seed)
    cut = lambda a, name, shape: a[pos[name]:pos[name] + int(np.prod(shape))].copy()
    params = {n: torch.from_numpy(cut(p_all, n, s)).to(cuda).view(s) for n, s in TREE_LEAVES}
    state = opt.init(params)
    for key, arr in (("m", m_all), ("v", v_all)):
        if key in state:
            state[key] = {n: torch.from_numpy(cut(arr, n, s)).to(cuda).view(s) for n, s in TREE_LEAVES}
    p_np = {n: cut(p_all, n, s) for n, s in TREE_LEAVES}
    m_np = {n: cut(m_all, n, s) if m_all is not None else None for n, s in TREE_LEAVES}
    v_np = {n: cut(v_all, n, s) if v_all is not None else None for n, s in TREE_LEAVES}
    for rnd in range(2):
        if bf16:
            xb = coracle.synth_bf16(K, ld, seed=seed + rnd)
            x = torch.from_numpy(xb.view(np.int16)).view(torch.bfloat16).to(cuda)
            xh = bf16_to_f32(xb)
        else:
            xh = coracle.synth_f32(K, ld, seed=seed + rnd)
            x = torch.from_numpy(xh).to(cuda)
        clients = [{n: x[k, pos[n]:pos[n] + int(np.prod(s))].view(s) for n, s in TREE_LEAVES} for k in range(K)]
        wi = _weights(K, seed + rnd)
        mean_out = {n: torch.empty_like(q) for n, q in params.items()}
        state = server.fused_tree_mean_update(list(zip(clients, wi)), opt, params, state, mean_out=mean_out,
                                              nontemporal=nt)
        assert state["count"] == rnd + 1
        for n, s in TREE_LEAVES:
            size = int(np.prod(s))
            if size == 0:
                continue
            g = coracle.wsum_f32(np.ascontiguousarray(xh[:, pos[n]:pos[n] + size]), f32(wi),
                                 scale=ref.mean_scale(wi))
            assert np.array_equal(bits(host(mean_out[n]).reshape(-1)), bits(g)), (rnd, n)
            p_np[n], m_np[n], v_np[n] = _np_step(h, rnd + 1, g, p_np[n], m_np[n], v_np[n])
            assert np.array_equal(bits(host(params[n]).reshape(-1)), bits(p_np[n])), (rnd, n)
            for key, want in (("m", m_np[n]), ("v", v_np[n])):
                if want is not None:
                    assert np.array_equal(bits(host(state[key][n]).reshape(-1)), bits(want)), (rnd, n, key)


# ------------------------------------------------------------------- special values
_SUB = float(np.float32(1e-42))
_S = np.array([0.0, -0.0, _SUB, -_SUB, np.inf, -np.inf, np.nan, 1e20, -1e20, 1e-30, 1e-20, -1e-25, 1.0, -1.0,
               0.5, 3e38], f32)  # 1e20^2 = inf; 1e-30^2 = 0, 1e-20^2 subnormal


def _special_inputs(coracle):
    """K = 2 deltas and p, m, v of 64 elements: every pairing of the specials above that a
    few strides reach, then the targeted cases in elements 0..5 (see the test)."""
    i = np.arange(64)
    d = np.stack([_S[i % 16], _S[(5 * i + i // 16) % 16]])
    d[:, 0] = 0.0                      # g = 0
    d[:, 1] = -0.0                     # g = -0
    d[:, 2] = (0.5, 0.25)              # g ordinary; v = g^2 exactly below
    d[:, 3] = (np.nan, 1.0)            # g NaN
    d[:, 4] = (0.125, 0.5)             # g ordinary; v NaN below
    d[:, 5] = (0.1, 0.3)               # centered rmsprop: v' < m'^2
    wi = [3, 5]
    with np.errstate(all="ignore"):
        g = coracle.wsum_f32(np.ascontiguousarray(d), f32(wi), scale=ref.mean_scale(wi))
    p = _S[(7 * i + 3) % 16].copy()
    m = _S[(3 * i + 1 + i // 16) % 16].copy()
    v = _S[(11 * i + 2 * (i // 16)) % 16].copy()
    m[[0, 1]], v[[0, 1]] = 0.0, 0.0    # adagrad: g = 0 and v = 0 gives 0, not NaN
    v[2] = g[2] * g[2]                 # yogi: sign(v - g^2) = 0
    m[2], m[3], v[3], m[4], v[4] = 0.25, 0.5, 1.0, -0.5, np.nan
    m[5], v[5] = 1.0, 1e-6             # the centered variance goes negative: NaN
    p[:6] = (1.0, -0.0, 0.5, 2.0, -1.0, 0.25)
    assert g[0] == 0 and g[1] == 0 and np.signbit(g[1]) and np.isnan(g[3]) and v[2] == f32(g[2] * g[2])
    return d.astype(f32), wi, g, p, m, v


def _check_special(h, t, g, p, m, v, got_mean, got_p, got_m, got_v):
    has_m, has_v = needs(h)
    p2, m2, v2 = _np_step(h, t, g, p.copy(), m.copy() if has_m else None, v.copy() if has_v else None)
    for what, got, want in (("mean", got_mean, g), ("p", got_p, p2), ("m", got_m, m2), ("v", got_v, v2)):
        if want is not None:
            ok = same(got, want)
            assert ok.all(), (what, np.flatnonzero(~ok).tolist(), got.reshape(-1)[~ok], want[~ok])
    if h["kind"] == "adagrad":  # g = 0, v = 0: u = 0 (not NaN), params keep their value (-0 + 0 is +0)
        assert np.array_equal(got_p[:2], p[:2]) and not got_v[:2].any()
    if h.get("centered"):
        assert np.isnan(got_p[5])


@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_special_values_dense(h, cuda, coracle):
    """k_dense_opt<f32, V=4, E=1, U=8>, K = 2, one 64-element leaf, the step with count 3:
    bits (signed zeros included) or NaN on both sides, against _np_server_step."""
    d, wi, g, p, m, v = _special_inputs(coracle)
    opt = make_server(h)
    slab = fedjax_amd.ClientDeltaSlab({"x": np.zeros(64, f32)}, 2, device=cuda)
    for k in range(2):
        slab.set_client(k, {"x": torch.from_numpy(d[k])})
    params = torch.from_numpy(p.copy()).to(cuda)
    state = _set_state(opt.init(params), m, v, 2)
    mean_out = torch.empty(64, device=cuda)
    state = server.fused_mean_update(slab, wi, opt, params, state, mean_out=mean_out)
    _check_special(h, 3, g, p, m, v, host(mean_out), host(params),
                   host(state["m"]) if "m" in state else None, host(state["v"]) if "v" in state else None)


@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_special_values_pytree(h, cuda, coracle):
    """k_ptrs_opt<f32, V=4>, the same inputs as one 64-element leaf."""
    d, wi, g, p, m, v = _special_inputs(coracle)
    opt = make_server(h)
    clients = [{"x": torch.from_numpy(d[k]).to(cuda)} for k in range(2)]
    params = {"x": torch.from_numpy(p.copy()).to(cuda)}
    state = opt.init(params)
    state["count"] = 2
    for key, val in (("m", m), ("v", v)):
        if key in state:
            state[key] = {"x": torch.from_numpy(val.copy()).to(cuda)}
    mean_out = {"x": torch.empty(64, device=cuda)}
    state = server.fused_tree_mean_update(list(zip(clients, wi)), opt, params, state, mean_out=mean_out)
    _check_special(h, 3, g, p, m, v, host(mean_out["x"]), host(params["x"]),
                   host(state["m"]["x"]) if "m" in state else None, host(state["v"]["x"]) if "v" in state else None)
