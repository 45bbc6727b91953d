"""The float64 reference of the server rules (oracle/optax_rules_ref.py) has teeth: a
float32 restatement with constants computed here from the public hyperparameters agrees
with it inside its bound, the bound is sharp (<= 1e-3 relative), deliberate errors in the
restatement break it, and ``ServerOptimizer.descriptor`` carries these constants.

No GPU: the probes, hyperparameter sets and the float32 restatement defined here are what
tests/test_gpu_server_kernels.py runs through the fused kernels.
"""
import types

import numpy as np
import pytest

from oracle import optax_rules_ref as rules

f32 = np.float32
COUNTS = [1, 2, 7, 1000, 100000]


def _schedule(c):
    return 0.1 / (1.0 + 0.5 * c)


# tests/test_gpu_parity.py's OPTIMIZERS as public hyperparameters, plus one schedule
HYPER = [
    dict(kind="sgd", lr=0.5),
    dict(kind="momentum", lr=0.1, momentum=0.9),
    dict(kind="momentum", lr=0.1, momentum=0.9, nesterov=True),
    dict(kind="adam", lr=10 ** -2.5, b1=0.9, b2=0.999, eps=1e-4),
    dict(kind="adagrad", lr=0.1, eps=1e-6, init_v=0.1),
    dict(kind="adagrad", lr=0.3, eps=1e-7, init_v=0.0),
    dict(kind="rmsprop", lr=0.01, decay=0.9, eps=1e-8),
    dict(kind="rmsprop", lr=0.01, decay=0.8, eps=1e-8, init_v=1.0, momentum=0.5),
    dict(kind="rmsprop", lr=0.01, decay=0.9, eps=1e-8, momentum=0.9, nesterov=True),
    dict(kind="rmsprop", lr=0.01, decay=0.9, eps=1e-8, centered=True),
    dict(kind="rmsprop", lr=0.02, decay=0.7, eps=1e-8, centered=True, init_v=1.0),
    dict(kind="yogi", lr=0.01, b1=0.9, b2=0.999, eps=1e-3),
    dict(kind="yogi", lr=0.05, b1=0.5, b2=0.99, eps=1e-4),
    dict(kind="momentum", lr=_schedule, momentum=0.9, nesterov=True),
]
N_PARITY = 13  # HYPER[:N_PARITY] mirrors OPTIMIZERS


def hyper_id(h):
    extra = [k for k in ("nesterov", "centered") if h.get(k)] + (["mom"] if h["kind"] == "rmsprop" and
                                                                  h.get("momentum") is not None else [])
    lr = "sched" if callable(h["lr"]) else f"{h['lr']:.3g}"
    return "-".join([h["kind"], lr] + extra)


def rule_kwargs(h):
    """Arguments of rules.step (the public hyperparameters, no initial values)."""
    return {k: v for k, v in h.items() if k not in ("kind", "init_v")}


def make_server(h):
    """The ServerOptimizer of the hyperparameter set ``h``."""
    from fedjax_amd import server
    k = h["kind"]
    if k in ("sgd", "momentum"):
        return server.sgd(h["lr"], momentum=h.get("momentum"), nesterov=h.get("nesterov", False))
    if k == "adam":
        return server.adam(h["lr"], b1=h["b1"], b2=h["b2"], eps=h["eps"], eps_root=h.get("eps_root", 0.0))
    if k == "adagrad":
        return server.adagrad(h["lr"], initial_accumulator_value=h["init_v"], eps=h["eps"])
    if k == "rmsprop":
        return server.rmsprop(h["lr"], decay=h["decay"], eps=h["eps"], initial_scale=h.get("init_v", 0.0),
                              centered=h.get("centered", False), momentum=h.get("momentum"),
                              nesterov=h.get("nesterov", False))
    return server.yogi(h["lr"], b1=h["b1"], b2=h["b2"], eps=h["eps"])


def needs(h):
    """(keeps m, keeps v)."""
    k = h["kind"]
    has_m = k in ("momentum", "adam", "yogi") or (k == "rmsprop" and (h.get("momentum") is not None
                                                                     or h.get("centered", False)))
    return has_m, k in ("adam", "adagrad", "rmsprop", "yogi")


def consts(h, t, mut=()):
    """The float32 constants of the step with incremented count ``t``, from the public
    hyperparameters alone (fields named as struct fjagg_server_opt's)."""
    k = h["kind"]
    lr = h["lr"]
    lr = lr(t if "sched_at_t" in mut else t - 1) if callable(lr) else lr
    b1 = h.get("b1", 0.9)
    b2 = h["decay"] if k == "rmsprop" else h.get("b2", 0.999)
    tb = t - 1 if "bc_t_minus_1" in mut else t
    with np.errstate(divide="ignore"):
        return types.SimpleNamespace(
            kind=1 + rules.KINDS.index(k), nesterov=int(h.get("nesterov", False)),
            neg_lr=f32(-float(np.asarray(lr, np.float64))), decay=f32(h.get("momentum") or 0.0),
            one_minus_b1=f32(1 - b1), b1=f32(b1), one_minus_b2=f32(1 - b2), b2=f32(b2),
            bc1=f32(1) - np.power(f32(b1), f32(tb)), bc2=f32(1) - np.power(f32(b2), f32(tb)),
            eps=f32(h.get("eps", 1e-8)), eps_root=f32(h.get("eps_root", 0.0)),
            flags=(1 if k == "rmsprop" and h.get("momentum") is not None else 0) | (
                2 if k == "rmsprop" and h.get("centered", False) else 0))


def _rsqrt(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(x.astype(np.float64))).astype(f32)


def f32_step(h, t, g, p, m, v, mut=()):
    """The rules in IEEE float32 ops (numpy: no contraction; / and sqrt correctly rounded),
    op order as the definitions read. ``mut`` names deliberate errors."""
    c = consts(h, t, mut)
    k = h["kind"]
    nesterov = bool(c.nesterov) and "no_nesterov" not in mut
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if k == "sgd":
            u = g
        elif k == "momentum":
            m = g + c.decay * m
            u = g + c.decay * m if nesterov else m
            out["m"] = m
        elif k in ("adam", "yogi"):
            m = c.one_minus_b1 * g + c.b1 * m
            if k == "adam":
                v = c.one_minus_b2 * (g * g) + c.b2 * v
            else:
                g2 = g * g
                v = v - (c.one_minus_b2 * np.sign(v - g2)).astype(f32) * g2
            out["m"], out["v"] = m, v
            mh, vh = (m, v) if "no_bc" in mut else (m / c.bc1, v / c.bc2)
            if "eps_in_sqrt" in mut:
                u = mh / np.sqrt(vh + c.eps_root + c.eps)
            else:
                u = mh / (np.sqrt(vh + c.eps_root) + c.eps)
        elif k == "adagrad":
            v = g * g + v
            out["v"] = v
            u = np.where(v > 0, _rsqrt(v + c.eps), f32(0)) * g
        else:
            v = c.one_minus_b2 * (g * g) + c.b2 * v
            out["v"] = v
            den = v
            if c.flags & 2:
                m = c.one_minus_b2 * g + c.b2 * m
                out["m"] = m
                den = v if "centered_no_m2" in mut else v - m * m
            u = g * _rsqrt(den + c.eps)
            if c.flags & 1:
                if "trace_before_lr" in mut:
                    m = u + c.decay * m
                    out["m"] = m
                    out["p"] = p + c.neg_lr * (u + c.decay * m if nesterov else m)
                else:
                    s = c.neg_lr * u
                    m = s + c.decay * m
                    out["m"] = m
                    out["p"] = p + (s + c.decay * m if nesterov else m)
        if "p" not in out:
            out["p"] = p + c.neg_lr * u
    assert all(x.dtype == f32 for x in out.values())
    return out


def _signed(rs, n, scale):
    return (rs.choice([-1.0, 1.0], n) * rs.uniform(0.25, 1.0, n) * scale).astype(f32)


def probe_state(h, n, seed, zero_params=False):
    """A chosen state before the step: random-sign m of magnitude 0.005..0.02, positive v
    of 1e-4..4e-4 (centered rmsprop: v >= m^2 + 1e-4), params 0 or of magnitude 0.25..1.
    Magnitudes keep every intermediate well inside float32's normal range and away from
    cancellation, so the reference's bound stays below 1e-3 relative."""
    rs = np.random.RandomState(seed)
    p = np.zeros(n, f32) if zero_params else _signed(rs, n, 1.0)
    m = _signed(rs, n, 0.02)
    v = (rs.uniform(0.25, 1.0, n) * 4e-4).astype(f32)
    if h.get("centered"):
        v = (m.astype(np.float64) ** 2 + v).astype(f32)
    has_m, has_v = needs(h)
    return p, (m if has_m else None), (v if has_v else None)


def probe_grad(n, seed):
    return _signed(np.random.RandomState(seed + 1000), n, 0.02)


N = 4096


def _probe(h, t, zero_params, mut=()):
    p, m, v = probe_state(h, N, seed=t % 97, zero_params=zero_params)
    g = probe_grad(N, seed=t % 97)
    want = rules.step(h["kind"], t, g, p, m, v, **rule_kwargs(h))
    got = f32_step(h, t, g, p, None if m is None else m.copy(), None if v is None else v.copy(), mut)
    assert set(got) == set(want)
    return got, want


@pytest.mark.parametrize("zero_params", [True, False], ids=["p0", "prand"])
@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_float32_restatement_agrees_and_bound_is_sharp(h, t, zero_params):
    got, want = _probe(h, t, zero_params)
    for key, (ref, bound) in want.items():
        ok = rules.within(got[key], ref, bound)
        assert ok.all(), (key, int((~ok).sum()), float(np.max(np.abs(got[key] - ref) / bound)))
        sharp = bound <= 1e-3 * np.abs(ref)
        assert sharp.mean() >= 0.99, (key, float(sharp.mean()))


# betas under which the count shows in the bias correction: 0.9 ** t is below float32's
# roundoff of 1 from t = 200 on (0.999 ** t from t = 20000), so t = 100000 takes b1 = 0.99999
def _mut_betas(t):
    return (0.9, 0.999) if t <= 1000 else (0.99999, 0.999)


def _adamlike(kind, t, b2=None):
    b1, b2_t = _mut_betas(t)
    return dict(kind=kind, lr=10 ** -2.5, b1=b1, b2=b2 or b2_t, eps=1e-4)


# eps inside the root moves u by eps / (2 s^2) instead of eps / s (s = sqrt(v_hat)): the two
# meet at s = 1/2, which b2 = 0.999 at t = 1 puts v_hat = 1000 v' next to; b2 = 0.99 keeps
# s <= 0.2 at every count
MUTATIONS = (
    [(m, _adamlike(k, t), t) for m in ("bc_t_minus_1", "no_bc") for k in ("adam", "yogi") for t in COUNTS]
    + [("eps_in_sqrt", _adamlike(k, t, b2=0.99), t) for k in ("adam", "yogi") for t in COUNTS]
    + [("no_nesterov", h, t) for h in (HYPER[2], HYPER[8]) for t in (1, 7)]
    + [("sched_at_t", HYPER[13], t) for t in COUNTS]
    + [("centered_no_m2", h, t) for h in (HYPER[9], HYPER[10]) for t in (1, 7)]
    + [("trace_before_lr", h, t) for h in (HYPER[7], HYPER[8]) for t in (1, 7)])


@pytest.mark.parametrize("mut,h,t", MUTATIONS, ids=[f"{m}-{hyper_id(h)}-t{t}" for m, h, t in MUTATIONS])
def test_mutation_violates_the_bound(mut, h, t):
    got, want = _probe(h, t, zero_params=True)
    for key, (ref, bound) in want.items():  # the unmutated restatement passes on these inputs
        assert rules.within(got[key], ref, bound).all(), key
    bad, want = _probe(h, t, zero_params=True, mut=(mut,))
    broken = np.zeros(N, bool)
    for key, (ref, bound) in want.items():
        broken |= ~rules.within(bad[key], ref, bound)
    assert broken.mean() >= 0.5, float(broken.mean())


@pytest.mark.parametrize("t", COUNTS)
@pytest.mark.parametrize("h", HYPER, ids=hyper_id)
def test_descriptor_carries_these_constants(h, t):
    d = make_server(h).descriptor(t)
    c = consts(h, t)
    for name in ("kind", "nesterov", "flags"):
        assert getattr(d, name) == getattr(c, name), name
    for name in ("neg_lr", "decay", "one_minus_b1", "b1", "one_minus_b2", "b2", "eps", "eps_root"):
        assert f32(getattr(d, name)).view(np.uint32) == f32(getattr(c, name)).view(np.uint32), name
    assert d.neg_lr == f32(rules.neg_lr(h["lr"], t))
    for name, b in (("bc1", c.b1), ("bc2", c.b2)):  # 1 - b32 ** t with powf's allowance
        pw = np.power(np.float64(b), np.float64(t))
        ref = 1.0 - pw
        assert abs(float(getattr(d, name)) - ref) <= 2 * rules.U * pw + rules.U * abs(ref), (name, t)


def test_hyper_mirrors_the_parity_suites_optimizers():
    from fedjax_amd import server
    from tests.test_gpu_parity import OPTIMIZERS
    assert len(OPTIMIZERS) == N_PARITY
    for make, h in zip(OPTIMIZERS, HYPER):
        assert make(server) == make_server(h), hyper_id(h)
