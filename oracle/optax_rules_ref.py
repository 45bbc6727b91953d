"""Test infrastructure only (the product never imports this, and this imports nothing of
the product): a float64 evaluation of the server rules fedjax.optimizers wraps from optax
(sgd / trace / scale_by_adam / scale_by_rss / scale_by_rms / scale_by_stddev /
scale_by_yogi, then scale_by_learning_rate and apply_updates), with a running
first-order bound of what a float32 evaluation of the same expression may differ by.

PARITY UNPINNED: optax is absent from this image; the rules below restate its published
definitions. ``t`` is the step's INCREMENTED count; a schedule is read at ``t - 1``.

    sgd        u = g
    momentum   m' = g + decay m;  u = g + decay m' (nesterov) | m'
    adam       m' = (1-b1) g + b1 m;  v' = (1-b2) g^2 + b2 v
               u = (m' / (1-b1^t)) / (sqrt(v' / (1-b2^t) + eps_root) + eps)
    adagrad    v' = g^2 + v;  u = g (v' + eps)^-1/2 where v' > 0, else 0
    rmsprop    v' = (1-decay) g^2 + decay v;  centered: m' = (1-decay) g + decay m,
               den = v' - m'^2 (else v');  u = g (den + eps)^-1/2
               with momentum: s = -lr u;  m' = s + mom m;  p' = p + (s + mom m' | m')
    yogi       m' = (1-b1) g + b1 m;  v' = v - (1-b2) sign(v - g^2) g^2;  u as adam's
    all but rmsprop with momentum:  p' = p + (-lr) u

Hyperparameters enter as the float32 values optax's weak-typed Python scalars become
(``f32(b)``, ``f32(1 - b)``, ``f32(eps)``, ``f32(-lr)``), evaluated exactly in float64.

Every value carries an absolute bound ``e`` for a float32 evaluation (unit roundoff
``U = 2**-24``): add/sub ``ea + eb + U|r|``; mul ``|a| eb + |b| ea + U|r|``; div, sqrt,
rsqrt their first-order propagation ``+ U|r|``; ``b32 ** t`` gets ``2 U b32**t`` (powf
within 1 ulp, margin 2). A float32 result passes when ``|x - ref| <= 2 * bound``: the
factor 2 covers the second-order terms. Discrete choices (adagrad's ``v' > 0``, yogi's
sign) are taken on the float64 values, so inputs where they sit on the edge are out of
scope here.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import numpy as np

U = 2.0 ** -24
KINDS = ("sgd", "momentum", "adam", "adagrad", "rmsprop", "yogi")


class _B:
    """A float64 value and the bound of its float32 evaluation's absolute error."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64) + np.zeros_like(self.v)

    @staticmethod
    def of(x):
        return x if isinstance(x, _B) else _B(x)

    def __add__(self, o):
        o = _B.of(o)
        r = self.v + o.v
        return _B(r, self.e + o.e + U * np.abs(r))

    def __sub__(self, o):
        o = _B.of(o)
        r = self.v - o.v
        return _B(r, self.e + o.e + U * np.abs(r))

    def __mul__(self, o):
        o = _B.of(o)
        r = self.v * o.v
        return _B(r, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(r))

    def __truediv__(self, o):
        o = _B.of(o)
        r = self.v / o.v
        return _B(r, self.e / np.abs(o.v) + np.abs(r) * o.e / np.abs(o.v) + U * np.abs(r))

    def sqrt(self):
        r = np.sqrt(self.v)
        return _B(r, self.e / (2.0 * r) + U * r)

    def rsqrt(self):
        r = 1.0 / np.sqrt(self.v)
        return _B(r, 0.5 * r * self.e / np.abs(self.v) + U * r)


def _c(x) -> float:
    """A hyperparameter as optax's weak-typed scalar: rounded to float32, held exactly."""
    return float(np.float32(x))


def _bias_correction(b: float, t: int) -> _B:
    """1 - b32 ** t."""
    pw = np.power(np.float64(_c(b)), np.float64(t))
    return _B(1.0) - _B(pw, 2.0 * U * pw)


def neg_lr(lr: Union[float, Callable[[int], float]], t: int) -> float:
    """f32(-lr) of the step whose incremented count is t (a schedule is read at t - 1)."""
    val = lr(t - 1) if callable(lr) else lr
    return _c(-float(np.asarray(val, np.float64)))


def step(kind: str, t: int, g, p, m=None, v=None, *, lr, momentum: Optional[float] = None,
         nesterov: bool = False, b1: float = 0.9, b2: float = 0.999, decay: Optional[float] = None,
         eps: float = 1e-8, eps_root: float = 0.0, centered: bool = False) -> dict:
    """One step of rule ``kind`` on float32 arrays. Returns ``{"p": (value, bound), "m": ...,
    "v": ...}`` with float64 arrays; "m" / "v" only where the rule keeps them. ``decay`` is
    rmsprop's (``b2`` is read when it is None); ``momentum`` is the trace decay."""
    if kind not in KINDS:
        raise ValueError(kind)
    for x in (g, p, m, v):
        if x is not None and np.asarray(x).dtype != np.float32:
            raise TypeError("g, p, m, v are float32 arrays")
    g, p = _B(g), _B(p)
    m = None if m is None else _B(m)
    v = None if v is None else _B(v)
    nlr = neg_lr(lr, t)
    out = {}
    if kind == "sgd":
        u = g
    elif kind == "momentum":
        d = _c(momentum)
        m = g + _B(d) * m
        u = g + _B(d) * m if nesterov else m
        out["m"] = m
    elif kind in ("adam", "yogi"):
        m = _B(_c(1 - b1)) * g + _B(_c(b1)) * m
        if kind == "adam":
            v = _B(_c(1 - b2)) * (g * g) + _B(_c(b2)) * v
        else:
            g2 = g * g
            sign = np.sign((v - g2).v)
            v = v - (_B(_c(1 - b2)) * _B(sign)) * g2
        out["m"], out["v"] = m, v
        mh, vh = m / _bias_correction(b1, t), v / _bias_correction(b2, t)
        u = mh / ((vh + _B(_c(eps_root))).sqrt() + _B(_c(eps)))
    elif kind == "adagrad":
        v = g * g + v
        out["v"] = v
        pos = v.v > 0
        s = (v + _B(_c(eps))).rsqrt()
        s = _B(np.where(pos, s.v, 0.0), np.where(pos, s.e, 0.0))
        u = s * g
    else:  # rmsprop
        dc = b2 if decay is None else decay
        v = _B(_c(1 - dc)) * (g * g) + _B(_c(dc)) * v
        out["v"] = v
        den = v
        if centered:
            m = _B(_c(1 - dc)) * g + _B(_c(dc)) * m
            out["m"] = m
            den = v - m * m
        u = g * (den + _B(_c(eps))).rsqrt()
        if momentum is not None:
            mom = _c(momentum)
            s = _B(nlr) * u
            m = s + _B(mom) * m
            out["m"] = m
            out["p"] = p + (s + _B(mom) * m if nesterov else m)
    if "p" not in out:
        out["p"] = p + _B(nlr) * u
    return {k: (x.v, x.e) for k, x in out.items()}


def within(x, ref, bound) -> np.ndarray:
    """bool per element: the float32 result ``x`` passes against ``(ref, bound)``."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(x, np.float64) - ref) <= 2.0 * bound
