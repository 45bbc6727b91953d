"""The case generator of the centered-clipping sweep (tests/centered_clip_cases.py), checked on
the numpy restatement alone: no GPU and no product code. It pins what keeps
tests/test_gpu_centered_clip_fuzz.py from being hollow: the cases are a function of the seed, the
default seeds reach every K class, tau regime and iteration count, enough of them have a leaf of
more than one norm block, a centre leaf that alone is misaligned, and special values, and every
median-tau case really clips some clients and not others."""
import os

import numpy as np

from tests import centered_clip_cases as cc


def _cases():
    if not hasattr(_cases, "v"):
        _cases.v = [cc.case(cc.SEED0 + s) for s in range(cc.NCASES)]
    return _cases.v


def _same(a, b):
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a if k != "_refs")
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return type(a) is type(b) and np.array(a).tobytes() == np.array(b).tobytes()
    return type(a) is type(b) and a == b


def test_defaults_agree_with_the_gpu_sweep():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_centered_clip_fuzz.py")).read()
    assert "cc.NCASES" in src and "cc.SEED0" in src and "skip" not in src and "xfail" not in src
    assert cc.NCASES >= 48


def test_generator_is_deterministic_per_seed():
    for s in (0, 1, 6, 11):
        a, b = cc.case.__wrapped__(cc.SEED0 + s), cc.case.__wrapped__(cc.SEED0 + s)
        assert a is not b and _same(a, b), s
        assert not _same(a, cc.case.__wrapped__(cc.SEED0 + s + 1))
    np.random.seed(1)  # no global random state
    assert _same(cc.case.__wrapped__(cc.SEED0), _cases()[0])


def test_cases_are_well_formed():
    for c in _cases():
        K, P, sizes = c["K"], c["P"], c["sizes"]
        assert K in cc.KS and 1 <= len(sizes) <= 9 and set(sizes) <= set(cc.SIZES)
        assert 1 <= P == sum(sizes) and K * P <= cc.MAX_ELEMENTS
        assert c["x"].shape == (K, P) and c["x"].dtype == np.float32 and c["v"].shape == (P,)
        assert 1 <= c["iterations"] <= 4 and c["tau_kind"] in cc.TAU_KINDS
        assert np.isfinite(np.float32(c["tau"])) and np.float32(c["tau"]) > 0
        assert c["delta_offsets"].shape == (K, len(sizes)) and c["centre_offsets"].shape == (len(sizes),)
        assert 0 <= c["delta_offsets"].min() and c["delta_offsets"].max() <= 3
        assert 0 <= c["centre_offsets"].min() and c["centre_offsets"].max() <= 3
        assert np.isfinite(c["v"]).all()
        zeros = c["v"][c["v"] == 0]
        assert P < 64 or (np.signbit(zeros).any() and not np.signbit(zeros).all()), "a centre with +0 and -0"
        clean = np.isfinite(c["x"]).all(axis=1) & (np.abs(c["x"]) < 1e29).all(axis=1)
        assert c["special"] == (not clean.all()) and sorted(np.flatnonzero(~clean)) == sorted(c["special_rows"])
        assert clean.sum() >= min(K, 2)


def _centre_alone_misaligned(c):
    """A non-empty leaf whose centre is 4-byte aligned only while every client's delta is 16-byte aligned."""
    return any(n > 0 and co != 0 and not c["delta_offsets"][:, l].any()
               for l, (n, co) in enumerate(zip(c["sizes"], c["centre_offsets"])))


def test_default_seeds_keep_the_sweep_from_being_hollow():
    cs = _cases()
    assert {cc.k_class(c["K"]) for c in cs} == {0, 1, 2, 3}, "every K class"
    assert {c["tau_kind"] for c in cs} == set(cc.TAU_KINDS), "every tau regime"
    assert {c["iterations"] for c in cs} == {1, 2, 3, 4}, "every iteration count"
    assert sum(max(c["sizes"]) > 65536 for c in cs) * 4 >= len(cs), "a leaf over one norm block"
    assert sum(_centre_alone_misaligned(c) for c in cs) * 4 >= len(cs), "a misaligned centre leaf, aligned deltas"
    assert sum(c["special"] for c in cs) * 3 >= len(cs), "specials"
    assert any(c["in_place"] for c in cs) and not all(c["in_place"] for c in cs)
    assert any(c["delta_offsets"].any() for c in cs), "misaligned deltas"
    assert any(not c["delta_offsets"].any() and not c["centre_offsets"].any() for c in cs), "everything aligned"
    assert any(0 in c["sizes"] for c in cs) and any(c["K"] == 1 for c in cs)


def test_median_tau_clips_some_clients_and_not_others():
    """In every median-tau case the restatement alone, over the case's own leaf cut, clips between
    one and K - 1 clients in the first iteration; huge clips nobody, tiny every usable client, and
    the boundary client's first factor is exactly 1."""
    seen = 0
    for c in _cases():
        centre, dist, fac = cc.reference(c)
        K = c["K"]
        usable = np.isfinite(dist[0])
        if c["tau_kind"] == "median":
            clipped = int((fac[0][usable] < 1).sum())
            assert 1 <= clipped <= K - 1 and (fac[0] == 1).any(), (c["seed"], clipped, K)
            seen += 1
        elif c["tau_kind"] == "huge":
            assert (fac[0][usable] == 1).all()
        elif c["tau_kind"] == "tiny":
            assert (fac[0][usable] < 1e-2).all() and usable.any()
        else:
            on = np.flatnonzero(dist[0] == np.float32(c["tau"]))
            assert on.size >= 1 and (fac[0][on] == 1).all() and ((fac[0] < 1).any() or usable.sum() == 1)
        assert not c["special"] or not np.isfinite(fac[0]).all() or (fac[0] == 0).any()
        assert dist.shape == fac.shape == (c["iterations"], K) and centre.shape == (c["P"],)
        assert np.isfinite(centre).all(), "skipped clients never reach the centre"
    assert seen >= 6
