"""The case generator of the compression sweep (tests/compression_cases.py), checked on the
numpy oracle alone: no GPU and no product code. It pins what tests/test_gpu_compression_fuzz.py
relies on: the cases are a function of the seed, the default seeds reach every kind of case the
sweep is there for, the float32 results of the float64 reductions of every kept terngrad / DRIVE
case do not depend on the summation order, the placements hold the case's values, and the oracle
runs every case."""
import numpy as np
import pytest
import torch

from oracle import compression_ref as cref
from oracle import jax_random_ref as jr
from oracle import tree_util_ref as tu
from tests import compression_cases as cc

SEEDS = range(7000, 7040)  # the seeds of tests/test_gpu_compression_fuzz.py (asserted below)
F32 = np.float32


def _cases():
    return [cc.case(s) for s in SEEDS]


def test_seeds_agree_with_the_gpu_sweep():
    import os

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_compression_fuzz.py")).read()
    assert "SEEDS = range(7000, 7040)" in src


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (float, np.floating)):
        return type(a) is type(b) and np.array(a).tobytes() == np.array(b).tobytes()
    return type(a) is type(b) and a == b


def test_generator_is_deterministic_per_seed():
    for s in (7005, 7009, 7013, 7024):
        a, b = cc.case.__wrapped__(s), cc.case.__wrapped__(s)
        assert a is not b and _same(a, b), s
        assert not _same(a, cc.case.__wrapped__(s + 5))
        assert cc.case(s) is cc.case(s) and _same(cc.case(s), a)  # memoised, and the same draw


def test_cases_are_within_the_lists_and_the_budget():
    for c in _cases():
        L = len(c["sizes"])
        assert 1 <= L <= 24 and all(n in cc.SIZES for n in c["sizes"])
        assert c["K"] in cc.KS and c["kind"] in cc.KINDS
        assert c["K"] * c["P"] <= cc.MAX_ELEMENTS and c["K"] * L <= cc.MAX_CLIENT_LEAVES
        assert all(int(np.prod(s)) == n and len(s) <= 3 for s, n in zip(c["shapes"], c["sizes"]))
        assert len(tu.flatten(cc.realize(c["struct"], list(range(L))))[0]) == L
        assert tu.flatten(cc.realize(c["struct"], list(range(L))))[0] == list(range(L))  # slots in flatten order
        if c["kind"].startswith("uniform"):
            assert c["num_levels"] in cc.LEVELS and c["num_levels"] != 4096
        if c["batch"] is not None:
            assert c["kind"] in ("rotated", "drive") and 1 <= c["batch"] <= c["K"]
            # the product's batch: max(1, min(K, budget // per-client bytes))
            per = cc.per_client_bytes(c["kind"], c["sizes"])
            assert max(1, min(c["K"], c["workspace_bytes"] // per)) == c["batch"]
        for l, p in enumerate(c["placements"]):
            seg = c["x"][:, c["offs"][l]:c["offs"][l + 1]]
            if p == "int32":
                assert (seg == np.round(seg)).all() and (np.abs(seg) < 1 << 24).all()


def test_default_seeds_reach_every_kind_of_case():
    cs = _cases()
    assert {c["kind"] for c in cs} == set(cc.KINDS)
    for kind in cc.KINDS:  # every aggregator meets every class of K
        assert {cc.k_class(c["K"]) for c in cs if c["kind"] == kind} == {0, 1, 2}, kind
    assert {c["K"] for c in cs} & {255, 256} and {c["K"] for c in cs} & {257, 260}  # both sides of the staging
    lead = [c for c in cs if c["sizes"][0] <= 3]
    assert 3 * len(lead) >= len(cs)
    assert {c["kind"] for c in lead} >= {"rotated", "drive"}
    assert {p for c in cs for p in c["placements"]} == set(cc.PLACEMENTS)
    assert any(len(set(c["placements"])) == 1 and c["placements"][0] == "own" for c in cs)
    assert {c["wkind"] for c in cs} == set(cc.WEIGHT_KINDS)
    assert {s for c in cs for s in c["special"]} == set(cc.SPECIALS)
    assert 4 * sum(bool(c["special"]) for c in cs) >= len(cs)
    for kind in ("rotated", "drive"):
        bs = [(c["K"], c["batch"]) for c in cs if c["kind"] == kind]
        assert any(b is None for _, b in bs), kind
        assert any(b is not None and b < K and K % b == 0 for K, b in bs), kind  # whole batches
        assert any(b is not None and K % b for K, b in bs), kind  # a short last batch
    lv = {c["num_levels"] for c in cs if c["kind"] == "uniform"}
    la = {c["num_levels"] for c in cs if c["kind"] == "uniform_arith"}
    assert min(lv | la) < 2048 <= max(x for x in lv | la if x < 4096) and max(lv | la) > 4096
    assert any(x > 4096 for x in la) and any(x < 4096 for x in la)  # both histogram modes
    assert any(x > 4096 for x in lv | la) and any(2048 <= x < 4096 for x in lv | la)
    for c in cs:  # the special values are in the data
        kinds = set(c["special"])
        x = c["x"]
        assert ("nan" in kinds) <= bool(np.isnan(x).any())
        assert ("pinf" in kinds) <= bool((x == np.inf).any()) and ("ninf" in kinds) <= bool((x == -np.inf).any())
        if not kinds:
            assert np.isfinite(x).all()
    assert any(np.signbit(c["x"][c["x"] == 0]).any() for c in cs)  # a -0.0
    assert any(((c["x"] != 0) & (np.abs(c["x"]) < np.finfo(F32).tiny)).any() for c in cs)  # a subnormal
    with np.errstate(all="ignore"):  # such a leaf may also hold an inf
        ratios = [abs(float(seg.mean())) / float(seg.std())
                  for c in cs if "offset_mean" in c["special"]
                  for l, m in enumerate(c["modes"]) if m == "offset_mean"
                  for seg in [c["x"][0, c["offs"][l]:c["offs"][l + 1]].astype(np.float64)]
                  if seg.size >= 31 and seg.std() > 0]
    assert any(300 < r < 3000 for r in ratios), ratios


def test_weights_kinds():
    for c in _cases():
        w = c["weights"]
        total = 0.0
        for v in w:
            total += v
        if c["wkind"] == "zero_total":
            assert total == 0 and all(type(v) is int for v in w)
        elif c["wkind"] == "one_zero":
            assert all(type(v) is int and v >= 0 for v in w) and (c["K"] == 1 or w.count(0) == 1) and total > 0
        else:
            assert all(type(v) is {"int": int, "float": float, "np32": np.float32}[c["wkind"]] and v > 0 for v in w)
        # the oracle's tree_mean of a zero total is the weighted sum times 0.0, not None
    c = next(c for c in _cases() if c["wkind"] == "zero_total")
    leaves = cc.reference(c)[0][0]
    assert leaves is not None and all(((a == 0) | np.isnan(a)).all() for a in leaves)


def _three_orders(v):
    """An independent restatement of the guard's three float64 sums."""
    v = np.asarray(v, np.float64).ravel()
    fwd = 0.0
    for chunk in np.array_split(v, max(1, v.size // 4096)):  # sequential: cumsum inside, carried across
        fwd = float(np.cumsum(np.concatenate([[fwd], chunk]))[-1])
    rev = float(np.add.accumulate(v[::-1].copy())[-1])
    return fwd, rev, float(np.sum(v))


def _f32_bits_equal(vals):
    a = np.array(vals, dtype=F32)
    return bool(np.isnan(a).all()) or len({int(b) for b in a.view(np.uint32)}) == 1


def test_reductions_do_not_depend_on_the_summation_order():
    """The guard, asserted again without the generator's own loop."""
    checked = 0
    for c in _cases():
        K, L, offs = c["K"], len(c["sizes"]), c["offs"]
        if c["kind"] == "terngrad":
            for k in range(K):
                for l in range(L):
                    v = c["x"][k, offs[l]:offs[l + 1]].astype(np.float64)
                    sig = []
                    with np.errstate(all="ignore"):
                        for s1, s2 in zip(_three_orders(v), _three_orders(v * v)):
                            var = s2 / v.size - (s1 / v.size) ** 2
                            var = var if var > 0.0 else (0.0 if var == var else var)
                            sig.append(F32(np.sqrt(var)) if np.isfinite(var) else F32(np.nan))
                        for shift in (v[0], float(np.median(v))):  # and shifted, as the kernel sums
                            if np.isfinite(shift):
                                u = v - shift
                                var = float(np.sum(u * u)) / v.size - (float(np.sum(u)) / v.size) ** 2
                                sig.append(F32(np.sqrt(max(var, 0.0))) if np.isfinite(var) else F32(np.nan))
                    assert _f32_bits_equal(sig), (c["seed"], k, l, sig)
                    checked += 1
        elif c["kind"] == "drive":
            rng = c["key"]
            for r in range(cc.ROUNDS):
                rng, rot = jr.split(rng)
                seq = jr.PRNGSequence(rot)
                for k in range(K):
                    lkeys = jr.split(next(seq), L)
                    for l in range(L):
                        with np.errstate(all="ignore"):
                            y = cref.structured_rotation(c["x"][k, offs[l]:offs[l + 1]], lkeys[l])[0].astype(np.float64)
                            assert _f32_bits_equal(_three_orders(y * y)), (c["seed"], r, k, l)
                            assert _f32_bits_equal(_three_orders(np.abs(y))), (c["seed"], r, k, l)
                        checked += 1
    assert checked > 1000
    # and the guard does see an order-dependent leaf: a leaf of mean / sigma = 1e7 is one
    v = (np.random.RandomState(0).standard_normal(3001) * 1e-6 + 10.0).astype(F32)
    fake = dict(kind="terngrad", K=1, sizes=[v.size], offs=np.array([0, v.size]), x=v[None, :])
    assert cc.order_sensitive(fake) == [(0, 0, 0)]


def test_placements_hold_the_values():
    seen_unaligned = 0
    for c in _cases():
        trees = cc.place(c, "cpu")
        assert len(trees) == c["K"]
        for k, tree in enumerate(trees):
            if k not in (0, 1, c["K"] - 1):
                continue
            leaves = tu.flatten(tree)[0]
            for l, (leaf, kind) in enumerate(zip(leaves, c["placements"])):
                want = c["x"][k, c["offs"][l]:c["offs"][l + 1]].reshape(c["shapes"][l])
                if kind == "host":
                    assert isinstance(leaf, np.ndarray) and leaf.dtype == np.float32
                    got = leaf
                else:
                    assert isinstance(leaf, torch.Tensor)
                    assert leaf.dtype == (torch.int32 if kind == "int32" else torch.float32)
                    got = leaf.to(torch.float32).numpy()
                    if kind == "noncontig" and c["sizes"][l] > 1:
                        assert not leaf.is_contiguous()
                    if kind == "offset_view":
                        assert leaf.data_ptr() % 4 == 0
                        seen_unaligned += leaf.data_ptr() % 16 != 0
                assert tuple(got.shape) == tuple(c["shapes"][l])
                assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (c["seed"], k, l)
        first = [l for l, p in enumerate(c["placements"]) if p == "offset_view"]
        if first:  # client 0's first offset view really is off 16-byte alignment
            leaf = tu.flatten(trees[0])[0][first[0]]
            base = leaf.untyped_storage().data_ptr()
            assert (leaf.data_ptr() - base) % 16 != 0 and (base % 16 == 0) <= (leaf.data_ptr() % 16 != 0)
    assert seen_unaligned > 20


def test_oracle_runs_every_case():
    for c in _cases():
        out = cc.reference(c)
        assert len(out) == cc.ROUNDS and cc.reference(c) is out
        for leaves, num_bits, rng in out:
            assert leaves is not None and [a.shape for a in leaves] == [tuple(s) for s in c["shapes"]]
            assert all(a.dtype == np.float32 for a in leaves)
            assert np.asarray(rng).dtype == np.uint32 and np.asarray(rng).shape == (2,)
            float(num_bits)
        assert not np.array_equal(out[0][2], out[1][2])
    # ordinary cases compare finite numbers
    finite = sum(all(np.isfinite(a).all() for a in cc.reference(c)[0][0]) for c in _cases())
    assert finite >= 30
