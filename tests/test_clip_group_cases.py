"""The case generator of the clipped / grouped mean sweep (tests/clip_group_cases.py), checked
on the numpy restatements alone: no GPU and no product code. It pins what
tests/test_gpu_clip_group_fuzz.py relies on: the cases are a function of the seed, most of
them compare finite numbers (not NaN with NaN), and the default seeds reach every kind of
case the sweep is there for."""
import ast
import os

import numpy as np
import torch

from tests import clip_group_cases as cg
from tests import clipped_mean_ref as cref

NCASES, SEED0 = 40, 5000  # the defaults of tests/test_gpu_clip_group_fuzz.py (asserted below)


def _cases():
    if not hasattr(_cases, "v"):
        _cases.v = [cg.case(SEED0 + s) for s in range(NCASES)]
    return _cases.v


def _module_constants(name):
    """Top-level ``NAME = <literal>`` assignments of a test module, without importing it."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    out = {}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            try:
                out[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    return out


def test_defaults_agree_with_the_gpu_sweep():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_clip_group_fuzz.py")).read()
    assert f'"FJ_FUZZ_CASES", "{NCASES}"' in src and f'"FJ_FUZZ_SEED0", "{SEED0}"' in src
    assert cg.SIZES == _module_constants("test_gpu_fuzz.py")["SIZES"]


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
    for s in (0, 3, 5, 17):
        a, b = cg.case.__wrapped__(SEED0 + s), cg.case.__wrapped__(SEED0 + s)
        assert a is not b and _same(a, b), s
        assert not _same(a, cg.case.__wrapped__(SEED0 + s + 1))
    # drawing other cases in between changes nothing (no global random state)
    np.random.seed(1)
    assert _same(cg.case.__wrapped__(SEED0), _cases()[0])


def test_cases_are_well_formed():
    for c in _cases():
        K, P = c["K"], c["P"]
        assert K in cg.KS and 1 <= len(c["sizes"]) <= 70
        assert c["x"].shape == (K, P) and c["x"].dtype == np.float32 and P == sum(c["sizes"])
        assert [int(np.prod(s, dtype=np.int64)) for s in c["shapes"]] == c["sizes"]
        assert all(len(s) <= 3 for s in c["shapes"])
        assert len(c["weights"]) == len(c["gweights"]) == K
        assert 1 <= c["G"] <= K + 3 and c["ids"].shape == (K,)
        assert c["ids"].min() >= -1 and c["ids"].max() < c["G"]
        assert set(c["placements"]) <= set(cg.PLACEMENTS)
        assert c["special"] or np.isfinite(c["x"]).all()
        assert c["special"] == (not np.isfinite(c["x"]).all()) or not c["special"]
    assert sum(not np.isfinite(c["x"]).all() for c in _cases()) <= NCASES // 4  # at most one case in four


def test_placements_on_the_cpu_hold_the_case_values():
    """place() on the CPU device: every leaf has its shape, kind and the row's values."""
    for c in _cases()[:12]:
        trees = cg.place(c, torch.device("cpu"))
        assert len(trees) == c["K"]
        for k in (0, c["K"] - 1):
            leaves = _leaves(trees[k])
            assert len(leaves) == len(c["sizes"])
            o = 0
            for leaf, n, s, kind in zip(leaves, c["sizes"], c["shapes"], c["placements"]):
                assert tuple(leaf.shape) == tuple(s)
                if kind == "host":
                    assert isinstance(leaf, np.ndarray) and leaf.dtype == np.float32
                    got = leaf
                else:
                    assert isinstance(leaf, torch.Tensor)
                    assert leaf.dtype == (torch.float64 if kind == "f64" else torch.float32)
                    if kind == "noncontig" and n > 1:
                        assert not leaf.is_contiguous()
                    if kind == "offset_view":
                        assert leaf.is_contiguous() and leaf.storage_offset() >= (c["view_start"] + k) % 4
                    got = leaf.to(torch.float32).contiguous().numpy()
                assert cref.bits(got.reshape(-1)).tobytes() == cref.bits(c["x"][k, o:o + n]).tobytes()
                o += n


def _leaves(tree):
    """Leaves in flatten order (dict keys sorted)."""
    if isinstance(tree, dict):
        return [x for k in sorted(tree) for x in _leaves(tree[k])]
    if isinstance(tree, (list, tuple)):
        return [x for t in tree for x in _leaves(t)]
    return [tree]


def test_most_cases_compare_finite_numbers():
    """A cap on degenerate cases: at least 75 % of the clipped cases have an all-finite reference
    mean, and at least 75 % of the grouped cases at least one group with an all-finite mean."""
    cs = _cases()
    finite_clipped = sum(bool(np.isfinite(cg.clipped_reference(c)[1]).all()) for c in cs)
    finite_grouped = sum(any(m is not None and np.isfinite(m).all() for m in cg.grouped_reference(c)) for c in cs)
    assert finite_clipped >= 0.75 * len(cs), finite_clipped
    assert finite_grouped >= 0.75 * len(cs), finite_grouped


def test_default_seeds_cover_every_kind():
    cs = _cases()
    assert {p for c in cs for p in c["placements"]} == set(cg.PLACEMENTS)
    assert any(len(set(c["placements"])) > 1 for c in cs)  # mixed within one tree
    assert any(0 in c["sizes"] for c in cs) and any(() in c["shapes"] for c in cs)
    assert any(len(s) == 3 for c in cs for s in c["shapes"])
    assert any(c["K"] >= 129 for c in cs) and {128, 129} <= {c["K"] for c in cs}
    assert any(len(c["sizes"]) > 64 for c in cs)
    assert {c["wkind"] for c in cs} == set(cg.WEIGHT_KINDS)
    assert {c["clip_kind"] for c in cs} == set(cg.CLIP_KINDS)
    factors = [cg.clipped_reference(c)[0] for c in cs]
    assert any((f == 1).all() for f in factors), "nothing clipped"
    assert any((f != 1).all() for f in factors), "everything clipped"
    assert any((f == 1).any() and (f < 1).any() for f in factors), "some clipped, some not"
    counts = [np.bincount(c["ids"][c["ids"] >= 0], minlength=c["G"]) for c in cs]
    assert any((n == 0).any() for n in counts), "an empty group"
    assert any((n == 1).any() for n in counts), "a single-member group"
    assert any((n > 60).any() for n in counts), "a group of more than 60 members"
    assert any(c["G"] > c["K"] for c in cs), "G > K"
    assert any((c["ids"] == -1).any() for c in cs)

    def totals(c):
        t = [0] * c["G"]
        for w, g in zip(c["gweights"], c["ids"]):
            if g >= 0:
                t[g] += w
        return t
    assert any(any(n > 0 and t == 0 for n, t in zip(cnt, totals(c))) for c, cnt in zip(cs, counts)), "a zero total"
    assert any(any(t != t for t in totals(c)) for c in cs), "a NaN weight in a group"
    assert any(c["special"] for c in cs)
    # both ends of the fold's plans: one workgroup per leaf and several; the native pointer walk
    # (every leaf a contiguous float32 device tensor) and the Python walk; a tree of no elements
    assert any(max(c["sizes"]) >= 65537 for c in cs) and any(0 < max(c["sizes"]) <= 64 for c in cs)
    assert any(set(c["placements"]) == {"own"} for c in cs)
    assert any(c["P"] == 0 and c["K"] * len(c["sizes"]) >= 2 for c in cs)
