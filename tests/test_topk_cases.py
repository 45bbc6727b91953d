"""The constructed and seeded top-k cases (tests/topk_cases.py) checked without a GPU, on the numpy
restatement (tests/topk_ref.py) and the host build of the select rules (tests/topk_select_host.cpp).
It pins what keeps tests/test_gpu_topk_limits.py and tests/test_gpu_topk_fuzz.py from being hollow:

* the staircases do what they are for: over their keep counts every bin of the level is the picked
  bin of some client, every (lane, position in its slice) pair of the scan occurs, lane 0 and lane
  255 included, with ``mult = 3`` the rank left inside the picked bin takes 1, 2 and 3, and the host
  program (one slice, and the device's 256 lane slices) agrees with numpy on every one of them;
* the count-limit rows hold more than 65 535 keys in one bin where they say they do;
* the layouts are a function of the seed, and the committed seeds reach every K class, the empty
  first / last / adjacent leaves, a 0-dimensional leaf, more than 16 leaves, a leaf of more than one
  chunk, misaligned and all-aligned cases, a strided leaf, a host client and every family, each
  with a stated floor;
* the definition check refuses a threshold one off in either direction and a wrong count."""
import os
import re

import numpy as np
import pytest

from tests import topk_cases as tc
from tests import topk_host
from tests import topk_ref as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAIRS = [(level, mult) for level in tc.STAIR_LEVELS for mult in tc.STAIR_MULTS]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = topk_host.compiler()
    assert cxx is not None, "the staircase conditions need a C++ compiler"
    return topk_host.build_host_program(cxx, tmp_path_factory.mktemp("topk_cases"))


def _layouts():
    return [tc.layout(tc.SEED0 + s) for s in range(tc.NCASES)]


# ------------------------------------------------------------------ constants
def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "fedjax_amd", "csrc", "fjsparse_dev.h")).read()
    consts = dict(re.findall(r"constexpr int (k\w+) = (\d+);", src))
    assert int(consts["kChunk"]) == tc.CHUNK and int(consts["kThreads"]) == tc.LANES
    assert int(consts["kMaxBins"]) == tc.stair_bins(0) and tc.stair_bins(1) == tc.stair_bins(2) == 1024


# ------------------------------------------------------------------ staircases
@pytest.mark.parametrize("level,mult", STAIRS)
def test_staircase_makes_every_lane_the_finder_at_every_position(host_program, tmp_path, level, mult):
    nb = tc.stair_bins(level)
    per = nb // tc.LANES
    x = tc.staircase(level, mult, np.random.RandomState(100 + 10 * level + mult))
    assert x.dtype == F32 and x.shape == (256, {0: 2304, 1: 1280, 2: 1280}[level] * mult)
    m = ref.keys(x)
    for k in (0, 1, 200, 255):  # mult keys in every bin, the extra ones in the top and the bottom bin
        want = np.full(nb, mult)
        want[nb - 1] += mult * k
        want[0] += mult * (256 - k)
        assert np.bincount(tc.stair_digit(m[k], level), minlength=nb).tolist() == want.tolist()
    others = m & ~np.uint32((nb - 1) << tc.stair_shift(level))
    assert len(np.unique(others)) == 1, "the other digits are fixed"
    if level == 0:
        assert others[0, 0] != 0 and not (m == 0).any(), "bin 0 holds subnormals, not zeros"
        assert (m[tc.stair_digit(m, 0) >= nb - per] > 0x7F800000).all(), "lane 0's bins are NaN patterns"
    else:
        assert 0x00800000 <= (int(others[0, 0]) & ~0xFFFFF) < 0x7F800000, "a normal-number prefix"
    assert np.signbit(x).any() and not np.signbit(x).all()
    assert not (np.sort(m, axis=1) == m).all(), "shuffled"

    cs = tc.staircase_counts(level, mult)
    assert len(cs) == per * (3 if mult == 3 else 1) and set(256 * mult * (j + 1) for j in range(per)) <= set(cs)
    want = ref.select_many(list(x), cs)
    picked, pairs = set(), set()
    for c in cs:
        d = tc.stair_digit(want[c][0], level)
        assert d.tolist() == [tc.staircase_bin(level, mult, c, k) for k in range(256)], (c, "the construction's own bins")
        picked |= set(d.tolist())
        # lane t owns the per bins below nb - 1 - t * per
        pairs |= {((nb - 1 - int(b)) // per, (nb - 1 - int(b)) % per) for b in d}
    assert picked == set(range(nb)), "every bin of the level is the picked bin of some client"
    assert pairs == {(t, j) for t in range(256) for j in range(per)}, "every lane finds, at every position of its slice"

    cases = [(x[k], c) for c in cs for k in range(256)]
    got = topk_host.run_host(host_program, cases, tmp_path)
    ranks = set()
    for i, ((row, c), (T, sent, trace)) in enumerate(zip(cases, got)):
        k = i % 256
        assert (T, sent) == (int(want[c][0][k]), int(want[c][1][k])), (c, k, hex(T), hex(int(want[c][0][k])))
        assert trace[2 * level] == tc.staircase_bin(level, mult, c, k)
        ranks.add(trace[2 * level + 1])
    if mult == 3:
        assert {1, 2, 3} <= ranks, "the rank left inside the picked bin: first, middle, last"
    else:
        assert 1 in ranks
    for c in cs:
        tc.check_definition(want[c][0], want[c][1], x, c, f"staircase {level} x{mult} c={c}")


# ------------------------------------------------------------------ count limits and families
@pytest.mark.parametrize("name", sorted(tc.LIMIT_ROWS))
def test_limit_rows_leave_sixteen_bits(name):
    x = tc.limit_rows(name)
    P = tc.LIMIT_ROWS[name]
    assert x.shape == (2, P) and x.dtype == F32
    assert P == (5 * tc.CHUNK + 1 if name != "gauss" else 2 ** 20 + 1) and -(-P // tc.CHUNK) == (6 if name != "gauss" else 65)
    assert tc.limit_counts(P) == [1, 65536, 65537, P - 1, P] and P - 1 > 65537
    for k in range(2):
        m = ref.keys(x[k])
        T = ref.threshold(x[k], 65537)  # a keep count the GPU test uses
        for level in tc.LIMIT_LEVELS[name]:
            # the histogram of this level: the keys whose higher digits are the threshold's
            above = np.uint32(tc.stair_shift(level) + 10)
            under = m[(m >> above) == (T >> above)] if level else m
            most = int(np.bincount(tc.stair_digit(under, level)).max())
            assert most > 65535, (name, k, level, most)
    assert np.array_equal(tc.limit_rows(name).view(np.uint32), x.view(np.uint32))  # a function of the name


def test_scaled_clients_differ_in_the_top_digit():
    x = tc.family("scaled", 16, 257, np.random.RandomState(1))
    for c in ref.keep_counts(257):
        T, _ = ref.select(list(x), c)
        assert len(set(tc.stair_digit(T, 0).tolist())) >= 8, c
    y = tc.family("gauss", 3, 40, np.random.RandomState(2))
    assert np.array_equal(y, ref.family("gauss", 3, 40, np.random.RandomState(2)))


# ------------------------------------------------------------------ the definition check has teeth
def test_definition_check_refuses_what_is_wrong():
    rng = np.random.RandomState(4)
    for name in ("gauss", "five", "signed_zero", "nan_inf"):
        x = ref.family(name, 3, 300, rng)
        for c in (1, 30, 200, 299, 300):
            T, sent = ref.select(list(x), c)
            tc.check_definition(T, sent, x, c)
            tc.check_definition(T.view(F32), sent, x, c)  # thresholds as the float32 the device returns
            for k in range(3):
                present = np.unique(ref.keys(x[k]))
                at = int(np.searchsorted(present, T[k]))
                for other in ([present[at + 1]] if at + 1 < present.size else []) + ([present[at - 1]] if at else []):
                    bad = T.copy()
                    bad[k] = other  # the next key present above, or below: the rank leaves it
                    with pytest.raises(AssertionError):
                        tc.check_definition(bad, sent, x, c)
                off = sent.copy()
                off[k] += 1
                with pytest.raises(AssertionError):
                    tc.check_definition(T, off, x, c)
    z = np.zeros((1, 9), F32)
    z[0, :4] = [1.0, -2.0, 3.0, -0.0]
    tc.check_definition(np.zeros(1, np.uint32), np.array([3], np.int32), z, 7)  # T = 0: zeros are never sent
    with pytest.raises(AssertionError):
        tc.check_definition(np.zeros(1, np.uint32), np.array([9], np.int32), z, 7)


# ------------------------------------------------------------------ the seeded layouts
def _same(a, b):
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return type(a) is type(b) and np.array(a).tobytes() == np.array(b).tobytes()
    return type(a) is type(b) and a == b


def test_defaults_agree_with_the_gpu_files():
    here = os.path.dirname(os.path.abspath(__file__))
    fuzz = open(os.path.join(here, "test_gpu_topk_fuzz.py")).read()
    limits = open(os.path.join(here, "test_gpu_topk_limits.py")).read()
    assert "tc.NCASES" in fuzz and "tc.SEED0" in fuzz
    for src in (fuzz, limits):
        assert "skip" not in src and "xfail" not in src
    assert "tc.check_definition(" in limits and "checked_select(" in limits and "checked_select(" in fuzz
    assert tc.NCASES >= 96


def test_generator_is_deterministic_per_seed():
    for s in (0, 1, 6, 11, 40):
        a, b = tc.layout.__wrapped__(tc.SEED0 + s), tc.layout.__wrapped__(tc.SEED0 + s)
        assert a is not b and _same(a, b), s
        assert not _same(a, tc.layout.__wrapped__(tc.SEED0 + s + 1))
    np.random.seed(1)  # no global random state
    assert _same(tc.layout.__wrapped__(tc.SEED0), tc.layout(tc.SEED0))
    small = next(lay for lay in _layouts() if lay["K"] * lay["P"] < 50000)
    np.random.seed(2)
    a = tc.trees(small)
    np.random.seed(3)
    assert _same(a, tc.trees(small))


def test_layouts_are_well_formed():
    for lay in _layouts():
        K, L, P, sizes, shapes = lay["K"], lay["L"], lay["P"], lay["sizes"], lay["shapes"]
        assert K in tc.KS and tc.k_class(K) == lay["seed"] % 4
        assert 1 <= L == len(sizes) == len(shapes) == len(lay["names"]) <= 40 and set(sizes) <= set(tc.SIZES)
        assert 1 <= P == sum(sizes) and K * P <= tc.MAX_ELEMENTS
        assert all(s in ((n,), ()) and int(np.prod(s)) == n for s, n in zip(shapes, sizes))
        assert sum(s == () for s in shapes) <= 1 and lay["names"] == sorted(lay["names"])
        assert lay["offsets"].shape == (K, L) and 0 <= lay["offsets"].min() and lay["offsets"].max() <= 3
        assert lay["aligned"] == ((lay["seed"] // 4) % 2 == 0) and not (lay["aligned"] and lay["offsets"].any())
        assert 1 <= lay["c"] <= P and lay["family"] in tc.FAMILIES
        assert len(lay["weights"]) == K and any(lay["weights"]) and set(lay["weights"]) <= set(tc.WEIGHTS)
        if lay["strided"]:
            k, l = lay["strided"]
            assert 0 <= k < K and sizes[l] >= 2
        assert lay["host_client"] is None or 0 <= lay["host_client"] < K
        assert lay["forced"] != 1 or sizes[0] == 0
        assert lay["forced"] != 2 or sizes[-1] == 0
        assert lay["forced"] != 3 or any(a == b == 0 for a, b in zip(sizes, sizes[1:]))
    lay = next(lay for lay in _layouts() if lay["K"] * lay["P"] < 50000 and () in lay["shapes"])
    t = tc.trees(lay)
    assert len(t) == lay["K"] and all(list(c) == lay["names"] for c in t)
    assert all(c[n].shape == s and c[n].dtype == F32 for c in t for n, s in zip(lay["names"], lay["shapes"]))


def test_default_seeds_keep_the_sweep_from_being_hollow():
    """Floors the committed seeds meet (NCASES = 96; the shares are those of topk_cases.layout):
    every K class 24 times (seed % 4), each forced placement of empty leaves 24 times
    ((seed // 8) % 4), aligned and misaligned 48 each; the drawn properties at about half
    their expected count."""
    ls = _layouts()
    n = len(ls)
    assert n == tc.NCASES
    for cls in range(4):
        assert sum(tc.k_class(lay["K"]) == cls for lay in ls) == n // 4, "every K class"
    assert {lay["K"] for lay in ls} >= {1, 9, 10, 16, 17, 18, 24, 25, 26, 33, 34}, "the fold's batch edges"
    assert sum(lay["sizes"][0] == 0 for lay in ls) >= n // 4, "an empty first leaf"
    assert sum(lay["sizes"][-1] == 0 for lay in ls) >= n // 4, "an empty last leaf"
    assert sum(any(a == b == 0 for a, b in zip(lay["sizes"], lay["sizes"][1:])) for lay in ls) >= n // 4, "adjacent empties"
    assert sum(() in lay["shapes"] for lay in ls) >= n // 8, "a 0-dimensional leaf"
    assert sum(lay["L"] > 16 for lay in ls) >= n // 8, "more than 16 leaves"
    assert max(lay["L"] for lay in ls) >= 30
    assert sum(max(lay["sizes"]) > tc.CHUNK for lay in ls) >= n // 8, "a leaf of more than one chunk"
    assert sum(lay["aligned"] for lay in ls) == n // 2 and sum(bool(lay["offsets"].any()) for lay in ls) >= n // 2 - 4
    assert sum(lay["strided"] is not None for lay in ls) >= n // 6, "a strided leaf"
    assert sum(lay["host_client"] is not None for lay in ls) >= n // 6, "a host client"
    assert any(lay["host_client"] == 0 for lay in ls) and any(lay["host_client"] not in (None, 0) for lay in ls)
    for name in tc.FAMILIES:
        assert sum(lay["family"] == name for lay in ls) >= 3, name
    assert sum(lay["c"] in ref.keep_counts(lay["P"]) for lay in ls) >= n // 3
    assert sum(lay["c"] not in ref.keep_counts(lay["P"]) for lay in ls) >= n // 4
    assert sum(0.0 in lay["weights"] for lay in ls) >= n // 3 and sum(-1.0 in lay["weights"] for lay in ls) >= n // 3
    assert sum(tc.WEIGHTS[-1] in lay["weights"] for lay in ls) >= n // 3, "a subnormal weight"
