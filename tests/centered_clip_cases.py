"""Seeded cases for centered clipping (no product code, no GPU), in the layout of
tests/clip_group_cases.py. ``case(seed)`` draws everything from the seed alone:

* K from KS: 1..12, 63..66 and 127..130 (around the fold's four clients in flight at larger
  counts) and 257; the class is ``seed % 4``, except that a case with a two-block leaf
  (``seed % 3 == 0``) keeps K <= 63 so that K x P stays within MAX_ELEMENTS;
* 1-9 leaves with sizes from SIZES (empty, 1..5, around 256 lanes, around the 2048 elements a
  lane block keeps in flight, around the fold's 8192-element workgroup, 65535 and 65537: under
  and over one 64 Ki-element norm block); at least one leaf is not empty (rounds of nothing but
  empty leaves are tests/test_gpu_centered_clip_limits.py's);
* a 0-3 element offset per (client, leaf) allocation (all 0 when ``seed % 2 == 0``: aligned
  deltas) and, separately, per centre leaf (all 0 when ``seed % 8 == 6``);
* 1-4 iterations; in place or into a fresh output;
* tau: "median" (of the finite distances from the first centre), "huge" (1e30), "tiny" (1e-3 of
  the smallest distance) or "boundary" (exactly one client's restated distance over the case's
  own leaf cut, so that client's first factor is exactly 1);
* client k's deltas are the centre plus N(0, 1) at a scale of its own; in a case with specials
  (``(seed // 2) % 2 == 1`` and K >= 3) up to K - 2 clients have 3 % of their elements replaced by
  +-0, NaN, +-inf or 1e30 (two clients at least stay finite: the median is of real numbers); the
  centre has +0 and -0 entries.

``case`` keeps what it drew; treat a case as read-only. ``reference(c, cut)`` evaluates the closed
restatement (tests/centered_clip_ref.py) for the case's rows cut into leaves of ``cut``.
"""
import functools

import numpy as np

from tests import centered_clip_ref as ref

F32 = np.float32
K_CLASSES = (tuple(range(1, 13)), (63, 64, 65, 66), (127, 128, 129, 130), (257,))
KS = [k for cls in K_CLASSES for k in cls]
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 65535, 65537]
TAU_KINDS = ("median", "huge", "tiny", "boundary")
MAX_ELEMENTS = 4 << 20
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e30], dtype=F32)
NCASES, SEED0 = 48, 7000  # the sweep the suite runs


def k_class(K):
    return next(i for i, cls in enumerate(K_CLASSES) if K in cls)


@functools.lru_cache(maxsize=256)
def case(seed):
    rs = np.random.RandomState(seed)
    two_blocks = seed % 3 == 0
    tau_kind = TAU_KINDS[int(rs.randint(4))] if seed % 2 else TAU_KINDS[(seed // 2) % 4]
    K = int(rs.choice(K_CLASSES[seed % 4]))
    if two_blocks:
        K = int(rs.choice(list(K_CLASSES[0]) + [63]))
    if tau_kind == "median" and K == 1:
        K = 2
    nleaves = int(rs.randint(1, 10))
    sizes = [int(rs.choice(SIZES)) for _ in range(nleaves)]
    if two_blocks:
        sizes[int(rs.randint(nleaves))] = 65537
    while sum(sizes) * K > MAX_ELEMENTS:  # shrink the largest leaf that may shrink
        order = sorted(range(nleaves), key=lambda i: -sizes[i])
        i = next(j for j in order if not (two_blocks and sizes[j] == 65537 and sizes.count(65537) == 1))
        sizes[i] = SIZES[max(SIZES.index(sizes[i]) - 3, 0)]
    if sum(sizes) == 0:
        sizes[int(rs.randint(nleaves))] = int(rs.choice([1, 3, 257]))
    P = sum(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    iterations = 1 + (seed // 4) % 4
    in_place = bool(rs.randint(2))
    delta_offsets = rs.randint(0, 4, size=(K, nleaves)) * (seed % 2)
    centre_offsets = rs.randint(0, 4, size=nleaves) * int(seed % 8 != 6)
    dense_offset, dense_pad = int(rs.randint(0, 4)) * (seed % 2), int(rs.randint(0, 4))
    v = (0.5 * rs.standard_normal(P)).astype(F32)
    zero = rs.rand(P) < 0.1
    v[zero] = np.where(rs.rand(int(zero.sum())) < 0.5, F32(0.0), F32(-0.0))
    scale = (0.25 * 2.0 ** (3.0 * rs.permutation(K) / K)).astype(F32)  # distinct, within a factor of 8
    x = (v + rs.standard_normal((K, P)).astype(F32) * scale[:, None]).astype(F32)
    special_rows = []
    if (seed // 2) % 2 == 1 and K >= 3:
        special_rows = [int(k) for k in np.flatnonzero(rs.rand(K) < 0.3)][:K - 2] or [int(rs.randint(K))]
        for k in special_rows:
            hit = rs.rand(P) < 0.03
            x[k, hit] = SPECIALS[rs.randint(0, len(SPECIALS), int(hit.sum()))]
            x[k, int(rs.randint(P))] = SPECIALS[int(rs.randint(2, len(SPECIALS)))]  # one that is not a zero
    with np.errstate(all="ignore"):
        d64 = ref.centered_distances_f64(x, v)
        fin = d64[np.isfinite(d64) & (d64 * d64 < 3e38)]
    assert fin.size >= min(K, 2)
    if tau_kind == "median":
        tau = float(np.median(fin))
    elif tau_kind == "huge":
        tau = 1e30
    elif tau_kind == "tiny":
        tau = 1e-3 * float(fin.min())
    else:
        d32 = ref.centered_distances_ref(x, v, sizes)
        usable = np.flatnonzero(np.isfinite(d32) & (d32 > 0))
        tau = float(np.sort(d32[usable])[(usable.size - 1) // 2])  # the lower median: any farther client clips
    x.setflags(write=False)
    v.setflags(write=False)
    return dict(seed=seed, K=K, P=P, sizes=sizes, offs=offs, iterations=iterations, in_place=in_place,
                delta_offsets=delta_offsets, centre_offsets=centre_offsets, dense_offset=dense_offset,
                dense_pad=dense_pad, x=x, v=v, special=bool(special_rows), special_rows=special_rows,
                tau_kind=tau_kind, tau=tau, _refs={})


def reference(c, cut=None):
    """(centre, distances, factors) of the closed restatement over the leaf cut ``cut`` (default:
    the case's own leaves), kept on the case."""
    cut = tuple(c["sizes"] if cut is None else cut)
    if cut not in c["_refs"]:
        c["_refs"][cut] = ref.centered_clip_ref(c["x"], c["v"], c["tau"], c["iterations"], sizes=list(cut))
    return c["_refs"][cut]


def describe(c):
    return (f"seed {c['seed']} (K={c['K']} sizes={c['sizes']} L={c['iterations']} tau={c['tau_kind']} "
            f"{'in place' if c['in_place'] else 'fresh'}{' specials' if c['special'] else ''})")
