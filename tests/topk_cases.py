"""Constructed and seeded cases for the top-k sparsified mean (no product code, no GPU), in the
layout of tests/centered_clip_cases.py. The CPU checks of this module are tests/test_topk_cases.py;
the GPU files tests/test_gpu_topk_limits.py and tests/test_gpu_topk_fuzz.py run what it makes.

``staircase(level, mult, rng)``: a float32 [256, P] slab that makes every lane of the scan the
finder, at every position of its slice. Every row holds ``mult`` keys in every bin of ``level``
(2048 bins at level 0, 1024 at levels 1 and 2; the other digits are fixed, at level 0 the lower
bits are non-zero so that bin 0 holds subnormals, not zeros, and the top bins hold inf / NaN
patterns), client ``k`` holds ``mult * k`` more keys in the top bin and ``mult * (256 - k)`` more
in the bottom bin: P = mult * (bins + 256), random signs, every row shuffled. With the keep
counts ``staircase_counts(level, mult)``, c = 256 * mult * (j + 1), client k's rank falls in bin
``bins - 1 - (256 * (j + 1) - 1 - k)``: over the bins / 256 calls every bin is the picked bin of
some client. With ``mult = 3`` the counts one and two below each are added: the rank left inside
the picked bin is then 3, 2 and 1.

``family(name, K, P, rng)``: tests/topk_ref.py's families and ``scaled``, Gaussian deltas times
``4 ** (k % 16 - 8)`` for client k: the clients of one call differ in their level-0 digit (the
exponent moves by two a client, the digit by 16), and so in every lower prefix and rank.

``limit_rows(name)``: K = 2 rows whose counts leave 16 bits: ``equal`` and ``hot_bin`` at
P = 5 * chunk + 1 = 81 921 (one bin holds every key at every level for ``equal``, at level 0 for
``hot_bin``) and ``gauss`` at P = 2**20 + 1 (65 chunks).

``layout(seed)`` draws, from the seed alone:

* K from K_CLASSES, around the fold's "client 0, then batches of eight, then a tail": 1..12,
  16..18, 24..26, 33..34; the class is ``seed % 4``;
* 1-40 leaves with sizes from SIZES (a quarter of the cases more than 16 leaves); three sizes in
  four come from the sizes up to 1025, and K * P <= MAX_ELEMENTS (the largest leaf shrinks until
  it is); at least one leaf is not empty;
* ``(seed // 8) % 4``: 0 nothing forced, 1 an empty first leaf, 2 an empty last leaf, 3 two
  adjacent empty leaves (SIZES holds 0 as well, so empties also fall where they may);
* a 0-dimensional leaf in about a quarter of the cases;
* per (client, leaf) an element offset 0..3, all zero when ``(seed // 4) % 2 == 0``;
* in about a third of the cases each: one leaf of one client a strided (non-contiguous) view,
  and one client's leaves numpy arrays on the host;
* a data family from FAMILIES; weights from WEIGHTS, not all zero; the keep count from
  ``ref.keep_counts(P)`` or uniform in [1, P].

``trees(lay)`` makes the K client dicts of a layout (leaf names sort in leaf order). A layout is
small and is kept; the data are not. Treat both as read-only.
"""
import functools

import numpy as np

from tests import topk_ref as ref

F32 = np.float32
CHUNK = 16384  # fjsparse::kChunk (tests/test_topk_cases.py holds it to the header)
LANES = 256  # fjsparse::kThreads: the lanes of the scan, and the clients of a staircase
FAMILIES = ref.FAMILIES + ("scaled",)
K_CLASSES = (tuple(range(1, 13)), (16, 17, 18), (24, 25, 26), (33, 34))
KS = [k for cls in K_CLASSES for k in cls]
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1]
SMALL = SIZES[:12]
MAX_ELEMENTS = 2 << 20
WEIGHTS = (0.0, 1.0, -1.0, 2.5, 0.125, 100.0, float(np.float32(1e-45)))  # the last: the smallest subnormal
NCASES, SEED0 = 96, 4200  # the sweep the suite runs (tests/test_topk_cases.py states what these seeds must reach)


# ------------------------------------------------------------------ staircases
STAIR_LEVELS, STAIR_MULTS = (0, 1, 2), (1, 3)
_STAIR_FIXED = {0: np.uint32(0x0002AAAA),                                  # the 20 bits under the top digit
                1: (np.uint32(0x3F8) << np.uint32(20)) | np.uint32(0x155),  # top digit of 1.0, lowest digit 0x155
                2: (np.uint32(0x3F8) << np.uint32(20)) | (np.uint32(0x12C) << np.uint32(10))}


def stair_bins(level):
    return 2048 if level == 0 else 1024


def stair_shift(level):
    return (20, 10, 0)[level]


def stair_digit(T, level):
    """The digit of key(s) T at `level` (numpy; the rule of fjsparse_dev.h restated)."""
    return (np.asarray(T, dtype=np.uint32) >> np.uint32(stair_shift(level))) & np.uint32(stair_bins(level) - 1)


def staircase(level, mult, rng):
    assert level in STAIR_LEVELS and mult in STAIR_MULTS
    nb, sh = stair_bins(level), np.uint32(stair_shift(level))
    every = np.repeat(np.arange(nb, dtype=np.uint32), mult)
    rows = []
    for k in range(LANES):
        d = np.concatenate([every, np.full(mult * k, nb - 1, np.uint32), np.zeros(mult * (LANES - k), np.uint32)])
        b = (d << sh) | _STAIR_FIXED[level] | (rng.randint(0, 2, d.size).astype(np.uint32) << np.uint32(31))
        rows.append(b[rng.permutation(d.size)])
    x = np.stack(rows).view(F32)
    assert x.shape == (LANES, mult * (nb + LANES))
    return x


def staircase_counts(level, mult):
    """The keep counts of a staircase: 256 * mult * (j + 1), and with mult = 3 one and two below."""
    out = []
    for j in range(stair_bins(level) // LANES):
        c = LANES * mult * (j + 1)
        out += [c - 2, c - 1, c] if mult == 3 else [c]
    return out


def staircase_bin(level, mult, c, k):
    """The bin client k's rank c falls in, from the construction alone (no sort)."""
    nb = stair_bins(level)
    top = mult * (1 + k)
    return nb - 1 if c <= top else max(nb - 2 - (c - top - 1) // mult, 0)


# ------------------------------------------------------------------ families
def family(name, K, P, rng):
    """A float32 [K, P] array of the named family: tests/topk_ref.py's, and `scaled`."""
    if name != "scaled":
        return ref.family(name, K, P, rng)
    x = rng.standard_normal((K, P)).astype(F32)
    scale = np.array([4.0 ** (k % 16 - 8) for k in range(K)], F32)
    return np.ascontiguousarray(x * scale[:, None], dtype=F32)


LIMIT_ROWS = {"equal": 5 * CHUNK + 1, "hot_bin": 5 * CHUNK + 1, "gauss": (1 << 20) + 1}
LIMIT_LEVELS = {"equal": (0, 1, 2), "hot_bin": (0,), "gauss": ()}  # where one bin holds more than 65 535 keys


def limit_rows(name):
    """The float32 [2, P] slab of a count-limit case."""
    return ref.family(name, 2, LIMIT_ROWS[name], np.random.RandomState(77 + sorted(LIMIT_ROWS).index(name)))


def limit_counts(P):
    return [1, 65536, 65537, P - 1, P]


# ------------------------------------------------------------------ the definition, by comparisons only
def check_definition(T, sent, rows, c, what=""):
    """Holds thresholds T (uint32 [K]) and sent (int32 [K]) to the definition on the rows
    themselves (float32 [K, P] or K flat rows): #{key > T} < c <= #{key >= T} and
    sent = #{key >= max(T, 1)}. Comparisons and counts only: nothing is sorted."""
    T = np.ascontiguousarray(T).view(np.uint32).ravel()
    sent = np.asarray(sent).ravel()
    assert len(rows) == T.size == sent.size, (what, len(rows), T.size, sent.size)
    for k, row in enumerate(rows):
        m = ref.keys(np.ravel(row))
        gt, ge = int((m > T[k]).sum()), int((m >= T[k]).sum())
        assert gt < c <= ge, (what, f"client {k}: T = {int(T[k]):#x}, #(key > T) = {gt}, c = {c}, #(key >= T) = {ge}")
        want = int((m >= max(int(T[k]), 1)).sum())
        assert int(sent[k]) == want, (what, f"client {k}: sent = {int(sent[k])}, #(key >= max(T, 1)) = {want}")


# ------------------------------------------------------------------ seeded layouts
def k_class(K):
    return next(i for i, cls in enumerate(K_CLASSES) if K in cls)


@functools.lru_cache(maxsize=None)
def layout(seed):
    rs = np.random.RandomState(seed)
    K = int(rs.choice(K_CLASSES[seed % 4]))
    span = rs.randint(4)  # a quarter of the cases have more than 16 leaves
    L = int(rs.randint(17, 38)) if span == 0 else int(rs.randint(1, 17))  # (up to three more are inserted below)
    sizes = [int(rs.choice(SMALL if rs.rand() < 0.75 else SIZES)) for _ in range(L)]
    forced = (seed // 8) % 4
    if forced == 1:
        sizes[0] = 0
    elif forced == 2:
        sizes[-1] = 0
    elif forced == 3:
        at = int(rs.randint(0, L))
        sizes[at:at] = [0, 0]
    while K * sum(sizes) > MAX_ELEMENTS:  # shrink the largest leaf
        i = int(np.argmax(sizes))
        sizes[i] = SIZES[SIZES.index(sizes[i]) - 3]
    if sum(sizes) == 0:
        live = [i for i in range(len(sizes))
                if not (forced == 1 and i == 0 or forced == 2 and i == len(sizes) - 1 or forced == 3 and i in (at, at + 1))]
        if live:
            sizes[live[int(rs.randint(len(live)))]] = int(rs.choice([1, 3, 257]))
        else:  # one leaf, and that one forced empty: a live one beside it
            sizes.insert(1 if forced == 1 else 0, int(rs.choice([1, 3, 257])))
    L, P = len(sizes), sum(sizes)
    shapes = [(n,) for n in sizes]
    ones = [i for i, n in enumerate(sizes) if n == 1]
    if ones and rs.rand() < 0.4:
        shapes[ones[int(rs.randint(len(ones)))]] = ()
    elif rs.rand() < 0.15:  # no leaf of one element: one more, 0-dimensional
        spots = [p for p in range(L + 1)  # (not where it would undo what was forced)
                 if not (forced == 1 and p == 0 or forced == 2 and p == L or forced == 3 and p == at + 1)]
        at0 = spots[int(rs.randint(len(spots)))]
        sizes.insert(at0, 1)
        shapes.insert(at0, ())
        L, P = L + 1, P + 1
    aligned = (seed // 4) % 2 == 0
    offsets = rs.randint(0, 4, size=(K, L)) * (0 if aligned else 1)
    wide = [i for i, n in enumerate(sizes) if n >= 2]
    strided = (int(rs.randint(K)), wide[int(rs.randint(len(wide)))]) if wide and rs.rand() < 0.35 else None
    host_client = int(rs.randint(K)) if rs.rand() < 0.35 else None
    name = FAMILIES[int(rs.randint(len(FAMILIES)))]
    w = [float(v) for v in rs.choice(WEIGHTS, K)]
    if not any(w):
        w[int(rs.randint(K))] = 1.0
    c = int(rs.choice(ref.keep_counts(P))) if rs.rand() < 0.5 else int(rs.randint(1, P + 1))
    names = [f"l{i:02d}" for i in range(L)]
    return dict(seed=seed, K=K, L=L, P=P, sizes=sizes, shapes=shapes, names=names, forced=forced, aligned=aligned,
                offsets=offsets, strided=strided, host_client=host_client, family=name, weights=w, c=c)


def trees(lay):
    """The K client dicts (name -> float32 array of the leaf's shape) of a layout."""
    rs = np.random.RandomState(lay["seed"] + 500009)
    K = lay["K"]
    out = [{} for _ in range(K)]
    for n, size, shape in zip(lay["names"], lay["sizes"], lay["shapes"]):
        v = family(lay["family"], K, size, rs) if size else np.zeros((K, 0), F32)
        for k in range(K):
            out[k][n] = np.array(v[k].reshape(shape), dtype=F32, order="C")  # (a copy; keeps a 0-dimensional shape)
    return out


def describe(lay):
    return (f"seed {lay['seed']} ({lay['family']} K={lay['K']} sizes={lay['sizes']} c={lay['c']}"
            f"{'' if lay['aligned'] else ' offsets'}{' strided' if lay['strided'] else ''}"
            f"{' host client' if lay['host_client'] is not None else ''})")
