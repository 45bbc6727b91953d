"""Seeded cases for the clipped and the grouped weighted mean (no product code, no GPU).

One case is K clients' deltas under one pytree structure, a placement per leaf, weights, a clip
norm and a grouping; ``case(seed)`` draws all of it from the seed alone, in the style of the
generator in tests/test_gpu_fuzz.py:

* a nested dict / list / tuple structure of 1-70 leaves, leaf sizes from SIZES (that file's
  list: empty, 1, the 4- and 8-element units, 64 / 256 lanes, 4096-element chunks, 65537),
  shapes of 0 to 3 dimensions;
* per leaf a placement: its own allocation, a view at a random element offset of a buffer the
  client's views share (4-byte aligned only), a non-contiguous view, a host numpy array, or a
  float64 array (which canonicalises to float32: the values are float32 values);
* K from KS (128 / 129 straddle the fused norm combine's client limit);
* weights: Python ints, Python floats, numpy float32 scalars, a zero total, a negative total;
* a clip norm: the median norm, below the least, above the greatest, 0, inf;
* G in [1, K + 3] groups with ids that include -1 and, with some probability each, an emptied
  group, a single-member group, a group whose weights sum to 0 and a group with a NaN weight
  (the grouped weights ``gweights`` are the weights with those edits);
* NaN / inf / -0 sprinkled into the deltas of one case in five.

``case`` keeps what it drew (the two sweeps and the generator's own test share the cases), so
treat a case as read-only; ``case.__wrapped__(seed)`` draws afresh.

``place`` realises a case as client pytrees on a torch device ("cpu" works: the CPU test checks
the placements there). ``clipped_reference`` / ``grouped_reference`` evaluate the numpy
restatements (tests/clipped_mean_ref.py, tests/grouped_mean_ref.py) for the case.
"""
import functools

import numpy as np
import torch

from tests import clipped_mean_ref as cref
from tests import grouped_mean_ref as gref

F32 = np.float32
SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
         4095, 4096, 4097, 8191, 12289, 65537]
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 128, 129, 257]
PLACEMENTS = ("own", "offset_view", "noncontig", "host", "f64")
WEIGHT_KINDS = ("int", "float", "np32", "zero", "negative")
CLIP_KINDS = ("median", "below_min", "above_max", "zero", "inf")
# what keeps a case quick (host walk and numpy restatement): elements and (client, leaf) pairs
MAX_ELEMENTS = 1_500_000
MAX_CLIENT_LEAVES = 2304


def _shape(rs, n):
    """A shape of n elements with 0 to 3 dimensions."""
    if n == 1 and rs.rand() < 0.5:
        return ()
    if n == 0 or rs.rand() < 0.4:
        return (n,)
    for d in (2, 3, 4, 5, 7, 8, 16, 31, 64):
        if n % d == 0 and rs.rand() < 0.5:
            m = n // d
            for e in (2, 3, 5, 8):
                if m % e == 0 and rs.rand() < 0.4:
                    return (d, e, m // e)
            return (d, m)
    return (n, 1) if rs.rand() < 0.2 else (n,)


def _structure(rs, nleaves):
    """A nested container of nleaves leaf slots; the slots are numbered in flatten order
    (dict keys sorted, which is not their insertion order)."""
    def build(count, depth):
        if count == 1 and (depth > 0 or rs.rand() < 0.3):
            return ["leaf", None]
        kind = rs.choice(["dict", "list", "tuple"]) if depth < 3 else "dict"
        parts = max(1, min(count, int(rs.randint(1, 5))))
        cuts = sorted(rs.choice(np.arange(1, count), size=parts - 1, replace=False)) if parts > 1 else []
        kids = [build(b - a, depth + 1) for a, b in zip([0] + list(cuts), list(cuts) + [count])]
        if kind == "dict":
            keys = ["k%02d" % v for v in rs.permutation(100)[:len(kids)]]
            return ["dict", dict(zip(keys, kids))]
        return [kind, kids]

    def number(node, nxt):
        kind, v = node
        if kind == "leaf":
            node[1] = nxt
            return nxt + 1
        for child in ([v[k] for k in sorted(v)] if kind == "dict" else v):
            nxt = number(child, nxt)
        return nxt
    root = build(nleaves, 0)
    assert number(root, 0) == nleaves
    return root


def realize(node, leaves):
    """The pytree of ``node`` with ``leaves[i]`` at slot i (slot order = flatten order)."""
    kind, v = node
    if kind == "leaf":
        return leaves[v]
    if kind == "dict":
        return {k: realize(c, leaves) for k, c in v.items()}
    kids = [realize(c, leaves) for c in v]
    return kids if kind == "list" else tuple(kids)


def _weights(rs, wkind, K):
    if wkind == "int":
        return [int(v) for v in rs.randint(1, 501, size=K)]
    if wkind == "float":
        return [float(v) for v in rs.rand(K) * 3 + 0.01]
    if wkind == "np32":
        return [F32(v) for v in rs.rand(K) * 3 + 0.01]
    ws = [int(v) for v in rs.randint(1, 501, size=K)]
    if wkind == "zero":  # +w, -w pairs (an odd client out weighs 0): groups may still have totals
        for k in range(1, K, 2):
            ws[k] = -ws[k - 1]
        if K % 2:
            ws[K - 1] = 0
        return ws
    for k in range(K):  # a negative total with some positive weights
        if rs.rand() < 0.75:
            ws[k] = -ws[k]
    return ws if sum(ws) < 0 else [-abs(w) for w in ws]


def _grouping(rs, K, weights, few):
    """(G, ids, gweights, edits): ids in {-1} | [0, G); ``edits`` names the forced edges.
    ``few``: at most 3 groups (with many clients: long member lists)."""
    G = int(rs.randint(1, min(K + 3, 6) + 1)) if rs.rand() < 0.5 else int(rs.randint(1, K + 4))
    if few:
        G = 1 + G % 3
    ids = rs.randint(0, G, size=K).astype(np.int64)
    ids[rs.rand(K) < 0.15] = -1
    gw, edits = list(weights), []
    if G >= 2 and rs.rand() < 0.35:  # an emptied group
        g = int(rs.randint(G))
        ids[ids == g] = (g + 1) % G if rs.rand() < 0.5 else -1
        edits.append("empty")
    if G >= 2 and rs.rand() < 0.35:  # exactly one member
        g, k = int(rs.randint(G)), int(rs.randint(K))
        ids[ids == g] = -1
        ids[k] = g
        edits.append("single")
    if K >= 2 and rs.rand() < 0.35:  # two members whose weights cancel
        g = int(rs.randint(G))
        a, b = (int(v) for v in rs.choice(K, size=2, replace=False))
        ids[ids == g] = -1
        ids[a] = ids[b] = g
        gw[b] = -gw[a]
        edits.append("zero_total")
    if rs.rand() < 0.25:  # a NaN weight on a member (on any client if nobody is a member)
        members = np.flatnonzero(ids >= 0)
        k = int(rs.choice(members)) if members.size else int(rs.randint(K))
        gw[k] = float("nan")
        edits.append("nan_weight")
    return G, ids, gw, edits


@functools.lru_cache(maxsize=512)
def case(seed):
    rs = np.random.RandomState(seed)
    K = int(rs.choice(KS))
    nleaves = int(rs.choice([1, 2, 3, 5, 8, 12, 40], p=[.12, .12, .12, .16, .2, .2, .08]))
    if seed % 10 == 5:  # beyond 64 leaves
        nleaves, K = 70, int(rs.choice([2, 3, 5, 9, 17]))
    elif seed % 10 == 3:  # beyond the fused combine's 128 clients
        K = int(rs.choice([128, 129, 257]))
    nleaves = max(1, min(nleaves, MAX_CLIENT_LEAVES // K))
    sizes = [int(rs.choice(SIZES)) for _ in range(nleaves)]
    if seed % 20 == 7:  # a tree of nothing but empty leaves
        sizes = [0] * nleaves
    while sum(sizes) * K > MAX_ELEMENTS:
        i = int(np.argmax(sizes))
        sizes[i] //= 3
    shapes = [_shape(rs, n) for n in sizes]
    struct = _structure(rs, nleaves)
    # one placement for the whole tree (the all-"own" tree is the common case and takes the
    # native pointer walk), or one drawn per leaf
    if rs.rand() < 0.45:
        placements = [str(rs.choice(PLACEMENTS, p=[.4, .3, .1, .1, .1]))] * nleaves
    else:
        placements = [str(p) for p in rs.choice(PLACEMENTS, size=nleaves, p=[.3, .3, .14, .13, .13])]
    gaps = [int(v) for v in rs.randint(0, 4, size=nleaves)]
    view_start = int(rs.randint(0, 4))
    P = sum(sizes)
    x = ((rs.rand(K, P) * 2 - 1) * 10.0 ** rs.randint(-3, 2, size=(K, 1))).astype(F32)
    special = seed % 5 == 2 and P > 0  # one case in five: non-finite values and -0 in the deltas
    if special:
        for v in (np.nan, np.inf, -np.inf, -0.0):
            for _ in range(int(rs.randint(0, 3))):
                x[rs.randint(K), rs.randint(P)] = v
        x[rs.randint(K), rs.randint(P)] = rs.choice([np.nan, np.inf, -np.inf])
    x.setflags(write=False)
    wkind = str(rs.choice(WEIGHT_KINDS, p=[.35, .25, .2, .1, .1]))
    weights = _weights(rs, wkind, K)
    with np.errstate(all="ignore"):
        n64 = cref.f64_norms(x)
    fin = n64[np.isfinite(n64)]
    clip_kind = str(rs.choice(CLIP_KINDS, p=[.4, .2, .2, .1, .1]))
    if clip_kind == "zero" or (fin.size == 0 and clip_kind != "inf"):
        max_norm = 0.0
    elif clip_kind == "inf":
        max_norm = float("inf")
    elif clip_kind == "median":
        max_norm = float(np.median(fin))
    elif clip_kind == "below_min":
        max_norm = 0.5 * float(fin.min())
    else:
        max_norm = 2.0 * float(fin.max()) if fin.max() > 0 else 1.0
    G, ids, gweights, edits = _grouping(rs, K, weights, few=seed % 20 == 13)
    return dict(seed=seed, K=K, P=P, sizes=sizes, shapes=shapes, struct=struct, placements=placements, gaps=gaps,
                view_start=view_start, x=x, special=special, wkind=wkind, weights=weights, clip_kind=clip_kind,
                max_norm=max_norm, G=G, ids=ids, gweights=gweights, group_edits=edits)


def template(c):
    """The case's structure with zero numpy leaves (a ClientDeltaSlab template)."""
    return realize(c["struct"], [np.zeros(s, F32) for s in c["shapes"]])


def place(c, device):
    """K client pytrees holding the rows of c["x"], every leaf placed as c["placements"] says.
    Device leaves are torch tensors on ``device``; "host" leaves are numpy float32 arrays."""
    X = torch.from_numpy(np.array(c["x"])).to(device)
    sizes, shapes, kinds = c["sizes"], c["shapes"], c["placements"]
    shared = sum(n + 4 for n, p in zip(sizes, kinds) if p == "offset_view") + 8
    trees = []
    for k in range(c["K"]):
        buf = torch.empty(shared, dtype=torch.float32, device=device)
        off, o, leaves = (c["view_start"] + k) % 4, 0, []
        for n, s, kind, gap in zip(sizes, shapes, kinds, c["gaps"]):
            seg = X[k, o:o + n]
            if kind == "own":
                leaf = seg.clone().reshape(s)
            elif kind == "offset_view":
                leaf = buf[off:off + n]
                leaf.copy_(seg)
                leaf = leaf.view(s)
                off += n + gap
            elif kind == "noncontig":  # every other element of a buffer twice as long
                b = torch.zeros(2 * n, dtype=torch.float32, device=device)
                b[::2] = seg
                leaf = b[::2].reshape(s)
                assert n <= 1 or leaf.data_ptr() == b.data_ptr()  # a view, not a copy
            elif kind == "host":
                leaf = np.array(c["x"][k, o:o + n]).reshape(s)
            else:
                leaf = seg.to(torch.float64).reshape(s)
            leaves.append(leaf)
            o += n
        trees.append(realize(c["struct"], leaves))
    return trees


def mean_scale(weights):
    """f32(1/W) if W > 0 else 0, W summed from 0.0 in client order (tree_util.py:86-96)."""
    W = 0.0
    for w in weights:
        W += w
    return F32((1.0 / W) if W > 0.0 else 0.0)


def clipped_reference(c, norms=None):
    """(factors, mean [P]) of the restatement, from ``norms`` (float32 [K]; default: the
    float64 norms rounded to float32)."""
    x = c["x"]
    with np.errstate(all="ignore"):
        if norms is None:
            norms = cref.f64_norms(x).astype(F32)
        fac = cref.clip_factors_ref(norms, c["max_norm"])
        w32 = np.array([F32(w) for w in c["weights"]], dtype=F32)
        return fac, cref.clipped_fold_ref(x, w32, fac, mean_scale(c["weights"]))


def grouped_reference(c):
    """The restatement's list of G means ([P] float32, or None)."""
    return gref.grouped_mean_ref(c["x"], c["gweights"], c["ids"], c["G"])
