"""Seeded cases for the compression aggregators (no product code, no GPU).

One case is K clients' deltas under one pytree structure, a placement per leaf, weights, an
aggregator kind with its parameters and a key; ``case(seed)`` draws all of it from the seed
alone, in the style of tests/clip_group_cases.py (whose structure, shape and realisation
helpers it shares):

* a nested dict / list / tuple structure of 1-24 leaves, leaf sizes from SIZES (1 to 3 elements,
  the 4-element quad, 32-bit sign words, 64 / 256 lanes, the 8192-element Walsh-Hadamard tile,
  the 16384-element statistics chunk, 65537), shapes of 0 to 3 dimensions; one case in three
  starts (in flatten order) with a leaf of 1, 2 or 3 elements, which takes every later leaf of
  the rotated and the DRIVE workspaces off 16-byte alignment;
* per leaf a placement: its own allocation, a view at a random element offset of a buffer the
  client's views share (4-byte aligned only), a non-contiguous view, a host numpy array, or an
  int32 tensor (integer values below 2^23 in magnitude);
* K from KS (kQGroup = 4 clients a load group, the 2 x 4 double-buffer tail, 256 clients staged
  at a time); the class of K rotates with the seed so that every aggregator meets every class;
* an aggregator kind (KINDS, rotating with the seed); for the uniform kinds num_levels from
  LEVELS (both sides of the 4096-entry level table and of the 4096-bin LDS histogram, whose
  group of clients per flush is 4096 // (num_levels + 1));
* weights: Python ints, Python floats, numpy float32 scalars, one zero weight among positive
  ones, a zero total (+w / -w pairs);
* for ``rotated`` / ``drive`` a ``workspace_bytes`` that gives batches of B clients, B from
  None (everything) or {1, 2, 3, K - 1, K} clipped to [1, K]: ``batch`` is B, ``workspace_bytes``
  is B times the per-client size the product uses (4 D, or 4 (D + Pp));
* values: normal deltas at scale 0.01; one case in four also has some of SPECIALS.

Budget: K * P <= MAX_ELEMENTS and K * L <= MAX_CLIENT_LEAVES. Cases of the 255..260 class are
drawn small enough to fit (at most 4 leaves, one of them above 513 elements); every other case
shrinks K first (down KS) and then its largest leaves.

Order-independence guard. terngrad's sigma and DRIVE's f32(sum y^2), f32(sum |y|) are float64
reductions rounded once to float32; the kernels sum in another order than the oracle. A case is
kept only if, for every (round, client, leaf), those float32 results have the same bits under
three summation orders (forward, reversed, numpy's pairwise) and, for sigma, as a two-pass
float64 std as well (the kernel shifts the data by its first element before it sums, the oracle
does not; both are float64 evaluations of the same number): ``order_sensitive(case)`` lists the
leaves where they do not, and ``case`` redraws such a leaf's values (deterministically from the
seed) until the list is empty. That is what makes "bitwise" a fair bar for those two kinds.

``case`` keeps what it drew, so treat a case as read-only; ``case.__wrapped__(seed)`` draws
afresh. ``place`` realises a case as client pytrees on a torch device ("cpu" works).
``reference`` runs the matching oracle aggregator (oracle/compression_ref.py) for two rounds.
"""
import functools

import numpy as np
import torch

from oracle import compression_ref as cref
from oracle import jax_random_ref as jr
from tests.clip_group_cases import _shape, _structure, realize

F32 = np.float32
SIZES = [1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 4095, 4096, 4097, 8191, 8192, 8193,
         16385, 65537]
KS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 255, 256, 257, 260]
K_CLASSES = ([1, 2, 3], [4, 5, 7, 8, 9, 12, 13], [255, 256, 257, 260])
KINDS = ("uniform", "uniform_arith", "rotated", "drive", "terngrad")
LEVELS = [2, 3, 5, 16, 255, 256, 257, 1366, 2047, 2048, 4095, 4097]
PLACEMENTS = ("own", "offset_view", "noncontig", "host", "int32")
WEIGHT_KINDS = ("int", "float", "np32", "one_zero", "zero_total")
BATCHES = (None, 1, 2, 3, "K-1", "K")
SPECIALS = ("nan", "pinf", "ninf", "negzero", "subnormal", "zero_client", "zero_all", "const", "offset_mean")
ROUNDS = 2
ROTATED_LEVELS = 4  # num_levels of the ``rotated`` kind
# what keeps a case quick (the numpy oracle and its threefry draws): elements and (client, leaf) pairs
MAX_ELEMENTS = 1_500_000
MAX_CLIENT_LEAVES = 2304
INT_BOUND = 1 << 23  # int32 leaves: |v| < 2^23, so every difference of two values is exact in float32


def k_class(K):
    return next(i for i, ks in enumerate(K_CLASSES) if K in ks)


def padded(n):
    return 1 << (int(n) - 1).bit_length()


def per_client_bytes(kind, sizes):
    """Bytes of workspace a client takes: the rotated leaves (rotated), or those and the
    inverse-rotated delta padded to a multiple of 4 (drive); fedjax_amd/_compress.py."""
    D = sum(padded(n) for n in sizes)
    P = sum(sizes)
    return 4 * D if kind == "rotated" else 4 * (D + (P + 3) // 4 * 4)


def _weights(rs, wkind, K):
    if wkind == "float":
        return [float(v) for v in rs.rand(K) * 3 + 0.01]
    if wkind == "np32":
        return [F32(v) for v in rs.rand(K) * 3 + 0.01]
    ws = [int(v) for v in rs.randint(1, 501, size=K)]
    if wkind == "one_zero" and K > 1:
        ws[int(rs.randint(K))] = 0
    if wkind == "zero_total":  # +w, -w pairs; an odd client out weighs 0
        for k in range(1, K, 2):
            ws[k] = -ws[k - 1]
        if K % 2:
            ws[K - 1] = 0
    return ws


def _leaf_values(seed, k, l, attempt, n, mode):
    """Client k's values of leaf l (float32 [n]); ``attempt`` > 0 is a redraw of the guard."""
    rs = np.random.RandomState([seed & 0x7FFFFFFF, k, l, attempt])
    if mode == "int32":
        return rs.randint(-INT_BOUND + 1, INT_BOUND, size=n).astype(F32)
    v = (rs.standard_normal(n) * 0.01).astype(F32)
    if mode == "offset_mean":  # mean / sigma of about 1e3
        v = (v + F32(10.0)).astype(F32)
    return v


def _patch(x, offs, patches):
    """Write the special values ``patches`` = [(kind, client or None, leaf, index, value)] into x:
    whole leaves first (index None), then single elements, so that none hides another."""
    for kind, k, l, idx, val in sorted(patches, key=lambda p: p[3] is not None):
        rows = slice(None) if k is None else k
        if idx is None:
            x[rows, offs[l]:offs[l + 1]] = val
        else:
            x[rows, offs[l] + idx] = val


def _sum3(v):
    """The float64 sum of v in three orders: forward, reversed, numpy's pairwise."""
    v = np.ascontiguousarray(v, np.float64)
    if v.size == 0:
        return 0.0, 0.0, 0.0
    return float(np.cumsum(v)[-1]), float(np.cumsum(v[::-1])[-1]), float(v.sum())


def _same_bits(vals):
    a = np.array(vals, F32)
    return bool(np.isnan(a).all() or (a.view(np.uint32) == a.view(np.uint32)[0]).all())


def _sigma_orders(v):
    """terngrad's float32 sigma (oracle/compression_ref.py std_f32) under the three orders, and
    as a two-pass float64 std: the kernel sums x - x[0], which takes the cancellation out of the
    one-pass formula, so where one-pass and two-pass round apart it may side with either."""
    v = np.asarray(v, np.float64).ravel()
    out = []
    with np.errstate(all="ignore"):
        for s1, s2 in zip(_sum3(v), _sum3(v * v)):
            mean = s1 / v.size
            var = max(s2 / v.size - mean * mean, 0.0)
            out.append(F32(np.sqrt(var)) if np.isfinite(var) else F32(np.nan))
        var = float(np.mean((v - np.mean(v)) ** 2))
        out.append(F32(np.sqrt(var)) if np.isfinite(var) else F32(np.nan))
    return out


def client_keys(c, rnd_rng):
    """The K client keys of the round whose aggregator state holds ``rnd_rng`` (the key chain of
    oracle/compression_ref.py's aggregators) and the next round's state key."""
    if c["kind"] == "rotated":
        rng2, _ = jr.split(rnd_rng)
        rng2, use = jr.split(rng2)
    else:
        rng2, use = jr.split(rnd_rng)
    seq = jr.PRNGSequence(use)
    return [next(seq) for _ in range(c["K"])], rng2


def order_sensitive(c, only=None):
    """[(round, client, leaf)] whose float32 reduction results depend on the summation order
    (terngrad: sigma; drive: the two sums of the rotated leaf). Empty for the other kinds.
    ``only``: a set of (client, leaf) to look at."""
    kind, x, offs = c["kind"], c["x"], c["offs"]
    K, L = c["K"], len(c["sizes"])
    bad = []
    if kind == "terngrad":
        for k in range(K):
            for l in range(L):
                if only is not None and (k, l) not in only:
                    continue
                if not _same_bits(_sigma_orders(x[k, offs[l]:offs[l + 1]])):
                    bad.append((0, k, l))
    elif kind == "drive":
        rng = c["key"]
        for r in range(ROUNDS):
            keys, rng = client_keys(c, rng)
            for k in range(K):
                lkeys = jr.split(keys[k], L)
                for l in range(L):
                    if only is not None and (k, l) not in only:
                        continue
                    with np.errstate(all="ignore"):
                        y = cref.structured_rotation(x[k, offs[l]:offs[l + 1]], lkeys[l])[0].astype(np.float64)
                        if not (_same_bits(_sum3(y * y)) and _same_bits(_sum3(np.abs(y)))):
                            bad.append((r, k, l))
    return bad


@functools.lru_cache(maxsize=64)
def case(seed):
    rs = np.random.RandomState(seed)
    kind = KINDS[seed % 5]
    kc = (seed // 5) % 3
    K = int(rs.choice(K_CLASSES[kc]))
    nleaves = int(rs.choice([1, 2, 3, 5, 8, 12, 24], p=[.1, .12, .14, .2, .2, .14, .1]))
    if kc == 2:  # drawn to fit the budget: K stays in its class
        nleaves = min(nleaves, 4)
        sizes = [int(rs.choice(SIZES[:18])) for _ in range(nleaves)]
        if rs.rand() < 0.6:
            sizes[int(rs.randint(nleaves))] = int(rs.choice([4095, 4096, 4097]))
    else:
        sizes = [int(rs.choice(SIZES)) for _ in range(nleaves)]
    if seed % 3 == 0:
        sizes[0] = int(rs.choice([1, 2, 3]))
    while K * len(sizes) > MAX_CLIENT_LEAVES or K * sum(sizes) > MAX_ELEMENTS:
        if K > 1:  # K first
            K = KS[KS.index(K) - 1]
        else:
            i = int(np.argmax(sizes))
            sizes[i] = SIZES[SIZES.index(sizes[i]) - 1]
    L = len(sizes)
    shapes = [_shape(rs, n) for n in sizes]
    struct = _structure(rs, L)
    if rs.rand() < 0.35:  # the all-"own" tree takes the native pointer walk
        placements = ["own"] * L
    else:
        placements = [str(p) for p in rs.choice(PLACEMENTS, size=L, p=[.3, .3, .14, .13, .13])]
    gaps = [int(v) for v in rs.randint(0, 4, size=L)]
    view_start = int(rs.randint(1, 4))  # client 0's first offset view is off 16-byte alignment
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P = int(offs[-1])
    # special values (one case in four); they go to float leaves
    special, patches, modes = [], [], ["int32" if p == "int32" else "normal" for p in placements]
    if seed % 4 == 1:
        q = seed // 4
        special = sorted({SPECIALS[q % 9], SPECIALS[(q + 4) % 9], str(rs.choice(SPECIALS))})
        for sk in special:
            l = int(rs.randint(L))
            if placements[l] == "int32":
                placements[l] = "own"
            k, i = int(rs.randint(K)), int(rs.randint(sizes[l]))
            if sk == "offset_mean":
                modes[l] = "offset_mean"
                continue
            modes[l] = "normal" if modes[l] == "int32" else modes[l]
            if sk == "zero_client":
                patches.append((sk, k, l, None, F32(0.0)))
            elif sk == "zero_all":
                patches.append((sk, None, l, None, F32(0.0)))
            elif sk == "const":  # k / 16: every float64 partial sum of x, x^2, |x| is exact
                patches.append((sk, None, l, None, F32(int(rs.randint(-40, 41)) / 16.0)))
            else:
                val = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf, "negzero": -0.0,
                       "subnormal": float(np.float32(1e-41))}[sk]
                patches.append((sk, k, l, i, F32(val)))
    attempts = np.zeros((K, L), dtype=np.int64)
    x = np.empty((K, P), dtype=F32)
    for k in range(K):
        for l in range(L):
            x[k, offs[l]:offs[l + 1]] = _leaf_values(seed, k, l, 0, sizes[l], modes[l])
    _patch(x, offs, patches)
    wkind = WEIGHT_KINDS[(seed // 3) % 5]
    weights = _weights(rs, wkind, K)
    num_levels = LEVELS[(2 * (seed // 5) + seed % 5) % len(LEVELS)] if kind.startswith("uniform") else None
    batch, workspace_bytes = None, None
    if kind in ("rotated", "drive"):
        b = BATCHES[(seed // 5 + seed % 5) % len(BATCHES)]
        if b is not None:
            batch = max(1, min(K, {"K-1": K - 1, "K": K}.get(b, b)))
            workspace_bytes = batch * per_client_bytes(kind, sizes)
    c = dict(seed=seed, kind=kind, K=K, P=P, sizes=sizes, shapes=shapes, offs=offs, struct=struct,
             placements=placements, gaps=gaps, view_start=view_start, x=x, special=special, patches=patches,
             modes=modes, wkind=wkind, weights=weights, num_levels=num_levels, batch=batch,
             workspace_bytes=workspace_bytes, key=jr.prng_key(seed), redraws=0)
    # the order-independence guard: redraw what depends on the summation order
    bad = order_sensitive(c)
    while bad:
        todo = {(k, l) for _, k, l in bad}
        for k, l in sorted(todo):
            attempts[k, l] += 1
            assert attempts[k, l] < 50, (seed, k, l)
            x[k, offs[l]:offs[l + 1]] = _leaf_values(seed, k, l, int(attempts[k, l]), sizes[l], modes[l])
            c["redraws"] += 1
        _patch(x, offs, patches)
        bad = order_sensitive(c, only=todo)
    x.setflags(write=False)
    return c


def client_leaves(c, k):
    """Client k's leaves as float32 numpy arrays in flatten order."""
    return [np.array(c["x"][k, a:b]).reshape(s) for a, b, s in zip(c["offs"][:-1], c["offs"][1:], c["shapes"])]


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
                leaf = seg.to(torch.int32).reshape(s)
            leaves.append(leaf)
            o += n
        trees.append(realize(c["struct"], leaves))
    return trees


def ref_aggregator(c):
    """(init, apply) of the oracle aggregator of the case."""
    kind, key = c["kind"], c["key"]
    if kind == "uniform":
        return cref.uniform_stochastic_quantizer(c["num_levels"], key)
    if kind == "uniform_arith":
        return cref.uniform_stochastic_quantizer(c["num_levels"], key, "arithmetic")
    if kind == "rotated":
        return cref.rotated_uniform_stochastic_quantizer(ROTATED_LEVELS, key, commute_inverse=True)
    if kind == "drive":
        return cref.structured_drive_quantizer(key)
    return cref.terngrad_quantizer(key)



@functools.lru_cache(maxsize=64)
def _reference(seed):
    from oracle import tree_util_ref as tu

    c = case(seed)
    clients = [("c%d" % k, realize(c["struct"], client_leaves(c, k)), c["weights"][k]) for k in range(c["K"])]
    init, apply = ref_aggregator(c)
    state, out = init(), []
    with np.errstate(all="ignore"):
        for _ in range(ROUNDS):
            agg, state = apply(clients, state)
            leaves = None if agg is None else [np.asarray(a, F32) for a in tu.flatten(agg)[0]]
            out.append((leaves, state.num_bits, np.array(state.rng)))
    return out


def reference(c):
    """[(mean leaves in flatten order or None, num_bits, rng)] after each of ROUNDS rounds of the
    oracle aggregator (``commute_inverse=True`` for ``rotated``: the product's operation order)."""
    return _reference(c["seed"])
