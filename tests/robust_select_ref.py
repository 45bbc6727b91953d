"""Restatements for the Gram-matrix aggregates, on the client VECTORS in float64 — no Gram
matrix anywhere: brute-force Krum (Blanchard et al., NeurIPS 2017) and the direct-form smoothed
Weiszfeld iteration (Pillutla et al., IEEE TSP 2022). Plus a numpy emulation of the Gram kernel's
arithmetic (float32 fmaf chains of C columns, added in float64): a bitwise reference on integer
data, a yardstick for accuracy on general data (chain_gram, gram_of_ranges). Plus the data, the
bounds and the case lists of the fuzz and limit tests (offset_data, krum_error_bound, sweep_cases)."""
import numpy as np


def krum_scores(x, f):
    """score_i = sum of the K - f - 2 smallest |x_i - x_j|^2, j != i; inf for a non-finite row
    (a row is compared only with finite rows; a non-finite neighbour is infinitely far)."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    finite = [bool(np.isfinite(x[k]).all()) for k in range(K)]
    scores = []
    for i in range(K):
        if not finite[i]:
            scores.append(np.inf)
            continue
        d = []
        for j in range(K):
            if j == i:
                continue
            if not finite[j]:
                d.append(np.inf)
                continue
            diff = x[i] - x[j]
            d.append(float(np.dot(diff, diff)))
        d.sort()
        s = 0.0
        for v in d[: K - f - 2]:
            s += v
        scores.append(s)
    return np.array(scores, dtype=np.float64)


def krum_select(x, f, m):
    """The m finite-score clients of smallest score, ties to the lower index."""
    scores = krum_scores(x, f)
    order = sorted(range(len(scores)), key=lambda k: (scores[k], k))
    return np.array([k for k in order if np.isfinite(scores[k])][:m], dtype=np.int64), scores


def weiszfeld(x, alpha, nu, iterations):
    """Direct form on the vectors: v = sum a_k x_k; d_k = |v - x_k|; beta_k = alpha_k / max(nu, d_k);
    a = beta / sum beta. Returns (a, v) with v the final point sum a_k x_k. Finite rows only."""
    x = np.asarray(x, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    a = alpha / alpha.sum()
    for _ in range(iterations):
        v = a @ x
        d = np.sqrt(((x - v[None, :]) ** 2).sum(axis=1))
        beta = alpha / np.maximum(nu, d)
        a = beta / beta.sum()
    return a, a @ x


def _fold(x, segs, arithmetic):
    """float32 accumulators of the column segments `segs` ((start, end) pairs, each one chain),
    every segment from +0 in column order; all segments advance together, one column (or one
    pair of columns) per step. Returns float64[len(segs), K, K]."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    K = x64.shape[0]
    x64 = np.concatenate([x64, np.zeros((K, 1))], axis=1)  # column P: the zero past a segment's end
    zero = x64.shape[1] - 1
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
    order = np.argsort(-(segs[:, 1] - segs[:, 0]), kind="stable")  # longest first: the live ones are a prefix
    start, length = segs[order, 0], (segs[order, 1] - segs[order, 0])
    acc = np.zeros((len(segs), K, K), dtype=np.float32)
    step = 2 if arithmetic == "pairwise" else 1
    for t in range(0, int(length.max(initial=0)), step):
        nb = int((length > t).sum())
        cols = x64[:, start[:nb] + t]
        prod = np.einsum("ib,jb->bij", cols, cols)
        if arithmetic == "pairwise":  # the two k-steps of one 32x32x2 instruction added first
            cols = x64[:, np.where(length[:nb] > t + 1, start[:nb] + t + 1, zero)]
            prod = prod + np.einsum("ib,jb->bij", cols, cols)
        elif arithmetic == "unfused":  # the product rounded on its own
            prod = prod.astype(np.float32).astype(np.float64)
        acc[:nb] = (acc[:nb].astype(np.float64) + prod).astype(np.float32)
    out = np.empty(acc.shape, dtype=np.float64)
    out[order] = acc
    return out


def gram_of_ranges(x, ranges, chain, arithmetic="fmaf", drop_partial=False):
    """The pytree route's arithmetic: `ranges` is a list of column ranges (start, end) of x[K, P]
    (the leaves laid side by side), in plan order (:func:`plan_ranges`). Every range is cut into
    chains of `chain` columns from ITS start; a chain accumulates every pair's products in float32
    in column order from +0; the chains are added in float64 in range order.

    `arithmetic`: "fmaf" is float32(float64(acc) + float64(a) * float64(b)). The float64 product
    of two float32 is exact; the sum is rounded to float64 and then to float32. Whenever that
    float64 sum is exact — integer data with every partial sum below 2^53, for one — there is one
    rounding and this IS fmaf(a, b, acc), bit for bit. On general data a double rounding is
    possible (rare), and the function is a yardstick only, not a bitwise reference.
    Two deliberately wrong arithmetics, for tests that show the data can tell them apart:
    "pairwise" float32(acc + (a0 b0 + a1 b1)) per pair of columns from the chain's start, and
    "unfused" float32(acc + float32(a b)). `drop_partial`: a range's last, shorter chain is lost
    (a kernel without the fold at a range's end)."""
    x = np.asarray(x, dtype=np.float32)
    segs = []
    for e0, e1 in ranges:
        for c0 in range(int(e0), int(e1), chain):
            if not (drop_partial and c0 + chain > e1):
                segs.append((c0, min(int(e1), c0 + chain)))
    G = np.zeros((x.shape[0], x.shape[0]), dtype=np.float64)
    for c in _fold(x, segs, arithmetic):
        G += c
    return G


def chain_gram(x, chain, arithmetic="fmaf", drop_partial=False):
    """The dense route's arithmetic in numpy: chains of `chain` columns from column 0, per chain
    every pair's products accumulated in float32 in column order from +0, chains added in float64
    (:func:`gram_of_ranges` over the one range [0, P)).

    On "mid-size integer" data (:func:`midsize_ints`) this is a BITWISE reference for
    fjagg_gram_dense with chain = FJAGG_GRAM_CHAIN: every product is an integer below 2^24 and
    every float32 partial sum an integer below 2^32, so float32(float64(acc) + a b) rounds once
    and equals fmaf(a, b, acc); every float64 addition of chains is exact (|G| < 2^53 for
    P <= 20000), so neither the chunk order nor the combine order matters. The same holds for any
    integer data whose sums stay below 2^53 (:func:`wide_ints`). On general float data the float64
    sum may round before the float32 rounding does (a rare double rounding) and the order of the
    float64 additions matters: there this is a yardstick for accuracy only, not a bitwise
    reference."""
    x = np.asarray(x, dtype=np.float32)
    return gram_of_ranges(x, [(0, x.shape[1])], chain, arithmetic, drop_partial)


def plan_ranges(blocks, leaf_n, unit):
    """Column ranges (start, end) of the rows laid side by side, one per entry of a pytree plan,
    in plan order. `blocks` is the int64 array of kernels.ptrs_plan (two words per entry), decoded
    as include/fjagg.h documents and k_gram_ptrs does: word 0 holds the first unit in bits 0..39,
    the leaf in bits 40..61, the tail flag in bit 62 and the element flag in bit 63; word 1 the end
    unit. A unit is `unit` elements (4 for float32; 1 for a plan made with FJAGG_UNALIGNED), or one
    element in an entry with the element flag; a tail entry covers [n // unit * unit, n) of its leaf."""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 2)
    leaf_n = [int(n) for n in leaf_n]
    offs = np.concatenate([[0], np.cumsum(leaf_n)])
    out = []
    for w0, w1 in blocks.tolist():
        leaf = (w0 >> 40) & 0x3FFFFF
        tail, elem = (w0 >> 62) & 1, w0 < 0
        u0 = w0 & ((1 << 40) - 1)
        n = leaf_n[leaf]
        if tail:
            e0, e1 = n // unit * unit, n
        elif elem:
            e0, e1 = u0, w1
        else:
            e0, e1 = u0 * unit, w1 * unit
        e1 = min(e1, n)
        out.append((int(offs[leaf]) + e0, int(offs[leaf]) + max(e0, e1)))
    return out


MIDSIZE = 2896  # 2896^2 < 2^23: see midsize_ints


def midsize_ints(rng, K, P, bound=MIDSIZE):
    """"Mid-size integer" data: integers uniform in [-2896, 2896] as float32. A product is an
    integer below 2^23.01 and a chain of 256 of them below 2^32, so most partial sums need more
    than float32's 24 bits (the result depends on the chain length and on the order inside the
    instruction) while every operation of :func:`chain_gram` is a single rounding."""
    return rng.integers(-bound, bound + 1, size=(K, P)).astype(np.float32)


BITWISE_KS = (1, 3, 33, 65, 129, 160, 257)
MIDSIZE_SEED = 2000000  # chosen so that even the 1 x 1 and 3 x 3 cases tell the arithmetics apart


def bitwise_columns(chunk_cols, chain=256):
    """The column counts of the bitwise tests: around one chain, past two chains, around two
    workgroup chunks of `chunk_cols` columns (kernels.gram_chunk_columns)."""
    return (1, chain - 1, chain, chain + 1, 2 * chain + 3, 2 * chunk_cols - 1, 2 * chunk_cols + 1)


def midsize_case(K, P):
    """The mid-size integer slab of the bitwise case (K, P), the same on the CPU and on the GPU."""
    return midsize_ints(np.random.default_rng(MIDSIZE_SEED + 1000 * K + P), K, P)


def wide_ints(rng, K, P):
    """Integers uniform in [-2^14, 2^14]: most products need more than 24 bits, so a product
    rounded on its own ("unfused") differs from the fused one, and everything stays an integer
    below 2^53."""
    return rng.integers(-(1 << 14), (1 << 14) + 1, size=(K, P)).astype(np.float32)


def absorption_rows(starts, P, ones=300):
    """Row i holds 2^12 at column starts[i], 1.0 at the next `ones` columns and zeros elsewhere.
    In a column-ordered float32 chain G_ii starts at 2^24 and every 2^24 + 1 rounds back to 2^24
    (ties to even) until the chain is folded and restarts from +0: G_ii - 2^24 counts the ones after
    the first fold, so it shows the column at which that fold happened."""
    x = np.zeros((len(starts), P), dtype=np.float32)
    for i, c in enumerate(starts):
        assert c + 1 + ones <= P
        x[i, c] = 4096.0
        x[i, c + 1:c + 1 + ones] = 1.0
    return x


def outlier_data(rng, K, P, outliers):
    """0.01 * N(0, 1) honest clients and `outliers` N(0, 1) ones at the end, float32."""
    x = (0.01 * rng.standard_normal((K, P))).astype(np.float32)
    if outliers:
        x[K - outliers:] = rng.standard_normal((outliers, P)).astype(np.float32)
    return x


# ------------------------------------------------------------------ Krum and the median on float data
GRAM_CHAIN = 256  # FJAGG_GRAM_CHAIN (tests assert it equals kernels.GRAM_CHAIN)
GAMMA_C = GRAM_CHAIN * 2.0 ** -24 / (1 - GRAM_CHAIN * 2.0 ** -24)
OFFSET_RATIOS = (0, 1, 10, 100, 1e3, 1e4)
OFFSET_P = 2003
# (K, f, m) of the float-data Krum tests, and per (K, ratio in {0, 1}) a seed at which the
# brute-force scores are separated by more than 2 E around and inside the selection
# (tests/test_robust_select_ref.py asserts it); larger ratios reuse the seed of ratio 1
OFFSET_KRUM = ((9, 2, 2), (16, 3, 4), (33, 6, 3))
OFFSET_SEEDS = {(9, 0): 0, (9, 1): 0, (16, 0): 0, (16, 1): 0, (33, 0): 0, (33, 1): 0}


def offset_outliers(K):
    return max(1, K // 5)


def offset_seed(K, ratio):
    return OFFSET_SEEDS[(K, 0 if ratio == 0 else 1)]


def offset_data(rng, K, P, ratio, outliers):
    """Clients with a common component: x_k = ratio * mu + N(0, 1), mu ~ N(0, 1) drawn once per
    case; the last `outliers` rows get an extra 3 * N(0, 1). float32. ratio is the size of the
    common component relative to the clients' spread: 0 is a round of centred deltas, 1e3 a round of
    models that differ in their fourth digit."""
    mu = rng.standard_normal(P)
    x = ratio * mu[None, :] + rng.standard_normal((K, P))
    if outliers:
        x[K - outliers:] += 3.0 * rng.standard_normal((outliers, P))
    return x.astype(np.float32)


def krum_error_bound(x, f):
    """E with |score_from_G - score_true| <= E for every client, G any Gram within the library's
    bound (d) (include/fjagg.h): |G_ij - <x_i, x_j>| <= gamma_C * mass_ij,
    mass = |x| |x|^T in float64, gamma_C = C u / (1 - C u), C = 256, u = 2^-24.

        E = (K - f - 2) * gamma_C * max_ij (mass_ii + mass_jj + 2 mass_ij)

    Derivation. d2(i, j) = G_ii + G_jj - 2 G_ij, so by (d) its error is at most
    D = gamma_C * max_ij (mass_ii + mass_jj + 2 mass_ij) for every pair. The clamp max(., 0) is a
    contraction and the true d2 is >= 0, so the clamped value is within D too. "The sum of the k
    smallest of n numbers" is k-Lipschitz in the max-norm: move every number by at most D and the
    sum of the k smallest moves by at most k D (the k smallest of the moved numbers sum to at most
    the moved versions of the old k smallest, and the other way round). With k = K - f - 2 that is
    E. The float64 roundings of the score's own additions and of the brute-force reference are below
    K * 2^-52 of the score, seven orders under gamma_C, and are not counted.

    Consequences used by the tests: if the true scores of two clients differ by more than 2 E their
    order under G is the true order; a selected client s and a usable unselected one u always
    satisfy true[s] <= true[u] + 2 E."""
    x64 = np.abs(np.asarray(x, dtype=np.float64))
    K = x64.shape[0]
    mass = x64 @ x64.T
    d = np.diagonal(mass)
    return (K - f - 2) * GAMMA_C * float((d[:, None] + d[None, :] + 2.0 * mass).max())


# ------------------------------------------------------------------ the seeded sweep
SWEEP_EDGE_KS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023, 1024)
SWEEP_HEAVY_KS = (192, 256, 257, 1024)  # edge cases whose plan is made longer than the chunk count


def int_krum(x, f, m):
    """Brute-force Krum on integer vectors in exact int64 arithmetic: (selected, scores) with the
    scores as float64 (exact: every sum is far below 2^53), ties to the lower index."""
    x = np.asarray(x)
    assert np.abs(x).max(initial=0) <= 90 and (x == np.rint(x)).all()  # (2 * 90)^2 fits an int16
    x = x.astype(np.int16)
    K = x.shape[0]
    scores = np.empty(K, dtype=np.int64)
    for i in range(K):
        diff = x - x[i]
        d = np.delete((diff * diff).sum(axis=1, dtype=np.int64), i)
        scores[i] = np.sort(d)[: K - f - 2].sum()
    return np.argsort(scores, kind="stable")[:m].astype(np.int64), scores.astype(np.float64)


def sweep_cases():
    """40 fixed-seed cases (K, leaves, views, f, m, seed) for the Gram pass and Krum on small
    integers. Even cases take K from the panel and block edges SWEEP_EDGE_KS, odd ones uniform in
    1..300. 1-7 leaves of 0..3000 elements: empty and 1-element leaves, 4n +- 1 and 256n +- 1 among
    them (K >= 1023: at most 600 elements in all). views: every odd client's leaves are views into
    one row of its own (a leaf at an element offset that is no multiple of 4 then takes element
    units), the even clients' leaves separate allocations; or all separate. f, m: a random valid
    Krum setting, None for K < 3."""
    rng = np.random.RandomState(20240)
    cases = []
    for i in range(40):
        K = int(SWEEP_EDGE_KS[i // 2]) if i % 2 == 0 else int(rng.randint(1, 301))
        small = K >= 1023
        heavy = i % 2 == 0 and K in SWEEP_HEAVY_KS
        while not heavy:
            leaves = []
            for _ in range(int(rng.randint(1, 8))):
                kind = int(rng.randint(0, 6))
                if kind == 0:
                    n = 0
                elif kind == 1:
                    n = 1
                elif kind == 2:
                    n = 4 * int(rng.randint(1, 30 if small else 750)) + (1 if rng.randint(2) else -1)
                elif kind == 3:
                    n = 256 * int(rng.randint(1, 2 if small else 12)) + (1 if rng.randint(2) else -1)
                else:
                    n = int(rng.randint(0, 101 if small else 3001))
                leaves.append(min(n, 3000))
            if not small or sum(leaves) <= 600:
                break
        views = bool(rng.randint(0, 4))  # three cases in four
        if heavy:
            # seven leaves of 4n + 1 elements as views: the leaves at offsets 1, 2, 3 mod 4 take element
            # units, 64 elements per plan entry, so the plan has more entries than the pytree kernel
            # has chunks (512 // panel pairs) and a chunk walks several of them
            lo, hi = (16, 17) if small else (260, 330) if K > 256 else (500, 600)
            leaves = [4 * int(rng.randint(lo, hi)) + 1 for _ in range(7)]
            if small:
                leaves[1] = leaves[2] = 4 * int(rng.randint(32, 34)) + 1
            views = True
        f = m = None
        if K >= 3:
            f = int(rng.randint(0, (K - 3) // 2 + 1))
            m = int(rng.randint(1, K - f + 1))
        cases.append((K, leaves, views, f, m, 5000 + i))
    return cases


def sweep_elem_mask(K, leaves, views):
    """The per-leaf element-unit mask of a sweep case's plan: with views (and an odd client, K >= 2)
    a leaf that starts at an element offset that is no multiple of 4 is not 16-byte aligned."""
    offs = np.concatenate([[0], np.cumsum(leaves)])[:-1]
    return np.array([bool(views and K >= 2 and n > 0 and o % 4) for o, n in zip(offs, leaves)])
