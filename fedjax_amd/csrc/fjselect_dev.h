// fjselect_dev.h — the selection rules of the whole-vector robust aggregates over the K x K
// float64 Gram matrix G of the client deltas (include/fjagg.h: fjagg_krum_select,
// fjagg_weiszfeld_select, fjagg_bulyan_select), and the tables of the second pass that follows
// them. Plain C++ that also compiles for the host, so the rules can be run against numpy without
// a GPU (tests/select_device_host.cpp, tests/bulyan_select_host.cpp); fjselect.hip is its only
// user in the library.
//
// Every function here is the work of ONE index (a client, a key position) or of the one lane
// that adds a sequential sum; the kernels give the indices to lanes and put barriers between the
// phases, krum_scores_host / krum_rank_host / weiszfeld_select_host below run the same phases as
// loops. All
// arithmetic is float64 in separate, uncontracted IEEE operations (the build has
// -ffp-contract=off on both sides); there is no FMA and no atomic, so the order of every sum is
// a function of (K, f, m) or of (K, iterations) alone.
//
// Krum: d2(i, j) = fl(fl(G_ii + G_jj) - fl(2 G_ij)), clamped at +0 when finite and +inf when not
// (or when either client is unusable: a non-finite G_kk). A non-negative double orders as its
// bits do, so row i's K - 1 distances become uint64 keys, padded to a power of two with all-ones
// keys (position i itself is a pad), sorted by a bitonic network, and the first K - f - 2 are
// added in that order from 0.0. The m smallest FINITE scores win, ties to the lower index.
//
// Smoothed Weiszfeld: see weiszfeld_select_host; every sum runs over the usable clients in
// ascending index, sequentially, from 0.0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FJS_HD __host__ __device__ __forceinline__
#else
#define FJS_HD inline
#endif

namespace fjselect {

constexpr int kMaxClients = 1024;
constexpr uint64_t kPadKey = ~0ull;
constexpr uint64_t kInfBits = 0x7ff0000000000000ull;

FJS_HD uint64_t bits_of(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__double_as_longlong(v);
#else
  uint64_t u;
  __builtin_memcpy(&u, &v, 8);
  return u;
#endif
}
FJS_HD double double_of(uint64_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)u);
#else
  double v;
  __builtin_memcpy(&v, &u, 8);
  return v;
#endif
}
FJS_HD bool finite(double v) { return (bits_of(v) & kInfBits) != kInfBits; }

// separate, correctly rounded IEEE operations
FJS_HD double add_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
FJS_HD double sub_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsub_rn(a, b);
#else
  return a - b;
#endif
}
FJS_HD double mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
FJS_HD double div_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
FJS_HD double sqrt_rn(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(a);
#else
  return __builtin_sqrt(a);
#endif
}

FJS_HD int pow2_at_least(int n) {
  int N = 2;
  while (N < n) N <<= 1;
  return N;
}

// ------------------------------------------------------------------------------------ Krum
// Key of position t in row i's padded key array: the bits of d2(i, t), or the pad for t = i and
// t >= K. gii / ok_i: the row's own diagonal entry and whether it is finite.
FJS_HD uint64_t krum_key(const double* __restrict__ G, int K, int i, int t, double gii, bool ok_i) {
  if (t >= K || t == i) return kPadKey;
  const double gjj = G[(int64_t)t * K + t];
  if (!ok_i || !finite(gjj)) return kInfBits;
  const double v = sub_rn(add_rn(gii, gjj), mul_rn(2.0, G[(int64_t)i * K + t]));
  if (!finite(v)) return kInfBits;
  return v > 0.0 ? bits_of(v) : 0ull;
}

// One compare-exchange of the bitonic network over keys[N]: index t at merge size k, distance j.
// An index pair is touched by its lower index alone, so all t of one (k, j) step are independent;
// the steps k = 2, 4 .. N, j = k/2 .. 1 need a barrier between them.
FJS_HD void bitonic_cx(uint64_t* keys, int t, int j, int k) {
  const int u = t ^ j;
  if (u > t) {
    const uint64_t a = keys[t], b = keys[u];
    if ((a > b) == ((t & k) == 0)) {
      keys[t] = b;
      keys[u] = a;
    }
  }
}

// The score of a row from its sorted keys: the first n = K - f - 2 of them, added in order from
// 0.0 (the pads sort last and n < K - 1, so they are never reached); +inf for an unusable client.
FJS_HD double krum_score(const uint64_t* keys, int n, bool ok_i) {
  if (!ok_i) return double_of(kInfBits);
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < n; ++c) s = add_rn(s, double_of(keys[c]));
  return s;
}

// Rank of client i by (score, index) among all K clients; score_keys[k] = bits of score_k (a
// score is never negative or NaN, so its bits order as it does; the infinite ones rank last).
FJS_HD int krum_rank(const uint64_t* score_keys, int K, int i) {
  const uint64_t mine = score_keys[i];
  int r = 0;
  for (int j = 0; j < K; ++j) r += (score_keys[j] < mine) || (score_keys[j] == mine && j < i);
  return r;
}

// how many of flags[0 .. i) are set: a selected client's slot in the ascending member order
FJS_HD int flags_below(const uint8_t* flags, int i) {
  int n = 0;
  for (int j = 0; j < i; ++j) n += flags[j];
  return n;
}

// One word of a group's plan image (fjagg_gather_member_ptrs; fjtrust.hip's gather): word idx is leaf
// idx % L of member slot j = idx / L and gets client order[j]'s pointer to that leaf from all[K*L].
// An order entry outside [0, K) copies nothing, whoever wrote the table.
FJS_HD void gather_member_word(const int64_t* __restrict__ all, int L, int K, const int32_t* __restrict__ order,
                               int64_t idx, int64_t* __restrict__ group) {
  const int64_t j = idx / L, l = idx - j * L;
  const int c = order[j];
  if ((unsigned)c < (unsigned)K) group[idx] = all[(int64_t)c * L + l];
}

// gscale of a group of `count` unit weights: the host's (1. / W if W > 0. else 0.), then float32
FJS_HD float krum_gscale(int count) { return count > 0 ? (float)div_rn(1.0, (double)count) : 0.0f; }

// ------------------------------------------------------------------------------ Weiszfeld
// np.maximum: a NaN on either side propagates
FJS_HD double max_np(double a, double b) { return (a >= b || a != a) ? a : b; }

// The sequential sum of term(j) over the j with ok[j], ascending, from 0.0. Eight terms are
// loaded before the eight additions, so the loads of a step are in flight together while the
// additions keep their order; a term of a skipped j is computed and dropped (never added).
template <class Term>
FJS_HD double seq_sum(int K, const uint8_t* ok, Term term) {
  double s = 0.0;
  int j = 0;
  for (; j + 8 <= K; j += 8) {
    double v[8];
    bool o[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v[u] = term(j + u);
      o[u] = ok[j + u] != 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s = o[u] ? add_rn(s, v[u]) : s;
  }
  for (; j < K; ++j)
    if (ok[j]) s = add_rn(s, term(j));
  return s;
}

// sum of v[k] over the usable k in ascending order, from 0.0 (the one lane's job)
FJS_HD double usable_sum(const double* v, const uint8_t* ok, int K) {
  return seq_sum(K, ok, [=](int k) { return v[k]; });
}

// (Ga)_k = sum_j fl(G_kj a_j) over the usable j; walks COLUMN k of G, which holds row k's bits
// (the Gram pass mirrors its lower triangle), so the lanes of a wave load consecutive doubles.
FJS_HD double weiszfeld_ga(const double* __restrict__ G, int K, int k, const double* a, const uint8_t* ok) {
  return seq_sum(K, ok, [=](int j) { return mul_rn(G[(int64_t)j * K + k], a[j]); });
}

// q = sum_k fl(a_k (Ga)_k) over the usable k (the one lane's job)
FJS_HD double weiszfeld_q(const double* a, const double* ga, const uint8_t* ok, int K) {
  return seq_sum(K, ok, [=](int k) { return mul_rn(a[k], ga[k]); });
}

// d_k = sqrt(max(q - 2 (Ga)_k + G_kk, 0)), a NaN propagating as in np.maximum
FJS_HD double weiszfeld_distance(double q, double ga_k, double gkk) {
  const double r = add_rn(sub_rn(q, mul_rn(2.0, ga_k)), gkk);
  return sqrt_rn(r > 0.0 ? r : (r == r ? 0.0 : r));
}

FJS_HD double weiszfeld_beta(double alpha_k, double nu, double d_k) { return div_rn(alpha_k, max_np(nu, d_k)); }

// W = the sequential float64 sum of the members' float32 weights, in member (= client) order
FJS_HD double member_total(const float* a32, const uint8_t* member, int K) {
  return seq_sum(K, member, [=](int k) { return (double)a32[k]; });
}
FJS_HD float total_gscale(double W) { return W > 0.0 ? (float)div_rn(1.0, W) : 0.0f; }

// ------------------------------------------------------------------------------------ Bulyan
// Bulyan's first stage (include/fjagg.h: fjagg_bulyan_select; fedjax_amd.robust.bulyan_select bit
// for bit): theta = K - 2f times, the client of smallest finite score among the set R of usable
// clients not yet chosen, which then leaves R. With n = |R| and c = max(n - f - 2, 1), score_i is
// the c smallest d2(i, j), j in R without i, added in ascending order from 0.0 (0.0 when n = 1);
// d2 is krum_key's value. K >= 4f + 3 and theta <= 128 bound K at 252 (kBulyanMaxClients): a
// client index fits a byte and one workgroup of 256 lanes owns one row per lane.
//
// Every row's K - 1 (key, index) pairs are sorted ONCE, by (key, index), and stored position-major
// (position p of row i at p*K + i), so the lanes of a wave walk consecutive words. A step takes a
// live row's first c live neighbours in that order: the sums of a fresh sort per step. Two
// neighbours at the same distance contribute the same term whichever is taken, so the sort need
// only order by the key; index order among equal keys cannot change any sum (it is there to make
// the sorted table itself a function of G alone).
constexpr int kBulyanMaxClients = 252;
constexpr int kBulyanMaxSelected = 128;  // theta: what the second stage's column routine takes
constexpr int kBulyanLanes = 256;
constexpr int kBulyanBatch = 16;  // loads in flight per lane in a step's walk

// bitonic_cx over (key, index) pairs
FJS_HD void bitonic_cx_pair(uint64_t* keys, uint8_t* idx, int t, int j, int k) {
  const int u = t ^ j;
  if (u > t) {
    const uint64_t a = keys[t], b = keys[u];
    const uint8_t ia = idx[t], ib = idx[u];
    if ((a > b || (a == b && ia > ib)) == ((t & k) == 0)) {
      keys[t] = b;
      keys[u] = a;
      idx[t] = ib;
      idx[u] = ia;
    }
  }
}

// neighbours a step needs of each of n remaining clients
FJS_HD int bulyan_neighbours(int n, int f) { return n - f - 2 > 1 ? n - f - 2 : 1; }

// Row i's score in a step: its first c live neighbours of the sorted tables, added in order from
// 0.0. Sixteen positions are loaded before the sixteen additions (as seq_sum does with eight); a position past the
// c-th live one is loaded and dropped. With no live neighbour (n = 1) the sum is 0.0.
FJS_HD double bulyan_score(const uint64_t* __restrict__ skeys, const uint8_t* __restrict__ sidx, int K, int i, int c,
                           const uint8_t* alive) {
  double s = 0.0;
  int taken = 0;
  for (int p0 = 0; p0 < K - 1 && taken < c; p0 += kBulyanBatch) {
    uint64_t kv[kBulyanBatch];
    uint8_t jv[kBulyanBatch];
#pragma unroll
    for (int u = 0; u < kBulyanBatch; ++u) {
      const int p = p0 + u < K - 1 ? p0 + u : K - 2;
      kv[u] = skeys[(int64_t)p * K + i];
      jv[u] = sidx[(int64_t)p * K + i];
    }
#pragma unroll
    for (int u = 0; u < kBulyanBatch; ++u) {
      const bool take = p0 + u < K - 1 && taken < c && alive[jv[u]] != 0;
      s = take ? add_rn(s, double_of(kv[u])) : s;
      taken += take;
    }
  }
  return s;
}

// What a client brings to a step's argmin: its score's bits (a score is never negative or NaN),
// or the pad when it is not in R or its score is not finite, so that a pad can never win.
FJS_HD uint64_t bulyan_candidate(double score, bool live) {
  return live && finite(score) ? bits_of(score) : kPadKey;
}
// (bits a, client ia) before (bits b, client ib): the smaller score, ties to the lower index
FJS_HD bool bulyan_before(uint64_t a, int ia, uint64_t b, int ib) { return a < b || (a == b && ia < ib); }

FJS_HD int bulyan_keep(int count, int f) { return count - 2 * f >= 1 ? count - 2 * f : 0; }
// the bits the host route passes: np.float32(1 / keep)
FJS_HD float bulyan_scale(int keep) { return keep > 0 ? (float)div_rn(1.0, (double)keep) : 0.0f; }

// ---------------------------------------------------- the whole rules as loops (host builds)
#if !defined(__HIP_DEVICE_COMPILE__)
// fjagg_krum_select's two launches. The first: scores[K] from G[K][K]; keys: scratch of
// pow2_at_least(K) words.
inline void krum_scores_host(const double* G, int K, int f, uint64_t* keys, double* scores) {
  const int N = pow2_at_least(K), n = K - f - 2;
  for (int i = 0; i < K; ++i) {
    const double gii = G[(int64_t)i * K + i];
    const bool ok_i = finite(gii);
    for (int t = 0; t < N; ++t) keys[t] = krum_key(G, K, i, t, gii, ok_i);
    for (int k = 2; k <= N; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1)
        for (int t = 0; t < N; ++t) bitonic_cx(keys, t, j, k);
    scores[i] = krum_score(keys, n, ok_i);
  }
}

// The second: from scores[K], selected[m] (best first, -1 padded), *count, order[m] (ascending
// client index, 0 padded), seg[2], wperm[m], gscale[1].
inline void krum_rank_host(const double* scores, int K, int m, int64_t* selected, int32_t* count, int32_t* order,
                           int32_t* seg, float* wperm, float* gscale) {
  uint64_t score_keys[kMaxClients];
  uint8_t flags[kMaxClients];
  for (int i = 0; i < K; ++i) score_keys[i] = bits_of(scores[i]);
  int c = 0;
  for (int i = 0; i < K; ++i) {
    const int r = krum_rank(score_keys, K, i);
    flags[i] = finite(scores[i]) && r < m;
    if (flags[i]) selected[r] = i;
    c += flags[i];
  }
  for (int i = 0; i < K; ++i)
    if (flags[i]) order[flags_below(flags, i)] = i;
  for (int r = c; r < m; ++r) {
    selected[r] = -1;
    order[r] = 0;
  }
  for (int r = 0; r < m; ++r) wperm[r] = 1.0f;
  *count = c;
  seg[0] = 0;
  seg[1] = c;
  gscale[0] = krum_gscale(c);
}

// fjagg_weiszfeld_select's outputs from G[K][K], alpha[K] (null: ones), nu, iterations:
// a[K], d[K], a32[K], *count, order[K] (0 padded), seg[2], wperm[K] (0 padded), gscale[1].
inline void weiszfeld_select_host(const double* G, int K, const double* alpha, double nu, int iterations, double* a,
                                  double* d, float* a32, int32_t* count, int32_t* order, int32_t* seg, float* wperm,
                                  float* gscale) {
  double al[kMaxClients], ga[kMaxClients], beta[kMaxClients];
  uint8_t ok[kMaxClients], member[kMaxClients];
  for (int k = 0; k < K; ++k) {
    ok[k] = finite(G[(int64_t)k * K + k]);
    al[k] = alpha ? alpha[k] : 1.0;
    beta[k] = 0.0;
  }
  const double S = usable_sum(al, ok, K);
  for (int k = 0; k < K; ++k) {
    a[k] = ok[k] ? div_rn(al[k], S) : 0.0;
    d[k] = ok[k] ? 0.0 : double_of(kInfBits);
  }
  for (int it = 0; it < iterations; ++it) {
    for (int k = 0; k < K; ++k) ga[k] = ok[k] ? weiszfeld_ga(G, K, k, a, ok) : 0.0;
    const double q = weiszfeld_q(a, ga, ok, K);
    for (int k = 0; k < K; ++k)
      if (ok[k]) {
        d[k] = weiszfeld_distance(q, ga[k], G[(int64_t)k * K + k]);
        beta[k] = weiszfeld_beta(al[k], nu, d[k]);
      }
    const double B = usable_sum(beta, ok, K);
    for (int k = 0; k < K; ++k)
      if (ok[k]) a[k] = div_rn(beta[k], B);
  }
  int c = 0;
  for (int k = 0; k < K; ++k) {
    a32[k] = (float)a[k];
    member[k] = ok[k] && a32[k] > 0.0f;
    c += member[k];
  }
  for (int k = 0; k < K; ++k)
    if (member[k]) {
      const int p = flags_below(member, k);
      order[p] = k;
      wperm[p] = a32[k];
    }
  for (int p = c; p < K; ++p) {
    order[p] = 0;
    wperm[p] = 0.0f;
  }
  *count = c;
  seg[0] = 0;
  seg[1] = c;
  gscale[0] = total_gscale(member_total(a32, member, K));
}

// fjagg_bulyan_select's two launches from G[K][K] and f (3 <= 4f + 3 <= K <= kBulyanMaxClients,
// theta = K - 2f <= kBulyanMaxSelected). skeys / sidx: the workspace, K * (K - 1) words and bytes.
// Outputs: selected[theta] (selection order, -1 padded), *count, step_scores[theta] (+inf padded),
// *keep, *scale, rows[theta] (the chosen clients ascending, then the last one repeated; 0s if none).
inline void bulyan_select_host(const double* G, int K, int f, uint64_t* skeys, uint8_t* sidx, int64_t* selected,
                               int32_t* count, double* step_scores, int32_t* keep, float* scale, int32_t* rows) {
  const int N = pow2_at_least(K), theta = K - 2 * f;
  uint64_t keys[kBulyanLanes];
  uint8_t idx[kBulyanLanes], alive[kBulyanLanes], chosen[kBulyanLanes];
  // the first launch: one workgroup per row
  for (int i = 0; i < K; ++i) {
    const double gii = G[(int64_t)i * K + i];
    const bool ok_i = finite(gii);
    for (int t = 0; t < N; ++t) {
      keys[t] = krum_key(G, K, i, t, gii, ok_i);
      idx[t] = (uint8_t)t;
    }
    for (int k = 2; k <= N; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1)
        for (int t = 0; t < N; ++t) bitonic_cx_pair(keys, idx, t, j, k);
    for (int p = 0; p < K - 1; ++p) {  // the pads (i itself, t >= K) sort last and stay behind
      skeys[(int64_t)p * K + i] = keys[p];
      sidx[(int64_t)p * K + i] = idx[p];
    }
  }
  // the second: one workgroup, lane i owns client i
  int n = 0, c = 0;
  for (int i = 0; i < K; ++i) {
    alive[i] = finite(G[(int64_t)i * K + i]);
    chosen[i] = 0;
    n += alive[i];
  }
  for (; c < theta; ++c) {
    uint64_t best = kPadKey;
    int who = K;
    const int take = bulyan_neighbours(n, f);
    for (int i = 0; i < K; ++i) {
      const double s = alive[i] ? bulyan_score(skeys, sidx, K, i, take, alive) : 0.0;
      const uint64_t cand = bulyan_candidate(s, alive[i] != 0);
      if (bulyan_before(cand, i, best, who)) {
        best = cand;
        who = i;
      }
    }
    if (best == kPadKey) break;  // R is empty, or no score is finite
    selected[c] = who;
    step_scores[c] = double_of(best);
    alive[who] = 0;
    chosen[who] = 1;
    --n;
  }
  int last = 0;
  for (int i = 0; i < K; ++i)
    if (chosen[i]) {
      rows[flags_below(chosen, i)] = i;
      last = i;
    }
  for (int r = c; r < theta; ++r) {
    selected[r] = -1;
    step_scores[r] = double_of(kInfBits);
    rows[r] = last;
  }
  *count = c;
  *keep = bulyan_keep(c, f);
  *scale = bulyan_scale(*keep);
}
#endif

}  // namespace fjselect
