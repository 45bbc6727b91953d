// fjrobust_dev.h — one column of the coordinate-wise robust means (include/fjagg.h): K float32
// values, one per client, to the mean of the clients of rank t .. K-1-t (fjagg_trim_*,
// trim_column) or of the beta clients closest to the column's median (fjagg_meamed_*,
// around_median_column). Plain C++ that also compiles for the host, so the selection and the
// tie rule can be run against the numpy restatement without a GPU; fjrobust.hip is its only
// user in the library.
//
// A lane owns a column. Its K values become uint32 keys that order as the floats do
// (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN), padded to N = 16 / 32 / 64 / 128 with
// 0xFFFFFFFF, and are sorted: blocks of 16 by a static 80-exchange bitonic network in
// registers, and for N > 16 the exchanges at distance >= 16 through the lane's own slots of an
// LDS tile (pairs of keys, 8-byte accesses, slot q of lane l at q*STRIDE + l: conflict-free and
// private to the lane, so no barrier). Every exchange puts the minimum at the lower index (the
// mirror form of the bitonic merge), so no stage has a direction. From the sorted keys come L of
// rank t, U of rank K-1-t and the counts of keys below L, above U and equal to U, which give the
// tie cuts nL and cU - nU. The kept values are then added in client order from a second read of
// the column, which the caches serve. Every loop over clients is rolled in steps of 16 or 32, so
// the code stays a few KiB for every N. The mean around the median differs only between the
// sort and the cuts: a counting loop over the sorted keys places its window of beta sorted
// positions, and the numbers trimmed below and above the window differ.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FJR_HD __host__ __device__ __forceinline__
#else
#define FJR_HD inline
#endif

namespace fjrobust {

struct alignas(8) KeyPair {
  uint32_t x, y;
};

// float bits -> key: unsigned order of the keys is the total order of the floats
FJR_HD uint32_t key_of(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
// and back
FJR_HD uint32_t bits_of(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

FJR_HD float as_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}
FJR_HD uint32_t as_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
#endif
}
// separate, uncontracted IEEE ops (the build has -ffp-contract=off on both sides)
FJR_HD float add_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}
FJR_HD float sub_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}
FJR_HD float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}

FJR_HD void cx(uint32_t& a, uint32_t& b) {  // compare-exchange: minimum to a
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// the plain stages of a bitonic merge over 16 registers: distances D, D/2, .. 1
template <int D>
FJR_HD void merge16(uint32_t (&r)[16]) {
#pragma unroll
  for (int d = D; d >= 1; d >>= 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((i & d) == 0) cx(r[i], r[i | d]);
  }
}

// 16 registers, ascending: for s = 2, 4, 8, 16 the mirror stage (i with i ^ (s-1)), then the
// plain stages s/4 .. 1. 80 exchanges.
FJR_HD void sort16(uint32_t (&r)[16]) {
#pragma unroll
  for (int s = 2; s <= 16; s <<= 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((i & (s >> 1)) == 0) cx(r[i], r[i ^ (s - 1)]);
#pragma unroll
    for (int d = s >> 2; d >= 1; d >>= 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((i & d) == 0) cx(r[i], r[i | d]);
    }
  }
}

constexpr uint32_t kPad = 0xFFFFFFFFu;

// N == 16: the K keys, padded, sorted in r.
template <class Load>
FJR_HD void sort_column16(Load load, int K, uint32_t (&r)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) r[j] = j < K ? key_of(load(j)) : kPad;
  sort16(r);
}

// N > 16: the K keys, padded, sorted in the lane's tile slots (slot q holds positions 2q, 2q+1).
template <int N, int STRIDE, class Load>
FJR_HD void sort_column_tile(Load load, int K, KeyPair* tile) {
  // 32 clients a step (32 loads in flight), as two sorted blocks of 16 into the tile
#pragma unroll 1
  for (int c = 0; c < N / 32; ++c) {
    uint32_t lo[16], hi[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      lo[j] = 32 * c + j < K ? key_of(load(32 * c + j)) : kPad;
      hi[j] = 32 * c + 16 + j < K ? key_of(load(32 * c + 16 + j)) : kPad;
    }
    sort16(lo);
    sort16(hi);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      tile[(16 * c + j) * STRIDE] = KeyPair{lo[2 * j], lo[2 * j + 1]};
      tile[(16 * c + 8 + j) * STRIDE] = KeyPair{hi[2 * j], hi[2 * j + 1]};
    }
  }
  // merges of size s = 32 .. N; positions in pairs: slot q holds positions 2q, 2q+1
#pragma unroll 1
  for (int s = 32; s <= N; s <<= 1) {
    {  // mirror stage: position i with i ^ (s-1), i.e. slot q with q ^ (s/2 - 1), halves swapped
      const int m = s >> 2;  // slots in the lower half of a block of s/2 slots
#pragma unroll 4
      for (int p = 0; p < N / 4; ++p) {
        const int q = ((p & ~(m - 1)) << 1) | (p & (m - 1));
        const int qp = q ^ ((s >> 1) - 1);
        KeyPair a = tile[q * STRIDE], c = tile[qp * STRIDE];
        cx(a.x, c.y);
        cx(a.y, c.x);
        tile[q * STRIDE] = a;
        tile[qp * STRIDE] = c;
      }
    }
#pragma unroll 1
    for (int d = s >> 2; d >= 16; d >>= 1) {  // plain stages through the tile
      const int m = d >> 1;                     // distance in slots
#pragma unroll 4
      for (int p = 0; p < N / 4; ++p) {
        const int q = ((p & ~(m - 1)) << 1) | (p & (m - 1));
        const int qp = q | m;
        KeyPair a = tile[q * STRIDE], c = tile[qp * STRIDE];
        cx(a.x, c.x);
        cx(a.y, c.y);
        tile[q * STRIDE] = a;
        tile[qp * STRIDE] = c;
      }
    }
#pragma unroll 1
    for (int b = 0; b < N / 16; ++b) {  // distances 8 .. 1 inside each block of 16, in registers
      uint32_t r[16];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const KeyPair a = tile[(8 * b + j) * STRIDE];
        r[2 * j] = a.x;
        r[2 * j + 1] = a.y;
      }
      merge16<8>(r);
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[(8 * b + j) * STRIDE] = KeyPair{r[2 * j], r[2 * j + 1]};
    }
  }
}

// the key at sorted position j: a chain of selects over the registers (no dynamic register
// index), or one read of the lane's tile slot j/2
FJR_HD uint32_t key_at(const uint32_t (&r)[16], int j) {
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) v = i == j ? r[i] : v;
  return v;
}
template <int STRIDE>
FJR_HD uint32_t key_at(const KeyPair* tile, int j) {
  const KeyPair a = tile[(j >> 1) * STRIDE];
  return (j & 1) ? a.y : a.x;
}

// below = keys < L, above = keys > U, cU = keys == U among the K clients: the first K sorted
// positions hold the clients' keys as a multiset (pads sort last)
FJR_HD void count_keys(const uint32_t (&r)[16], int K, uint32_t L, uint32_t U, int& below, int& above, int& cU) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < K) {
      below += r[j] < L;
      above += r[j] > U;
      cU += r[j] == U;
    }
  }
}
template <int STRIDE>
FJR_HD void count_keys(const KeyPair* tile, int K, uint32_t L, uint32_t U, int& below, int& above, int& cU) {
#pragma unroll 4
  for (int q = 0; 2 * q < K; ++q) {
    const KeyPair e = tile[q * STRIDE];
    below += e.x < L;
    above += e.x > U;
    cU += e.x == U;
    if (2 * q + 1 < K) {
      below += e.y < L;
      above += e.y > U;
      cU += e.y == U;
    }
  }
}

// The kept values, added in client order from a second read of the column: the tile no longer
// has that order. A client is kept iff L <= key <= U and, if key == L, its running index among
// the L-valued is >= nL and, if key == U, its running index among the U-valued is < keepU.
// (Keeping the K keys in registers instead, with every client loop unrolled, measured the same
// rate with ten times the code and three times the registers: DESIGN 3l.)
template <class Load>
FJR_HD uint32_t kept_sum(Load load, int K, uint32_t L, uint32_t U, int nL, int keepU, bool do_scale, float scale) {
  int iL = 0, iU = 0;
  bool started = false;
  float s = 0.f;
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += 16) {
    uint32_t v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = k0 + j < K ? load(k0 + j) : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (k0 + j < K) {
        const uint32_t key = key_of(v[j]);
        const bool isL = key == L, isU = key == U;
        const bool keep = key >= L && key <= U && (!isL || iL >= nL) && (!isU || iU < keepU);
        iL += isL;
        iU += isU;
        const float x = as_float(v[j]);
        const float sum = add_rn(s, x);
        s = keep ? (started ? sum : x) : s;
        started = started || keep;
      }
    }
  }
  return as_bits(do_scale ? mul_rn(s, scale) : s);
}

// The column's result bits. load(k) returns client k's float bits for any 0 <= k < K (k is
// uniform over the wave; every client is loaded twice, see below); tile is this lane's slot 0
// of the LDS tile (N/2 slots STRIDE apart; unused, may be null, when N == 16).
// 1 <= K <= N, 0 <= 2t < K.
template <int N, int STRIDE, class Load>
FJR_HD uint32_t trim_column(Load load, int K, int t, bool do_scale, float scale, KeyPair* tile) {
  static_assert(N == 16 || N == 32 || N == 64 || N == 128, "instantiated widths");
  uint32_t L = 0, U = 0;
  int below = 0, above = 0, cU = 0;
  const int rl = t, ru = K - 1 - t;
  if constexpr (N == 16) {
    uint32_t r[16];
    sort_column16(load, K, r);
    L = key_at(r, rl);
    U = key_at(r, ru);
    count_keys(r, K, L, U, below, above, cU);
  } else {
    sort_column_tile<N, STRIDE>(load, K, tile);
    L = key_at<STRIDE>(tile, rl);
    U = key_at<STRIDE>(tile, ru);
    count_keys<STRIDE>(tile, K, L, U, below, above, cU);
  }
  // tie cuts: the first t sorted positions are the keys below L and then nL copies of L; the
  // last t are nU copies of U and then the keys above U.
  return kept_sum(load, K, L, U, t - below, cU - (t - above), do_scale, scale);
}

// A table entry as an index into [0, K): the project's rule for device tables, a stale entry can
// give a wrong result but never an address outside the slab. K >= 1.
FJR_HD int clamp_index(int32_t i, int K) { return i < 0 ? 0 : (i >= K ? K - 1 : (int)i); }

// Bucketing (include/fjagg.h, fjagg_trim_bucket_*): a per-bucket load made from a per-client
// one, so that trim_column and kept_sum run over bucket means with nothing else changed. Bucket
// j holds the clients table(j*s + i), i = 0 .. n_j - 1, n_j = min(s, K - j*s); its value is the
// first member verbatim, then a = fl(a + x) in table order, then fl(a * f32(1 / n_j)) unless
// n_j == 1, and a NaN so computed becomes 0x7FC00000 (a bucket of one keeps its member's bits).
// Only the last bucket can be short: inv_s is f32(1 / s), inv_last f32(1 / n_last).
// load(k) as for trim_column; table(m) returns entry m of the client table for 0 <= m < K,
// uniform over the wave, and is clamped here. The member loop is rolled (s is a run-time value)
// in steps of 8 whose loads are issued together before the first is added: two groups of 4
// without a branch inside (a position past the bucket's end loads the last member again and is
// not added), the second group skipped when the bucket ends before it. The routine is inlined
// at every load of the column routine, so its code has to stay this small.
template <class Load, class Table>
struct BucketLoad {
  Load load;
  Table table;
  int K, s;
  float inv_s, inv_last;
  // members i0 .. i0+3 of the bucket at m0: the four table entries first (four scalar loads in
  // flight on the device), then the four client loads
  FJR_HD void members4(int m0, int n, int i0, uint32_t* v) const {
    int r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = clamp_index(table(m0 + (i0 + i < n ? i0 + i : n - 1)), K);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = load(r[i]);
  }
  FJR_HD uint32_t operator()(int j) const {
    const int m0 = j * s;
    const int n = K - m0 < s ? K - m0 : s;
    uint32_t first = 0;
    float a = 0.f;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += 8) {
      uint32_t v[8];
      members4(m0, n, i0, v);
      if (i0 + 4 < n) {
        members4(m0, n, i0 + 4, v + 4);
      } else {
#pragma unroll
        for (int i = 4; i < 8; ++i) v[i] = 0u;
      }
      if (i0 == 0) first = v[0];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float x = as_float(v[i]);
        a = i0 + i < n ? (i0 + i == 0 ? x : add_rn(a, x)) : a;
      }
    }
    if (n == 1) return first;
    // IEEE leaves the sign and payload of a NaN result open, and the sign decides which end of
    // the order it is trimmed from: a computed NaN is the canonical +NaN on every machine
    const uint32_t y = as_bits(mul_rn(a, n == s ? inv_s : inv_last));
    return (y & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : y;
  }
};
template <class Load, class Table>
FJR_HD BucketLoad<Load, Table> bucket_load(Load load, Table table, int K, int s, float inv_s, float inv_last) {
  return BucketLoad<Load, Table>{load, table, K, s, inv_s, inv_last};
}

// Distance of a sorted key from the median's, as the bits of a non-negative float32 (which order
// as the floats do): 0 for the median's own key, else |fl(v - med)| with a NaN (a NaN operand,
// or inf - inf) replaced by +inf.
FJR_HD uint32_t distance_of(uint32_t key, uint32_t med_key, float med) {
  const uint32_t d = as_bits(sub_rn(as_float(bits_of(key)), med)) & 0x7FFFFFFFu;
  return key == med_key ? 0u : (d > 0x7F800000u ? 0x7F800000u : d);
}

// The mean around the median (include/fjagg.h, fjagg_meamed_*): the result bits of the column
// whose kept clients are the beta closest to the lower median s_mid, mid = (K-1)/2. With s the
// sorted values and d_j the distance of s_j from the median, d falls up to mid and rises after
// it, so the kept sorted positions are a window [a, a + beta) around mid, and "d[a + beta] <
// d[a]" (the value just above the window is strictly closer than the window's lowest) is true
// for a prefix of the candidate starts a_lo .. a_hi-1: the window starts at a_lo plus the number
// of true candidates, a rolled counting loop with no data-dependent branch. A tie keeps the
// lower side. load and tile as for trim_column; 1 <= K <= N, 1 <= beta <= K.
template <int N, int STRIDE, class Load>
FJR_HD uint32_t around_median_column(Load load, int K, int beta, bool do_scale, float scale, KeyPair* tile) {
  static_assert(N == 16 || N == 32 || N == 64 || N == 128, "instantiated widths");
  const int mid = (K - 1) >> 1;
  const int a_lo = mid - beta + 1 > 0 ? mid - beta + 1 : 0, a_hi = mid < K - beta ? mid : K - beta;
  uint32_t L = 0, U = 0;
  int below = 0, above = 0, cU = 0, a = a_lo;
  if constexpr (N == 16) {
    uint32_t r[16], d[16];
    sort_column16(load, K, r);
    const uint32_t mk = key_at(r, mid);
    const float med = as_float(bits_of(mk));
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = distance_of(r[j], mk, med);
    // every pair of positions beta apart, by static index: the candidate starts are uniform
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
      for (int j = i + 1; j < 16; ++j) a += (j - i == beta && i >= a_lo && i < a_hi && d[j] < d[i]) ? 1 : 0;
    }
    L = key_at(r, a);
    U = key_at(r, a + beta - 1);
    count_keys(r, K, L, U, below, above, cU);
  } else {
    sort_column_tile<N, STRIDE>(load, K, tile);
    const uint32_t mk = key_at<STRIDE>(tile, mid);
    const float med = as_float(bits_of(mk));
#pragma unroll 2
    for (int i = a_lo; i < a_hi; ++i)  // uniform positions: two tile reads a step
      a += distance_of(key_at<STRIDE>(tile, i + beta), mk, med) < distance_of(key_at<STRIDE>(tile, i), mk, med);
    L = key_at<STRIDE>(tile, a);  // the lane's own position: still its own slots
    U = key_at<STRIDE>(tile, a + beta - 1);
    count_keys<STRIDE>(tile, K, L, U, below, above, cU);
  }
  // the trim rule with two counts: a positions below the window, K - beta - a above it
  return kept_sum(load, K, L, U, a - below, cU - (K - beta - a - above), do_scale, scale);
}

}  // namespace fjrobust
