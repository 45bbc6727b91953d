// fjrobust_dev.h — one column of the coordinate-wise trimmed mean (include/fjagg.h,
// fjagg_trim_*): K float32 values, one per client, to the mean of the clients of rank
// t .. K-1-t. Plain C++ that also compiles for the host, so the selection and the tie rule
// can be run against the numpy restatement without a GPU; fjrobust.hip is its only user in
// the library.
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
// the code stays a few KiB for every N.
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

// The column's result bits. load(k) returns client k's float bits for any 0 <= k < K (k is
// uniform over the wave; every client is loaded twice, see below); tile is this lane's slot 0
// of the LDS tile (N/2 slots STRIDE apart; unused, may be null, when N == 16).
// 1 <= K <= N, 0 <= 2t < K.
template <int N, int STRIDE, class Load>
FJR_HD uint32_t trim_column(Load load, int K, int t, bool do_scale, float scale, KeyPair* tile) {
  static_assert(N == 16 || N == 32 || N == 64 || N == 128, "instantiated widths");
  constexpr uint32_t kPad = 0xFFFFFFFFu;
  uint32_t L = 0, U = 0;
  int below = 0, above = 0, cU = 0;  // keys < L, keys > U, keys == U among the K clients
  const int rl = t, ru = K - 1 - t;
  if constexpr (N == 16) {
    uint32_t r[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) r[j] = j < K ? key_of(load(j)) : kPad;
    sort16(r);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      L = j == rl ? r[j] : L;
      U = j == ru ? r[j] : U;
    }
    // the first K sorted positions hold the clients' keys as a multiset (pads sort last)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < K) {
        below += r[j] < L;
        above += r[j] > U;
        cU += r[j] == U;
      }
    }
  } else {
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
    const KeyPair a = tile[(rl >> 1) * STRIDE], c = tile[(ru >> 1) * STRIDE];
    L = (rl & 1) ? a.y : a.x;
    U = (ru & 1) ? c.y : c.x;
    // the first K sorted positions hold the clients' keys as a multiset (pads sort last)
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

  // tie cuts: the first t sorted positions are the keys below L and then nL copies of L; the
  // last t are nU copies of U and then the keys above U. The kept values are then added in
  // client order from a second read of the column: the tile no longer has that order. (Keeping
  // the K keys in registers instead, with every client loop unrolled, measured the same rate
  // with ten times the code and three times the registers: DESIGN 3l.)
  const int nL = t - below, keepU = cU - (t - above);
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

}  // namespace fjrobust
