// fjtrimsel_dev.h — one column of the trimmed mean by rank SELECTION (include/fjagg.h,
// fjagg_trim_select_*): the rule of fjrobust_dev.h's trim_column without its sort, for up to 1024
// clients. Plain C++ that also compiles for the host, so the descent, the cuts and the keep rule
// can be run against the numpy restatement without a GPU; fjtrimsel.hip is its only user in the
// library.
//
// The rule needs five numbers of a column's K keys (fjrobust::key_of): L of rank t, U of rank
// K-1-t, and the counts of keys below L, above U and equal to U. The key of rank r is the
// largest v with |{key < v}| <= r, so it is built from its most significant bit down: bit b is
// set iff the count of keys below (v | 1 << b) is still <= r. Both ranks descend together, one
// bit a step, 32 steps whatever the data (BITS = 16 steps over the 16-bit keys of bfloat16
// values, key16_of below: fjtrimsel16.hip). A step asks only "how many client keys are below
// these two candidates": how the keys are held and counted is the caller's (a wave's registers
// and ballots on the device, a loop on the host). The count that admitted a bit is the count
// below the prefix so far, so the descent ends with |{key < L}| and |{key < U}| in hand; one
// more question, |{key == U}|, completes the five. No question can count a slot that holds no
// client: the caller counts by client index, and 0xFFFFFFFF, a legal key, needs no special case.
#pragma once
#include <stdint.h>

#include "fjrobust_dev.h"

namespace fjtrimsel {

constexpr int kMaxClients = 1024;

// what the kept sum needs of a column: the two keys and the tie cuts of fjrobust::kept_sum
struct Cuts {
  uint32_t L, U;
  int nL;     // the first nL clients (in client order) with key L are trimmed
  int keepU;  // the first keepU clients with key U are kept
};

// count2(a, b, na, nb): na = clients with key < a, nb = clients with key < b.
// count_eq(u): clients with key == u. 1 <= K, 0 <= 2t < K. Every key is below 2^BITS.
template <int BITS = 32, class Count2, class CountEq>
FJR_HD Cuts select_cuts(Count2 count2, CountEq count_eq, int K, int t) {
  const int rl = t, ru = K - 1 - t;
  uint32_t L = 0, U = 0;
  int belowL = 0, belowU = 0;
#pragma unroll 1
  for (int b = BITS - 1; b >= 0; --b) {
    const uint32_t cl = L | (1u << b), cu = U | (1u << b);
    int nl, nu;
    count2(cl, cu, nl, nu);
    const bool tl = nl <= rl, tu = nu <= ru;
    L = tl ? cl : L;
    belowL = tl ? nl : belowL;
    U = tu ? cu : U;
    belowU = tu ? nu : belowU;
  }
  const int cU = count_eq(U);
  const int above = K - belowU - cU;
  // fjrobust::trim_column's cuts, unchanged: the first t sorted positions are the keys below L
  // and then nL copies of L; the last t are nU = t - above copies of U and then the keys above U
  return Cuts{L, U, t - belowL, cU - (t - above)};
}

// fjrobust::kept_sum's keep rule for the client whose key is `key`, the iL-th (from 0) in client
// order with key L and the iU-th with key U
FJR_HD bool kept(uint32_t key, const Cuts& c, int iL, int iU) {
  const bool isL = key == c.L, isU = key == c.U;
  return key >= c.L && key <= c.U && (!isL || iL >= c.nL) && (!isU || iU < c.keepU);
}

// The 16-bit key of a bfloat16 value's bits b: the top half of fjrobust::key_of(b << 16), whose low
// half (0xFFFF or 0x0000) depends on the sign alone, so keys of bfloat16 values compare as their
// top halves do and tie exactly when the values' bits are equal. Zero-extended in a uint32.
FJR_HD uint32_t key16_of(uint32_t b) { return b ^ ((b >> 15) ? 0xFFFFu : 0x8000u); }
// its inverse, shifted into place: the float32 bits of the bfloat16 value whose key is k
FJR_HD uint32_t float_bits_of_key16(uint32_t k) { return (k ^ ((k >> 15) ? 0x8000u : 0xFFFFu)) << 16; }

// fl(s + x) with the running sum as the instruction's FIRST operand. IEEE leaves open which
// payload a sum of two NaNs carries; the hardware takes the first operand's, and the compiler is
// free to commute a plain add. fjagg_trim_*'s kernels add with the sum first, so this pins the
// same order: the contract's "bit for bit, NaN payloads included" for K <= 128.
FJR_HD float add_sum_first(float s, float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(s), "v"(x));
  return r;
#else
  return s + x;
#endif
}

// The sum of n >= 1 kept values given in client order: the first verbatim, then fl(s + v), then
// the scale. at(j) returns the float bits of the j-th kept value; the reads of a step of 16 are
// issued before its adds.
template <class At>
FJR_HD uint32_t chain_sum(At at, int n, bool do_scale, float scale) {
  float s = fjrobust::as_float(at(0));
#pragma unroll 1
  for (int j0 = 1; j0 < n; j0 += 16) {
    uint32_t v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = at(j0 + j < n ? j0 + j : n - 1);  // past the end: read again, not added
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float sum = add_sum_first(s, fjrobust::as_float(v[j]));
      s = j0 + j < n ? sum : s;
    }
  }
  return fjrobust::as_bits(do_scale ? fjrobust::mul_rn(s, scale) : s);
}

}  // namespace fjtrimsel
