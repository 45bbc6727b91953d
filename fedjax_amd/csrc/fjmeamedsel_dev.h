// fjmeamedsel_dev.h — one column of the mean around the median by rank SELECTION (include/fjagg.h,
// fjagg_meamed_select_*): the rule of fjrobust_dev.h's around_median_column without its
// sort, for up to 1024 participating clients. Plain C++ that also compiles for the host, so the
// three descents can be run against the numpy restatement without a GPU; fjmeamedsel.hip is its only
// user in the library.
//
// A column is K keys (fjrobust::key_of), mid = (K-1)/2, keep count beta. The sorted positions are
// never formed; what is known of them comes from counts.
//   1. med, the key of rank mid, by fjtrimsel_dev.h's bit descent with one rank. With below =
//      |{key < med}| and cM = |{key == med}|, the positions below mid hold the keys < med and then
//      e_lo = mid - below copies of med; the positions above it hold e_hi = cM - 1 - e_lo copies
//      and then the keys > med.
//   2. Every client gets one word, its SIDED DISTANCE: d = fjrobust::distance_of (the bits of a
//      non-negative float32, which order as unsigned integers, <= 0x7F800000) for a key < med,
//      d | 1 << 31 for a key > med, and kNoSide for med's own copies, whose distance is 0 and
//      whose side is a matter of e_lo and e_hi. "How many positions of the lower side are closer
//      than D" is then |{word < D}| + (D > 0 ? e_lo : 0), and of the upper side |{word < (D |
//      1 << 31)}| - below + (D > 0 ? e_hi : 0): the same question the key descent asks, of other
//      words. The distance falls towards mid from below and rises above it (rounding is monotone,
//      the specials land on 0 or +inf), so the greedy of the specification keeps mid and the
//      beta - 1 first of the other K - 1 positions in the order (distance, lower side first). D*,
//      the distance of rank beta - 2 among them, is found by a second descent over the 31 distance
//      bits; the places left after the positions closer than D* go to the lower side's ties first.
//      With n_lo kept lower positions the window starts at a = mid - n_lo.
//   3. L of rank a and U of rank a + beta - 1 by the two-rank descent, and fjrobust::kept_sum's tie
//      cuts with the two trim counts a and K - beta - a.
// The kept values are then fjtrimsel's: kept(), compaction in client order, chain_sum().
#pragma once
#include <stdint.h>

#include "fjtrimsel_dev.h"

namespace fjmeamedsel {

constexpr int kMaxClients = fjtrimsel::kMaxClients;
constexpr uint32_t kUpper = 0x80000000u;   // the side bit of a sided distance
constexpr uint32_t kNoSide = 0xFFFFFFFFu;  // a copy of the median: above every sided distance

// the word of step 2 for a client's key
FJR_HD uint32_t sided_distance(uint32_t key, uint32_t med_key, float med) {
  const uint32_t d = fjrobust::distance_of(key, med_key, med);
  return key == med_key ? kNoSide : (key > med_key ? d | kUpper : d);
}

// What a caller provides (a wave's registers and ballots on the device, loops on the host):
//   col.keys_below(v)                  clients with key < v
//   col.keys_below2(a, b, na, nb)      na = clients with key < a, nb = clients with key < b
//   col.keys_equal(v)                  clients with key == v
//   col.place(med_key)                 form every client's sided distance from med_key
//   col.sided_below2(a, b, na, nb)     the same counts over the sided distances
//   col.sided_equal(v)
// No question can count a slot that holds no client: the caller counts by client index.

// The key of rank r (0 <= r < K) and the number of keys below it: select_cuts' descent, one rank.
template <class Col>
FJR_HD uint32_t select_rank(Col& col, int r, int& below) {
  uint32_t v = 0;
  below = 0;
#pragma unroll 1
  for (int b = 31; b >= 0; --b) {
    const uint32_t c = v | (1u << b);
    const int n = col.keys_below(c);
    const bool t = n <= r;
    v = t ? c : v;
    below = t ? n : below;
  }
  return v;
}

// select_cuts' descent for two arbitrary ranks 0 <= rl <= ru < K, trimming tl positions below
// rank rl and tu above rank ru (tl = rl and tu = K - 1 - ru: the cuts are the trimmed mean's with
// two trim counts).
template <class Col>
FJR_HD fjtrimsel::Cuts select_cuts2(Col& col, int K, int rl, int ru) {
  uint32_t L = 0, U = 0;
  int belowL = 0, belowU = 0;
#pragma unroll 1
  for (int b = 31; b >= 0; --b) {
    const uint32_t cl = L | (1u << b), cu = U | (1u << b);
    int nl, nu;
    col.keys_below2(cl, cu, nl, nu);
    const bool tl = nl <= rl, tu = nu <= ru;
    L = tl ? cl : L;
    belowL = tl ? nl : belowL;
    U = tu ? cu : U;
    belowU = tu ? nu : belowU;
  }
  const int cU = col.keys_equal(U);
  const int above = K - belowU - cU;
  return fjtrimsel::Cuts{L, U, rl - belowL, cU - ((K - 1 - ru) - above)};
}

// Steps 1 and 2: the first kept sorted position. 1 <= beta <= K. Leaves the sided distances placed.
template <class Col>
FJR_HD int window_start(Col& col, int K, int beta) {
  const int mid = (K - 1) >> 1;
  if (beta == 1) return mid;
  int below;
  const uint32_t med = select_rank(col, mid, below);
  const int e_lo = mid - below, e_hi = col.keys_equal(med) - 1 - e_lo;
  col.place(med);
  // D* of rank beta - 2 among the K - 1 other positions, the counts below it a side. Bit 31 is the
  // side, and no distance is above +inf's bits, so 31 steps.
  const int rank = beta - 2;
  uint32_t D = 0;
  int lt_lo = 0, lt_hi = 0;
#pragma unroll 1
  for (int b = 30; b >= 0; --b) {
    const uint32_t c = D | (1u << b);  // > 0: the median's copies are closer on both sides
    int nlo, nup;
    col.sided_below2(c, c | kUpper, nlo, nup);  // nup counts the whole lower side too
    const int lo = nlo + e_lo, hi = nup - below + e_hi;
    const bool t = lo + hi <= rank;
    D = t ? c : D;
    lt_lo = t ? lo : lt_lo;
    lt_hi = t ? hi : lt_hi;
  }
  const int eq_lo = col.sided_equal(D) + (D == 0 ? e_lo : 0);
  const int left = beta - 1 - lt_lo - lt_hi;  // >= 1: the position of rank beta - 2 is at D* itself
  return mid - (lt_lo + (left < eq_lo ? left : eq_lo));
}

// The whole rule up to the cuts; *start receives a.
template <class Col>
FJR_HD fjtrimsel::Cuts window_cuts(Col& col, int K, int beta, int* start) {
  const int a = window_start(col, K, beta);
  *start = a;
  return select_cuts2(col, K, a, a + beta - 1);
}

}  // namespace fjmeamedsel
