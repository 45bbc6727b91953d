// fjsparse_dev.h — the digit and scan rules of the top-k radix select (fjsparse.hip) as plain
// C++ that also builds for the host: tests/topk_select_host.cpp runs the same functions level
// by level with g++ and compares them with numpy bit for bit. Internal to the library; the C
// ABI is include/fjcomp.h (fjcomp_topk_*).
//
// The magnitude key of a float32 v is m(v) = bits(v) & 0x7fffffff, compared as uint32:
// |NaN| > inf > finite > subnormal > 0. The threshold T of a row is its c-th largest key. The
// select finds T most-significant digit first, 11 / 10 / 10 bits of the 31-bit key: per level
// one histogram of the digit over the elements whose higher digits equal the prefix chosen so
// far, then a walk of the bins from the top until the running count reaches the remaining rank.
//
// Every count is an integer, so a histogram does not depend on the order its atomic adds
// arrive in: T and the counts are exact and the same on every run. Every bin index is a masked
// digit (digit() below: a shift and an AND with bins - 1), so no value of the data, NaN and inf
// included, can address outside a histogram of bins(level) counters.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FJSPARSE_HD __host__ __device__ inline
#else
#define FJSPARSE_HD inline
#endif

namespace fjsparse {

constexpr int kLevels = 3;
constexpr int kMaxBins = 2048;         // bins of level 0: what one histogram row holds
constexpr int kChunk = 16384;          // elements of one row a histogram workgroup counts
constexpr int kThreads = 256;          // threads of every workgroup here
constexpr int kFoldTile = 1024;        // elements one fold workgroup owns (256 lanes x 4)
constexpr int kMaxClients = 4096;      // the clipped fold's limit

FJSPARSE_HD uint32_t key(uint32_t bits) { return bits & 0x7fffffffu; }
FJSPARSE_HD int shift(int level) { return level == 0 ? 20 : (level == 1 ? 10 : 0); }
FJSPARSE_HD int bins(int level) { return level == 0 ? 2048 : 1024; }
// The bin of key m at `level`: always in [0, bins(level)).
FJSPARSE_HD uint32_t digit(uint32_t m, int level) { return (m >> shift(level)) & (uint32_t)(bins(level) - 1); }
// Whether the digits of m above `level` equal `prefix` (the digits chosen so far, right-aligned;
// level 0 has none and every key matches).
FJSPARSE_HD bool matches(uint32_t m, uint32_t prefix, int level) {
  return level == 0 || (m >> (shift(level) + 10)) == prefix;
}

struct Pick {
  int found;        // 1 once a slice held the rank
  uint32_t digit;   // the chosen bin
  uint32_t rank;    // the rank that remains inside that bin, >= 1
  uint32_t ge;      // elements in bins >= digit
};

// One slice of the walk from the top: bins hi, hi-1, ..., hi-n+1 of `hist`, of which `above`
// elements lie in bins higher than hi. If the running count reaches `rank` inside the slice
// (above < rank <= above + the slice's sum), *p is written. The slices of one histogram
// partition its bins, so exactly one slice writes when 1 <= rank <= the histogram's total.
// The device gives every lane one slice and `above` from a prefix sum of the slice sums; the
// host calls it once over all bins, or slice by slice: the same result.
FJSPARSE_HD void scan_slice(const uint32_t* hist, int hi, int n, uint32_t above, uint32_t rank, Pick* p) {
  uint32_t run = above;
  for (int j = 0; j < n; ++j) {
    const uint32_t h = hist[hi - j];
    if (run < rank && rank <= run + h) {
      p->found = 1;
      p->digit = (uint32_t)(hi - j);
      p->rank = rank - run;
      p->ge = run + h;
    }
    run += h;
  }
}

// After the last level: T is the prefix with the last digit appended, and `sent` counts the
// keys >= max(T, 1). `c` is the keep count, `rank_in` the rank that entered the last level
// (c - rank_in keys lie above the last prefix group), `p` the last level's pick. With T = 0
// the picked bin holds exactly the zeros, which are never sent.
FJSPARSE_HD uint32_t threshold(uint32_t prefix, const Pick& p) { return (prefix << 10) | p.digit; }
FJSPARSE_HD uint32_t sent_count(uint32_t c, uint32_t rank_in, uint32_t T, const Pick& p, uint32_t picked_bin_count) {
  const uint32_t ge = (c - rank_in) + p.ge;
  return T == 0 ? ge - picked_bin_count : ge;
}

}  // namespace fjsparse
