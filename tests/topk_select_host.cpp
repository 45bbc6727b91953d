// The digit and scan rules of fedjax_amd/csrc/fjsparse_dev.h built for the host: reads rows, runs
// the three-level select the kernels run (a histogram per level over the keys whose higher digits
// match the prefix, then the walk from the top), and writes the threshold and the sent count raw,
// for tests/test_topk_ref.py to compare with numpy bit for bit. The walk runs twice per level,
// once as a single slice over all bins and once as the device's 256 lane slices with their
// prefix sums; a disagreement between the two is an error (exit 6).
//
// cases file:   int32 n, then per case int32 P, int32 c, uint32 bits[P]
// results file: per case uint32 T, int32 sent, then per level uint32 digit, uint32 rank
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fjsparse_dev.h"

namespace {
template <class T>
bool get(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
template <class T>
void put(FILE* f, const T* p, size_t n) {
  fwrite(p, sizeof(T), n, f);
}

// the device's walk: lane t owns the per bins below nb - 1 - t * per
fjsparse::Pick walk_lanes(const std::vector<uint32_t>& hist, int nb, uint32_t rank) {
  const int lanes = fjsparse::kThreads, per = nb / lanes;
  std::vector<uint32_t> incl(lanes);
  uint32_t run = 0;
  for (int t = 0; t < lanes; ++t) {
    for (int j = 0; j < per; ++j) run += hist[nb - (t + 1) * per + j];
    incl[t] = run;
  }
  fjsparse::Pick out = {0, 0u, 0u, 0u};
  for (int t = 0; t < lanes; ++t) {
    const int lo = nb - (t + 1) * per;
    uint32_t sum = 0;
    for (int j = 0; j < per; ++j) sum += hist[lo + j];
    fjsparse::Pick p = {0, 0u, 0u, 0u};
    fjsparse::scan_slice(hist.data() + lo, per - 1, per, incl[t] - sum, rank, &p);
    if (p.found) {
      if (out.found) return fjsparse::Pick{2, 0u, 0u, 0u};  // two slices claim the rank
      p.digit += (uint32_t)lo;
      out = p;
    }
  }
  return out;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n = 0;
  if (!get(in, &n, 1)) return 3;
  for (int32_t cs = 0; cs < n; ++cs) {
    int32_t head[2];
    if (!get(in, head, 2)) return 3;
    const int32_t P = head[0], c = head[1];
    if (P < 1 || c < 1 || c > P) return 4;
    std::vector<uint32_t> bits((size_t)P);
    if (!get(in, bits.data(), bits.size())) return 3;
    uint32_t prefix = 0, rank = (uint32_t)c, T = 0, trace[2 * fjsparse::kLevels];
    int32_t sent = 0;
    for (int level = 0; level < fjsparse::kLevels; ++level) {
      const int nb = fjsparse::bins(level);
      if (nb > fjsparse::kMaxBins || nb % fjsparse::kThreads) return 5;
      std::vector<uint32_t> hist((size_t)nb, 0u);
      for (uint32_t b : bits) {
        const uint32_t m = fjsparse::key(b);
        if (fjsparse::matches(m, prefix, level)) hist.at(fjsparse::digit(m, level)) += 1;  // .at(): a digit is a bin
      }
      fjsparse::Pick one = {0, 0u, 0u, 0u};
      fjsparse::scan_slice(hist.data(), nb - 1, nb, 0u, rank, &one);
      const fjsparse::Pick many = walk_lanes(hist, nb, rank);
      if (one.found != 1 || many.found != 1 || one.digit != many.digit || one.rank != many.rank || one.ge != many.ge)
        return 6;
      trace[2 * level] = one.digit;
      trace[2 * level + 1] = one.rank;
      if (level < fjsparse::kLevels - 1) {
        prefix = (level ? (prefix << 10) : 0u) | one.digit;
        rank = one.rank;
      } else {
        if (hist[one.digit] != one.ge - (rank - one.rank)) return 6;  // how the kernel recovers the picked bin's count
        T = fjsparse::threshold(prefix, one);
        sent = (int32_t)fjsparse::sent_count((uint32_t)c, rank, T, one, hist[one.digit]);
      }
    }
    put(out, &T, 1);
    put(out, &sent, 1);
    put(out, trace, 2 * fjsparse::kLevels);
  }
  if (fclose(out) != 0) return 5;
  fclose(in);
  return 0;
}
