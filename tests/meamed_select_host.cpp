// Host build of the column rule of fedjax_amd/csrc/fjmeamedsel_dev.h for tests/test_meamed_select_ref.py: the three
// descents, the cuts, the keep rule and the chain the kernels use, with the keys in plain arrays counted by loops.
// cases:   int32 count, then per case: int32 K, beta, P, uint32 scale bits, uint32 x[K][P].
// results: per case uint32 a[P] (the window's start), y[P], then kept[K][P] (1 = client k is kept in column p).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fjmeamedsel_dev.h"

struct HostColumn {
  std::vector<uint32_t> key, sided;
  static int below(const std::vector<uint32_t>& r, uint32_t v) { int n = 0; for (uint32_t e : r) n += e < v; return n; }
  static int equal(const std::vector<uint32_t>& r, uint32_t v) { int n = 0; for (uint32_t e : r) n += e == v; return n; }
  int keys_below(uint32_t v) const { return below(key, v); }
  void keys_below2(uint32_t a, uint32_t b, int& na, int& nb) const { na = below(key, a), nb = below(key, b); }
  int keys_equal(uint32_t v) const { return equal(key, v); }
  void place(uint32_t med_key) {
    const float med = fjrobust::as_float(fjrobust::bits_of(med_key));
    sided.resize(key.size());
    for (size_t k = 0; k < key.size(); ++k) sided[k] = fjmeamedsel::sided_distance(key[k], med_key, med);
  }
  void sided_below2(uint32_t a, uint32_t b, int& na, int& nb) const { na = below(sided, a), nb = below(sided, b); }
  int sided_equal(uint32_t v) const { return equal(sided, v); }
};

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static void run_case(int K, int beta, int P, uint32_t scale_bits, const uint32_t* x, std::vector<uint32_t>& out) {
  std::vector<uint32_t> kept_bits(K), y(P), mask((size_t)K * P);
  HostColumn col;
  col.key.resize(K);
  out.assign(P, 0u);
  for (int p = 0; p < P; ++p) {
    for (int k = 0; k < K; ++k) col.key[k] = fjrobust::key_of(x[(size_t)k * P + p]);
    int a = -1;
    const fjtrimsel::Cuts cuts = fjmeamedsel::window_cuts(col, K, beta, &a);
    if (a < 0 || a + beta > K) abort();
    out[p] = (uint32_t)a;
    int iL = 0, iU = 0, n = 0;
    for (int k = 0; k < K; ++k) {
      const bool keep = fjtrimsel::kept(col.key[k], cuts, iL, iU);
      iL += col.key[k] == cuts.L, iU += col.key[k] == cuts.U;
      mask[(size_t)k * P + p] = keep;
      if (keep) kept_bits[n++] = fjrobust::bits_of(col.key[k]);
    }
    if (n != beta) abort();  // the cuts keep exactly the ranks a .. a + beta - 1
    auto at = [&](int j) { if (j < 0 || j >= n) abort(); return kept_bits[j]; };  // never past the kept values
    y[p] = fjtrimsel::chain_sum(at, n, true, fjrobust::as_float(scale_bits));
  }
  out.insert(out.end(), y.begin(), y.end());
  out.insert(out.end(), mask.begin(), mask.end());
}

int main(int argc, char** argv) {
  FILE* in = argc == 3 ? fopen(argv[1], "rb") : nullptr;
  FILE* res = in ? fopen(argv[2], "wb") : nullptr;
  if (!res) return 2;
  int32_t count = 0;
  if (!read_all(in, &count, 4) || count < 0) return 3;
  for (int32_t c = 0; c < count; ++c) {
    int32_t h[4];  // K, beta, P, scale bits
    if (!read_all(in, h, sizeof(h))) return 3;
    const int K = h[0], beta = h[1], P = h[2];
    if (K < 1 || K > fjmeamedsel::kMaxClients || beta < 1 || beta > K || P < 1 || P > (1 << 16)) return 4;
    std::vector<uint32_t> x((size_t)K * P), out;
    if (!read_all(in, x.data(), x.size() * 4)) return 3;
    run_case(K, beta, P, (uint32_t)h[3], x.data(), out);
    if (fwrite(out.data(), 4, out.size(), res) != out.size()) return 5;
  }
  return fclose(res) == 0 ? 0 : 5;
}
