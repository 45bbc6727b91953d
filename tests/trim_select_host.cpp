// Host build of the column rule of fedjax_amd/csrc/fjtrimsel_dev.h for tests/test_trim_select_ref.py: the descent,
// the cuts, the keep rule and the chain the kernels use, with the keys in a plain array and counted by a loop.
// cases:   int32 count, then per case: int32 K, t, P, uint32 scale bits, uint32 x[K][P].
// results: per case uint32 y[P], then uint32 kept[K][P] (1 = client k is kept in column p).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fjtrimsel_dev.h"

static bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static void run_case(int K, int t, int P, uint32_t scale_bits, const uint32_t* x, std::vector<uint32_t>& out) {
  std::vector<uint32_t> key(K), kept_bits(K), mask((size_t)K * P);
  out.assign(P, 0u);
  for (int p = 0; p < P; ++p) {
    for (int k = 0; k < K; ++k) key[k] = fjrobust::key_of(x[(size_t)k * P + p]);
    auto count2 = [&](uint32_t a, uint32_t b, int& na, int& nb) {
      na = nb = 0;
      for (int k = 0; k < K; ++k) na += key[k] < a, nb += key[k] < b;
    };
    auto count_eq = [&](uint32_t u) { int n = 0; for (int k = 0; k < K; ++k) n += key[k] == u; return n; };
    const fjtrimsel::Cuts cuts = fjtrimsel::select_cuts(count2, count_eq, K, t);
    int iL = 0, iU = 0, n = 0;
    for (int k = 0; k < K; ++k) {
      const bool keep = fjtrimsel::kept(key[k], cuts, iL, iU);
      iL += key[k] == cuts.L, iU += key[k] == cuts.U;
      mask[(size_t)k * P + p] = keep;
      if (keep) kept_bits[n++] = fjrobust::bits_of(key[k]);
    }
    if (n != K - 2 * t) abort();  // the cuts keep exactly the ranks t .. K-1-t
    auto at = [&](int j) { if (j < 0 || j >= n) abort(); return kept_bits[j]; };  // never past the kept values
    out[p] = fjtrimsel::chain_sum(at, n, true, fjrobust::as_float(scale_bits));
  }
  out.insert(out.end(), mask.begin(), mask.end());
}

int main(int argc, char** argv) {
  FILE* in = argc == 3 ? fopen(argv[1], "rb") : nullptr;
  FILE* res = in ? fopen(argv[2], "wb") : nullptr;
  if (!res) return 2;
  int32_t count = 0;
  if (!read_all(in, &count, 4) || count < 0) return 3;
  for (int32_t c = 0; c < count; ++c) {
    int32_t h[4];  // K, t, P, scale bits
    if (!read_all(in, h, sizeof(h))) return 3;
    const int K = h[0], t = h[1], P = h[2];
    if (K < 1 || K > fjtrimsel::kMaxClients || t < 0 || 2 * t >= K || P < 1 || P > (1 << 16)) return 4;
    std::vector<uint32_t> x((size_t)K * P), out;
    if (!read_all(in, x.data(), x.size() * 4)) return 3;
    run_case(K, t, P, (uint32_t)h[3], x.data(), out);
    if (fwrite(out.data(), 4, out.size(), res) != out.size()) return 5;
  }
  return fclose(res) == 0 ? 0 : 5;
}
