// FLTrust's selection rule of fedjax_amd/csrc/fjtrust_dev.h built for the host: reads cases, runs
// fltrust_select_host (the pieces the kernel runs, as loops) and the ordered combine, and writes
// every output raw, for tests/test_fltrust_ref.py to compare with numpy bit for bit.
//
// cases file:   int32 n, then per case  int32 K, float q_s, float a[K], float q[K]
// results file: per case  double cos[K], double trust[K], float factors[K], float norms[K],
//               float server_norm, double total, int32 count, int32 order[K], int32 seg[2],
//               float wperm[K], float gscale, float combined (fjtrust::combine of a[0 .. K))
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fjtrust_dev.h"

namespace {
template <class T>
bool get(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
template <class T>
void put(FILE* f, const T* p, size_t n) {
  fwrite(p, sizeof(T), n, f);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n = 0;
  if (!get(in, &n, 1)) return 3;
  for (int32_t c = 0; c < n; ++c) {
    int32_t K = 0;
    float qs = 0;
    if (!get(in, &K, 1) || !get(in, &qs, 1)) return 3;
    if (K < 1 || K > fjtrust::kMaxClients) return 4;
    std::vector<float> a(K), q(K), factors(K), norms(K), wperm(K);
    std::vector<double> cosv(K), trust(K);
    std::vector<int32_t> order(K);
    if (!get(in, a.data(), K) || !get(in, q.data(), K)) return 3;
    int32_t count = 0, seg[2];
    float server_norm = 0, gscale = 0;
    double total = 0;
    fjtrust::fltrust_select_host(a.data(), q.data(), qs, K, cosv.data(), trust.data(), factors.data(), norms.data(),
                                 &server_norm, &total, &count, order.data(), seg, wperm.data(), &gscale);
    const float combined = fjtrust::combine(a.data(), K);
    put(out, cosv.data(), K);
    put(out, trust.data(), K);
    put(out, factors.data(), K);
    put(out, norms.data(), K);
    put(out, &server_norm, 1);
    put(out, &total, 1);
    put(out, &count, 1);
    put(out, order.data(), K);
    put(out, seg, 2);
    put(out, wperm.data(), K);
    put(out, &gscale, 1);
    put(out, &combined, 1);
  }
  if (fclose(out) != 0) return 5;
  fclose(in);
  return 0;
}
