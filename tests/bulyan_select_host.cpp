// Bulyan's first stage of fedjax_amd/csrc/fjselect_dev.h built for the host: reads cases, runs
// bulyan_select_host (the pieces the two kernels run, as loops) and writes every output raw, for
// tests/test_bulyan_select_ref.py to compare with numpy bit for bit.
//
// cases file:   int32 n, then per case int32 K, int32 f, double G[K*K]
// results file: per case, with theta = K - 2f: int64 selected[theta], int32 count,
//               double step_scores[theta], int32 keep, float scale, int32 rows[theta]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fjselect_dev.h"

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
    int32_t head[2];
    if (!get(in, head, 2)) return 3;
    const int K = head[0], f = head[1];
    // what fjagg_bulyan_select refuses
    if (f < 0 || K < 4 * f + 3 || K > fjselect::kBulyanMaxClients || K - 2 * f > fjselect::kBulyanMaxSelected)
      return 4;
    const int theta = K - 2 * f;
    std::vector<double> G((size_t)K * K), step_scores(theta);
    if (!get(in, G.data(), G.size())) return 3;
    // exactly the workspace the entry asks for: a walk past it is the sanitizer's to report
    std::vector<uint64_t> skeys((size_t)K * (K - 1));
    std::vector<uint8_t> sidx((size_t)K * (K - 1));
    std::vector<int64_t> selected(theta);
    std::vector<int32_t> rows(theta);
    int32_t count = 0, keep = 0;
    float scale = 0;
    fjselect::bulyan_select_host(G.data(), K, f, skeys.data(), sidx.data(), selected.data(), &count,
                                 step_scores.data(), &keep, &scale, rows.data());
    put(out, selected.data(), theta);
    put(out, &count, 1);
    put(out, step_scores.data(), theta);
    put(out, &keep, 1);
    put(out, &scale, 1);
    put(out, rows.data(), theta);
  }
  if (fclose(out) != 0) return 5;
  fclose(in);
  return 0;
}
