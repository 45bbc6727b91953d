// The selection rules of fedjax_amd/csrc/fjselect_dev.h built for the host: reads cases, runs
// krum_scores_host + krum_rank_host / weiszfeld_select_host (the pieces the kernels run, as loops)
// and writes every output raw, for tests/test_select_device_ref.py to compare with numpy bit for bit.
//
// cases file:   int32 n, then per case
//     int32 mode (0 Krum, 1 Weiszfeld), int32 K, int32 a, int32 b, double nu, double G[K*K], and with
//     mode 1 and a != 0: double alpha[K].   Krum: a = f, b = m.  Weiszfeld: a = has_alpha, b = iterations.
//     A Krum case with K < 0 reuses the scores of the case before it (the same G and f, another m):
//     -K is K, and no G follows.
// results file: per case
//     Krum:      double scores[K], int64 selected[m], int32 count, int32 order[m], int32 seg[2],
//                float wperm[m], float gscale
//     Weiszfeld: double a[K], double d[K], float a32[K], int32 count, int32 order[K], int32 seg[2],
//                float wperm[K], float gscale
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
  std::vector<double> scores;  // of the latest Krum case that brought a G
  for (int32_t c = 0; c < n; ++c) {
    int32_t head[4];
    double nu = 0;
    if (!get(in, head, 4) || !get(in, &nu, 1)) return 3;
    const int mode = head[0], a = head[2], b = head[3];
    const bool again = mode == 0 && head[1] < 0;
    const int K = again ? -head[1] : head[1];
    if (K < 1 || K > fjselect::kMaxClients) return 4;
    if (again && (int)scores.size() != K) return 4;
    std::vector<double> G(again ? 0 : (size_t)K * K), alpha;
    if (!get(in, G.data(), G.size())) return 3;
    int32_t count = 0, seg[2];
    float gscale = 0;
    if (mode == 0) {
      const int f = a, m = b;
      if (f < 0 || K < 2 * f + 3 || m < 1 || m > K - f) return 4;
      if (!again) {
        std::vector<uint64_t> keys(fjselect::pow2_at_least(K));
        scores.assign(K, 0.0);
        fjselect::krum_scores_host(G.data(), K, f, keys.data(), scores.data());
      }
      std::vector<int64_t> selected(m);
      std::vector<int32_t> order(m);
      std::vector<float> wperm(m);
      fjselect::krum_rank_host(scores.data(), K, m, selected.data(), &count, order.data(), seg, wperm.data(), &gscale);
      put(out, scores.data(), K);
      put(out, selected.data(), m);
      put(out, &count, 1);
      put(out, order.data(), m);
      put(out, seg, 2);
      put(out, wperm.data(), m);
      put(out, &gscale, 1);
    } else {
      if (a) {
        alpha.resize(K);
        if (!get(in, alpha.data(), K)) return 3;
      }
      if (b < 0) return 4;
      std::vector<double> av(K), d(K);
      std::vector<float> a32(K), wperm(K);
      std::vector<int32_t> order(K);
      fjselect::weiszfeld_select_host(G.data(), K, a ? alpha.data() : nullptr, nu, b, av.data(), d.data(), a32.data(),
                                      &count, order.data(), seg, wperm.data(), &gscale);
      put(out, av.data(), K);
      put(out, d.data(), K);
      put(out, a32.data(), K);
      put(out, &count, 1);
      put(out, order.data(), K);
      put(out, seg, 2);
      put(out, wperm.data(), K);
      put(out, &gscale, 1);
    }
  }
  if (fclose(out) != 0) return 5;
  fclose(in);
  return 0;
}
