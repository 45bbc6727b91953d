// Host build of the per-column routines of fedjax_amd/csrc/fjrobust_dev.h, for
// tests/test_around_median_ref.py: the same template code the kernels instantiate, run on the
// CPU over cases read from a file, so that the window rule and the tie cuts can be compared
// bitwise with the numpy restatement without a GPU.
//
//   around_median_host <cases> <results>
//
// cases:   int32 count, then per case: int32 mode (0 = mean around the median, 1 = trimmed
//          mean), K, arg (keep count or trim count), P, uint32 scale bits, uint32 x[K][P].
// results: per case, for every width N in {16, 32, 64, 128} with N >= K in that order, uint32 y[P].
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fjrobust_dev.h"

namespace {

template <int N>
void run_case(int mode, int K, int arg, int P, uint32_t scale_bits, const uint32_t* x, std::vector<uint32_t>& out) {
  std::vector<fjrobust::KeyPair> tile(N / 2);
  const float scale = fjrobust::as_float(scale_bits);
  for (int p = 0; p < P; ++p) {
    auto load = [=](int k) { return x[(size_t)k * P + p]; };
    out.push_back(mode == 0 ? fjrobust::around_median_column<N, 1>(load, K, arg, true, scale, tile.data())
                            : fjrobust::trim_column<N, 1>(load, K, arg, true, scale, tile.data()));
  }
}

bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* res = in ? fopen(argv[2], "wb") : nullptr;
  if (!in || !res) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  int32_t count = 0;
  if (!read_all(in, &count, 4) || count < 0) return 3;
  for (int32_t c = 0; c < count; ++c) {
    int32_t h[4];
    uint32_t scale_bits;
    if (!read_all(in, h, sizeof(h)) || !read_all(in, &scale_bits, 4)) return 3;
    const int mode = h[0], K = h[1], arg = h[2], P = h[3];
    const bool arg_ok = mode == 0 ? (arg >= 1 && arg <= K) : (mode == 1 && arg >= 0 && 2 * arg < K);
    if (K < 1 || K > 128 || P < 0 || P > (1 << 20) || !arg_ok) return 4;
    std::vector<uint32_t> x((size_t)K * P), out;
    if (!x.empty() && !read_all(in, x.data(), x.size() * 4)) return 3;
    if (K <= 16) run_case<16>(mode, K, arg, P, scale_bits, x.data(), out);
    if (K <= 32) run_case<32>(mode, K, arg, P, scale_bits, x.data(), out);
    if (K <= 64) run_case<64>(mode, K, arg, P, scale_bits, x.data(), out);
    run_case<128>(mode, K, arg, P, scale_bits, x.data(), out);
    if (!out.empty() && fwrite(out.data(), 4, out.size(), res) != out.size()) return 5;
  }
  fclose(in);
  return fclose(res) == 0 ? 0 : 5;
}
