// Host build of the bucket adaptor of fedjax_amd/csrc/fjrobust_dev.h over trim_column, for
// tests/test_bucket_ref.py: the same template code the kernels instantiate, run on the CPU over
// cases read from a file, so that the bucket means, the clamp and the trim rule over them can be
// compared bitwise with the numpy restatement without a GPU.
//
//   bucket_column_host <cases> <results>
//   bucket_column_host clamp <i> <K>      prints clamp_index(i, K)
//
// cases:   int32 count, then per case: int32 K, s, t, P, has_perm, uint32 scale bits, uint32
//          inv_s bits, uint32 inv_last bits, int32 perm[K] if has_perm, uint32 x[K][P].
// results: per case, for every width N in {16, 32, 64, 128} with N >= B in that order, uint32 y[P].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fjrobust_dev.h"

namespace {

template <int N>
void run_case(int K, int s, int t, int P, const int32_t* perm, uint32_t scale_bits, uint32_t inv_s, uint32_t inv_last,
              const uint32_t* x, std::vector<uint32_t>& out) {
  std::vector<fjrobust::KeyPair> tile(N / 2);
  const int B = (K + s - 1) / s;
  for (int p = 0; p < P; ++p) {
    auto load = [=](int k) {
      if (k < 0 || k >= K) abort();  // the adaptor must never ask for a client outside the slab
      return x[(size_t)k * P + p];
    };
    auto table = [=](int m) {
      if (m < 0 || m >= K) abort();  // nor for an entry outside the table
      return perm ? perm[m] : (int32_t)m;
    };
    auto bucket = fjrobust::bucket_load(load, table, K, s, fjrobust::as_float(inv_s), fjrobust::as_float(inv_last));
    out.push_back(fjrobust::trim_column<N, 1>(bucket, B, t, true, fjrobust::as_float(scale_bits), tile.data()));
  }
}

bool read_all(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "clamp") == 0) {
    printf("%d\n", fjrobust::clamp_index((int32_t)strtoll(argv[2], nullptr, 10), (int)strtol(argv[3], nullptr, 10)));
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s <cases> <results> | clamp <i> <K>\n", argv[0]);
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
    int32_t h[5];
    uint32_t f[3];
    if (!read_all(in, h, sizeof(h)) || !read_all(in, f, sizeof(f))) return 3;
    const int K = h[0], s = h[1], t = h[2], P = h[3], has_perm = h[4];
    if (K < 1 || K > 4096 || s < 1 || s > K || P < 0 || P > (1 << 20)) return 4;
    const int B = (K + s - 1) / s;
    if (B > 128 || t < 0 || 2 * t >= B) return 4;
    std::vector<int32_t> perm(has_perm ? K : 0);
    if (has_perm && !read_all(in, perm.data(), perm.size() * 4)) return 3;
    std::vector<uint32_t> x((size_t)K * P), out;
    if (!x.empty() && !read_all(in, x.data(), x.size() * 4)) return 3;
    const int32_t* pt = has_perm ? perm.data() : nullptr;
    if (B <= 16) run_case<16>(K, s, t, P, pt, f[0], f[1], f[2], x.data(), out);
    if (B <= 32) run_case<32>(K, s, t, P, pt, f[0], f[1], f[2], x.data(), out);
    if (B <= 64) run_case<64>(K, s, t, P, pt, f[0], f[1], f[2], x.data(), out);
    run_case<128>(K, s, t, P, pt, f[0], f[1], f[2], x.data(), out);
    if (!out.empty() && fwrite(out.data(), 4, out.size(), res) != out.size()) return 5;
  }
  fclose(in);
  return fclose(res) == 0 ? 0 : 5;
}
