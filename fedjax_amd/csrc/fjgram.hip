// fjgram.hip — the K x K Gram matrix G[i][j] = <x_i, x_j> of the client deltas, in float64
// (include/fjagg.h: fjagg_gram_dense, fjagg_gram_ptrs). Krum (Blanchard et al., NeurIPS 2017)
// and the smoothed-Weiszfeld geometric median (Pillutla et al., IEEE TSP 2022) are functions of
// G alone (fedjax_amd/robust.py), so one pass over the deltas serves both.
//
// The pass is X * X^T, on the exact f32-input matrix instruction v_mfma_f32_32x32x2_f32: per
// pair (i, j) a k-ordered fmaf chain. A 256-lane workgroup owns one 128 x 128 block of G (a pair
// of 128-row panels I <= J) over one chunk of columns; each of its four waves owns a 64 x 64
// quadrant as four 32 x 32 accumulators. The columns go through LDS in slabs of kBK, two
// buffers, the next slab's global loads in flight while the current one is multiplied. Every
// FJAGG_GRAM_CHAIN columns (and at the end of a leaf's range) the f32 accumulators are added
// into float64 registers and zeroed; a chunk's float64 block goes to the workspace, and
// k_gram_combine adds the chunks in chunk order and mirrors the lower triangle. No atomics: the
// order of every addition is a function of (K, P) or of the plan.
//
// Rows past K and columns past a range's end are zeros written into LDS, never loaded.
// Loads are 4 bytes wide, so float32's own alignment is all a row or a leaf needs: the pass is
// bound by the matrix unit (K = 128: 64 FLOP per byte loaded, about three times the ratio of the
// instruction's peak to the HBM rate), not by its loads.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "fjagg.h"

extern __attribute__((visibility("hidden"))) __thread char fjagg_g_err[512];
#define g_err fjagg_g_err

namespace {

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FJAGG_EHIP, "%s: %s", what, hipGetErrorString(e));
  return FJAGG_OK;
}

constexpr int64_t kMaxRowBytes = 1ll << 30;
constexpr int kMaxClients = 1024;
constexpr int kPanel = 128;               // rows of G per workgroup block side
constexpr int kBK = 16;                   // columns per LDS slab
constexpr int kPitch = kBK + 1;           // odd: 32 rows at one column fall into 32 banks
constexpr int kSlabsPerChain = FJAGG_GRAM_CHAIN / kBK;
constexpr int kPanelWords = kPanel * kPitch;
// The split into chunks is a function of (K, P) alone (not of the device), so the order of the
// float64 additions is too: about kTasks workgroups over all panel pairs, a chunk never under
// kMinChunkChains chains (a chunk's 128 KiB block of partial sums is written once per chunk).
constexpr int64_t kTasks = 512;
constexpr int64_t kMinChunkChains = 4;
static_assert(FJAGG_GRAM_CHAIN % kBK == 0 && kBK % 2 == 0, "a chain is whole slabs, a slab whole k-pairs");

typedef float f32x16 __attribute__((ext_vector_type(16)));

int64_t panels_of(int64_t K) { return (K + kPanel - 1) / kPanel; }
int64_t pairs_of(int64_t K) { const int64_t n = panels_of(K); return n * (n + 1) / 2; }
int64_t chunk_target(int64_t K) { const int64_t t = kTasks / pairs_of(K); return t < 1 ? 1 : t; }

// columns per workgroup chunk of the dense pass
int64_t dense_chunk_cols(int64_t K, int64_t P) {
  const int64_t nchains = (P + FJAGG_GRAM_CHAIN - 1) / FJAGG_GRAM_CHAIN, tgt = chunk_target(K);
  int64_t cpc = (nchains + tgt - 1) / tgt;
  if (cpc < kMinChunkChains) cpc = kMinChunkChains;
  return cpc * FJAGG_GRAM_CHAIN;
}
int64_t ptrs_chunks(int64_t K, int64_t nblk) { const int64_t t = chunk_target(K); return nblk < t ? nblk : t; }

struct DenseSrc {
  const float* x;
  int64_t ld;
  __device__ const float* row(int r, int) const { return x + (int64_t)r * ld; }
};
struct PtrsSrc {
  const int64_t* in_ptrs;
  int L;
  __device__ const float* row(int r, int leaf) const {
    return reinterpret_cast<const float*>(in_ptrs[(int64_t)r * L + leaf]);
  }
};

struct Tile {
  f32x16 acc[4];      // quadrant blocks (a0,b0) (a0,b1) (a1,b0) (a1,b1), one chain's f32 sums
  double sum[4][16];  // the chains added up
  bool on[4];         // a block with a row or a column past K is never multiplied
};

__device__ __forceinline__ void fold_chain(Tile& t) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      t.sum[a][r] += (double)t.acc[a][r];
      t.acc[a][r] = 0.0f;
    }
}

// Columns [e0, e1) of one leaf (or of the dense rows): chains of FJAGG_GRAM_CHAIN columns from
// e0. rowA0 / rowB0: first client of the two panels; diag: they are the same panel, staged once.
template <class Src>
__device__ __forceinline__ void gram_range(const Src& src, int leaf, int K, int rowA0, int rowB0, bool diag,
                                           int64_t e0, int64_t e1, float* lds, Tile& t) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int scol = tid & (kBK - 1), srow = tid / kBK;  // staging: 16 rows x kBK columns a pass
  constexpr int kPasses = kPanel / (256 / kBK);
  const float* pa[kPasses];
  const float* pb[kPasses];
#pragma unroll
  for (int i = 0; i < kPasses; ++i) {
    const int ra = rowA0 + srow + i * (256 / kBK), rb = rowB0 + srow + i * (256 / kBK);
    pa[i] = ra < K ? src.row(ra, leaf) : nullptr;
    pb[i] = (!diag && rb < K) ? src.row(rb, leaf) : nullptr;
  }
  float va[kPasses], vb[kPasses];
  auto fetch = [&](int64_t s) {
    const int64_t c = e0 + s * kBK + scol;
    const bool ok = c < e1;
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
      va[i] = (ok && pa[i]) ? pa[i][c] : 0.0f;
      vb[i] = (ok && pb[i]) ? pb[i][c] : 0.0f;
    }
  };
  auto stage = [&](int buf) {
    float* sa = lds + buf * 2 * kPanelWords;
    float* sb = sa + kPanelWords;
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
      const int o = (srow + i * (256 / kBK)) * kPitch + scol;
      sa[o] = va[i];
      if (!diag) sb[o] = vb[i];
    }
  };
  const int64_t ns = (e1 - e0 + kBK - 1) / kBK;
  if (ns <= 0) return;
  // lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: with B = A^T both are
  // X[block row + (l & 31)][column + (l >> 5)]
  const int fa = ((wave >> 1) * 64 + (lane & 31)) * kPitch + (lane >> 5);
  const int fb = ((wave & 1) * 64 + (lane & 31)) * kPitch + (lane >> 5);
  fetch(0);
  stage(0);
  __syncthreads();
  for (int64_t s = 0; s < ns; ++s) {
    const int buf = (int)(s & 1);
    if (s + 1 < ns) fetch(s + 1);
    const float* sa = lds + buf * 2 * kPanelWords;
    const float* sb = diag ? sa : sa + kPanelWords;
    auto multiply = [&](auto full) {  // full: all four blocks on, no branch between the MFMAs
#pragma unroll
      for (int kk = 0; kk < kBK; kk += 2) {
        const float a0 = sa[fa + kk], a1 = sa[fa + 32 * kPitch + kk];
        const float b0 = sb[fb + kk], b1 = sb[fb + 32 * kPitch + kk];
        if (full.value || t.on[0]) t.acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, t.acc[0], 0, 0, 0);
        if (full.value || t.on[1]) t.acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, t.acc[1], 0, 0, 0);
        if (full.value || t.on[2]) t.acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, t.acc[2], 0, 0, 0);
        if (full.value || t.on[3]) t.acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, t.acc[3], 0, 0, 0);
      }
    };
    if (t.on[3]) multiply(std::true_type{});  // (a1, b1) on: so are the other three
    else multiply(std::false_type{});
    if ((s + 1) % kSlabsPerChain == 0 || s + 1 == ns) fold_chain(t);
    if (s + 1 < ns) stage(buf ^ 1);
    __syncthreads();  // slab s+1 is staged; nobody still reads slab s
  }
}

__device__ __forceinline__ void pair_of(int pair, int npanels, int& I, int& J) {
  int i = 0;
  while (pair >= npanels - i) {
    pair -= npanels - i;
    ++i;
  }
  I = i;
  J = i + pair;
}

__device__ __forceinline__ void tile_init(Tile& t, int K, int rowA0, int rowB0) {
  const int wave = threadIdx.x >> 6;
  const int ra = rowA0 + (wave >> 1) * 64, rb = rowB0 + (wave & 1) * 64;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    t.on[a] = ra + (a >> 1) * 32 < K && rb + (a & 1) * 32 < K;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      t.acc[a][r] = 0.0f;
      t.sum[a][r] = 0.0;
    }
  }
}

// The workgroup's 128 x 128 float64 block: C/D map col = lane & 31, row = (reg & 3) + 8 * (reg >> 2)
// + 4 * (lane >> 5) within each 32 x 32 block.
__device__ __forceinline__ void tile_store(const Tile& t, double* blk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int r0 = (wave >> 1) * 64 + (a >> 1) * 32 + 4 * (lane >> 5);
    const int c = (wave & 1) * 64 + (a & 1) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) blk[(r0 + (r & 3) + 8 * (r >> 2)) * kPanel + c] = t.sum[a][r];
  }
}

// grid (chunks, pairs); ws[chunk][pair][128][128] float64
__global__ __launch_bounds__(256) void k_gram_dense(const float* __restrict__ x, int64_t ld, int K, int64_t P,
                                                    int64_t chunk_cols, int npanels, double* __restrict__ ws) {
  __shared__ float lds[2 * 2 * kPanelWords];
  int I, J;
  pair_of(blockIdx.y, npanels, I, J);
  Tile t;
  tile_init(t, K, I * kPanel, J * kPanel);
  const int64_t e0 = (int64_t)blockIdx.x * chunk_cols;
  const int64_t e1 = e0 + chunk_cols < P ? e0 + chunk_cols : P;
  gram_range(DenseSrc{x, ld}, 0, K, I * kPanel, J * kPanel, I == J, e0, e1, lds, t);
  tile_store(t, ws + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (kPanel * kPanel));
}

// Pytree path: chunk blockIdx.x walks the plan entries [b0, b1) of the image (fjrobust.hip
// k_trim_ptrs decodes an entry the same way), each a column range of one leaf.
__global__ __launch_bounds__(256) void k_gram_ptrs(const int64_t* __restrict__ img, int L, int K, int V, int64_t nblk,
                                                   int npanels, double* __restrict__ ws) {
  __shared__ float lds[2 * 2 * kPanelWords];
  int I, J;
  pair_of(blockIdx.y, npanels, I, J);
  Tile t;
  tile_init(t, K, I * kPanel, J * kPanel);
  const int64_t* leaf_n = img + (int64_t)K * L + L;
  const int64_t* blocks = leaf_n + L;
  const int64_t b0 = (int64_t)blockIdx.x * nblk / gridDim.x, b1 = ((int64_t)blockIdx.x + 1) * nblk / gridDim.x;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t be = blocks[2 * b];
    const int leaf = (int)((be >> 40) & 0x3fffff);
    const bool tail = (be >> 62) & 1;
    const bool elem = ((uint64_t)be >> 63) != 0;
    const int64_t u0 = be & ((1ll << 40) - 1), u1 = blocks[2 * b + 1];
    const int64_t n = leaf_n[leaf];
    const int64_t e0 = tail ? n / V * V : (elem ? u0 : u0 * V);
    int64_t e1 = tail ? n : (elem ? u1 : u1 * V);
    if (e1 > n) e1 = n;
    gram_range(PtrsSrc{img, L}, leaf, K, I * kPanel, J * kPanel, I == J, e0, e1, lds, t);
  }
  tile_store(t, ws + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (kPanel * kPanel));
}

// G[i][j] = the chunks' partial sums added in chunk order. Pairs hold I <= J only: an entry below
// the diagonal panels reads its mirror image, which is the same sum of the same products.
__global__ __launch_bounds__(256) void k_gram_combine(const double* __restrict__ ws, int K, int nchunks, int npanels,
                                                      double* __restrict__ gram) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)K * K) return;
  int i = (int)(idx / K), j = (int)(idx % K);
  if (i / kPanel > j / kPanel) {
    const int s = i;
    i = j;
    j = s;
  }
  const int I = i / kPanel, J = j / kPanel;
  const int64_t pair = (int64_t)I * npanels - (int64_t)I * (I - 1) / 2 + (J - I);
  const int64_t npairs = (int64_t)npanels * (npanels + 1) / 2;
  const double* p = ws + pair * (kPanel * kPanel) + (i % kPanel) * kPanel + (j % kPanel);
  double s = 0.0;
  for (int c = 0; c < nchunks; ++c) s += p[(int64_t)c * npairs * (kPanel * kPanel)];
  gram[idx] = s;
}

int gram_check(int in_dtype, int64_t K, int flags, int allowed) {
  if (in_dtype != FJAGG_F32) return fail(FJAGG_EUNSUPPORTED, "gram: float32 deltas only");
  if (flags & FJAGG_ACCUMULATE) return fail(FJAGG_EUNSUPPORTED, "gram: no FJAGG_ACCUMULATE");
  if (flags & FJAGG_NARROW) return fail(FJAGG_EUNSUPPORTED, "gram: no FJAGG_NARROW plans");
  if (flags & FJAGG_HOST_TABLES) return fail(FJAGG_EUNSUPPORTED, "gram: device plan only (no FJAGG_HOST_TABLES)");
  if (flags & FJAGG_ZEROED_WS) return fail(FJAGG_EUNSUPPORTED, "gram: no FJAGG_ZEROED_WS (the workspace needs no zeroing)");
  if (flags & FJAGG_UNBALANCED) return fail(FJAGG_EUNSUPPORTED, "gram: no FJAGG_UNBALANCED");
  if (flags & ~allowed) return fail(FJAGG_EUNSUPPORTED, "gram: unsupported flags 0x%x", flags & ~allowed);
  if (K < 1) return fail(FJAGG_EINVAL, "K must be >= 1 (got %lld)", (long long)K);
  if (K > kMaxClients) return fail(FJAGG_EUNSUPPORTED, "gram: K <= %d clients (got %lld)", kMaxClients, (long long)K);
  return FJAGG_OK;
}

int combine(const double* ws, int64_t K, int64_t nchunks, double* gram, hipStream_t s) {
  const unsigned grid = (unsigned)((K * K + 255) / 256);
  hipLaunchKernelGGL(k_gram_combine, dim3(grid), dim3(256), 0, s, ws, (int)K, (int)nchunks, (int)panels_of(K), gram);
  return check_launch("k_gram_combine");
}

}  // namespace

extern "C" {

int64_t fjagg_gram_chunk_columns(int64_t K, int64_t P) {
  g_err[0] = 0;
  if (K < 1 || K > kMaxClients || P < 1) return fail(FJAGG_EINVAL, "gram: need 1 <= K <= %d and P >= 1", kMaxClients);
  return dense_chunk_cols(K, P);
}

int64_t fjagg_gram_workspace_bytes(int64_t K, int64_t P_or_total, int64_t nblk) {
  g_err[0] = 0;
  if (K < 1 || K > kMaxClients || nblk < 0 || (nblk == 0 && P_or_total < 1))
    return fail(FJAGG_EINVAL, "gram: need 1 <= K <= %d, and P >= 1 or nblk >= 1", kMaxClients);
  int64_t nchunks;
  if (nblk > 0) {
    nchunks = ptrs_chunks(K, nblk);
  } else {
    const int64_t cc = dense_chunk_cols(K, P_or_total);
    nchunks = (P_or_total + cc - 1) / cc;
  }
  return nchunks * pairs_of(K) * kPanel * kPanel * (int64_t)sizeof(double);
}

int fjagg_gram_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, double* gram_dev, void* ws_dev,
                     int64_t ws_bytes, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = gram_check(in_dtype, K, flags, 0)) return rc;
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "gram: rows <= 1 GiB");
  if (!x_dev || !gram_dev || !ws_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  const int64_t need = fjagg_gram_workspace_bytes(K, P, 0);
  if (ws_bytes < need)
    return fail(FJAGG_EINVAL, "gram: needs %lld workspace bytes (got %lld)", (long long)need, (long long)ws_bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t cc = dense_chunk_cols(K, P), nchunks = (P + cc - 1) / cc;
  double* ws = reinterpret_cast<double*>(ws_dev);
  hipLaunchKernelGGL(k_gram_dense, dim3((unsigned)nchunks, (unsigned)pairs_of(K)), dim3(256), 0, s,
                     reinterpret_cast<const float*>(x_dev), ld, (int)K, P, cc, (int)panels_of(K), ws);
  if (int rc = check_launch("k_gram_dense")) return rc;
  return combine(ws, K, nchunks, gram_dev, s);
}

int fjagg_gram_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, double* gram_dev,
                    void* ws_dev, int64_t ws_bytes, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = gram_check(in_dtype, K, flags, FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev || !gram_dev || !ws_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  const int64_t need = fjagg_gram_workspace_bytes(K, 0, nblk);
  if (ws_bytes < need)
    return fail(FJAGG_EINVAL, "gram: needs %lld workspace bytes (got %lld)", (long long)need, (long long)ws_bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nchunks = ptrs_chunks(K, nblk);
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  double* ws = reinterpret_cast<double*>(ws_dev);
  hipLaunchKernelGGL(k_gram_ptrs, dim3((unsigned)nchunks, (unsigned)pairs_of(K)), dim3(256), 0, s, image_dev, L, (int)K,
                     V, nblk, (int)panels_of(K), ws);
  if (int rc = check_launch("k_gram_ptrs")) return rc;
  return combine(ws, K, nchunks, gram_dev, s);
}

}  // extern "C"
