// fjsparse.hip — top-k sparsified mean (include/fjcomp.h: fjcomp_topk_select_dense / _ptrs,
// fjcomp_topk_mean_dense / _ptrs). Every client keeps the coordinates of its whole delta whose
// magnitude key m(v) = bits(v) & 0x7fffffff is at least its own threshold T_k, the c-th largest
// key of its row; the rest count as +0 in tree_mean's fold:
//
//   x~_k[i] = m(x_k[i]) >= T_k ? x_k[i] : +0
//   s = fl(x~_0[i] w_0);  s = fl(s + fl(x~_k[i] w_k)), k = 1 .. K-1;  y[i] = fl(s scale)
//
// T_k is exact: a three-level radix select, most significant digit first (11 / 10 / 10 bits,
// fjsparse_dev.h). Per level
//
//   k_topk_hist   a workgroup takes kChunk elements of one client's row, counts the digit of
//                 every element whose higher digits match the client's prefix into an LDS
//                 histogram (integer LDS atomics) and adds its non-empty bins to hist[k][bins]
//                 (integer global atomics);
//   k_topk_scan   one workgroup per client walks the bins from the top until the running count
//                 reaches the remaining rank, writes the digit and the rank left inside it, and
//                 zeroes the row for the next level. The last level writes T_k and sent_k, the
//                 count of keys >= max(T_k, 1), from its own histogram and the ranks it was given.
//
// Integer counts make every histogram independent of the order its atomics arrive in. Every
// bin index is a masked digit (fjsparse::digit), so no data-dependent address can leave a
// histogram; hist rows are kMaxBins wide whatever the level. The histograms are zeroed on the
// stream inside the entry (and again by every scan), so a captured round replays correctly.
//
// k_topk_fold is the dense walk with T_k beside w_k: a lane owns four consecutive elements,
// walks the clients in order with eight rows' loads in flight, and applies the same multiply, add
// and scale as the exact fold. Built with contraction off: no multiply-add is fused.
//
// Both addressings share the kernels through a row functor: DenseRows (base, leading dimension)
// and PtrRows (in_ptrs[K*L], leaf_n[L], chunk_prefix[L+1]); a chunk never spans two leaves, and
// one histogram per client spans all its leaves. Float32 only.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjcomp.h"
#include "fjsparse_dev.h"

// The thread-local message behind fjagg_last_error() (defined in fjagg.hip), declared as
// fjcenter.hip declares it.
extern __attribute__((visibility("hidden"))) __thread char sparse_err[512] __asm__("fjagg_g_err");

static_assert(FJCOMP_TOPK_CHUNK == fjsparse::kChunk, "fjcomp.h and fjsparse_dev.h disagree on the chunk");
static_assert(FJCOMP_TOPK_MAX_CLIENTS == fjsparse::kMaxClients, "fjcomp.h and fjsparse_dev.h disagree on K");

namespace {

using namespace fjsparse;

int refuse(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(sparse_err, sizeof(sparse_err), fmt, ap);
  va_end(ap);
  return code;
}

int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(FJAGG_EHIP, "%s: %s", what, hipGetErrorString(e));
  return FJAGG_OK;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kTilesPerChunk = kChunk / kFoldTile;

// ------------------------------------------------------------------ row functors
// locate(chunk): the leaf the chunk lies in, that leaf's size and the chunk's first element in
// it; row(k, leaf): the leaf's base in client k's row; out(leaf): the leaf's base in the result.
struct DenseRows {
  const float* base;
  int64_t ld, P;
  float* y;
  __device__ __forceinline__ void locate(int64_t chunk, int64_t* leaf, int64_t* n, int64_t* i0) const {
    *leaf = 0;
    *n = P;
    *i0 = chunk * kChunk;
  }
  __device__ __forceinline__ const float* row(int64_t k, int64_t) const { return base + k * ld; }
  __device__ __forceinline__ float* out(int64_t) const { return y; }
};

struct PtrRows {
  const float* const* in_ptrs;  // [K * L], client-major
  float* const* out_ptrs;       // [L] (the fold only)
  const int64_t* leaf_n;        // [L]
  const int64_t* chunk_prefix;  // [L + 1], running sum of ceil(leaf_n / kChunk)
  int64_t L;
  __device__ __forceinline__ void locate(int64_t chunk, int64_t* leaf, int64_t* n, int64_t* i0) const {
    int64_t lo = 0, hi = L;  // chunk_prefix[lo] <= chunk < chunk_prefix[hi]; empty leaves are skipped
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (chunk_prefix[mid] <= chunk) lo = mid;
      else hi = mid;
    }
    *leaf = lo;
    *n = leaf_n[lo];
    *i0 = (chunk - chunk_prefix[lo]) * kChunk;
  }
  __device__ __forceinline__ const float* row(int64_t k, int64_t leaf) const { return in_ptrs[k * L + leaf]; }
  __device__ __forceinline__ float* out(int64_t leaf) const { return out_ptrs[leaf]; }
};

// Four consecutive elements' bits from p[i .. i+cnt), zeros past cnt. VEC: p + i is 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t i, int cnt, uint32_t (&v)[4]) {
  if (VEC && cnt == 4) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(p + i);
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? __float_as_uint(p[i + j]) : 0u;
  }
}

// ------------------------------------------------------------------ histogram pass
template <int LEVEL, class ROWS, bool VEC>
__global__ __launch_bounds__(kThreads) void k_topk_hist(ROWS rows, const uint32_t* __restrict__ prefix,
                                                        uint32_t* __restrict__ hist) {
  constexpr int NB = LEVEL == 0 ? 2048 : 1024;
  static_assert(NB <= kMaxBins, "a histogram row holds kMaxBins counters");
  __shared__ uint32_t sh[NB];
  const int64_t k = blockIdx.y;
  for (int e = threadIdx.x; e < NB; e += kThreads) sh[e] = 0;
  __syncthreads();
  int64_t leaf, n, i0;
  rows.locate(blockIdx.x, &leaf, &n, &i0);
  const float* __restrict__ p = rows.row(k, leaf);
  const uint32_t pre = LEVEL ? prefix[k] : 0u;
  const int64_t end = i0 + kChunk < n ? i0 + kChunk : n;
  auto count = [&](uint32_t b, bool valid) {
    const uint32_t m = key(b);
    // digit() is masked to [0, NB): the LDS address cannot leave sh whatever b holds
    if (valid && matches(m, pre, LEVEL)) atomicAdd(&sh[digit(m, LEVEL)], 1u);
  };
  constexpr int kStep = kThreads * 4, kAhead = 4;
  for (int64_t i = i0 + threadIdx.x * 4; i < end; i += (int64_t)kStep * kAhead) {
    uint32_t v[kAhead][4];
    int cnt[kAhead];
#pragma unroll
    for (int a = 0; a < kAhead; ++a) {
      const int64_t ia = i + (int64_t)a * kStep;
      const int64_t left = end - ia;
      cnt[a] = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
      if (cnt[a] > 0) load4<VEC>(p, ia, cnt[a], v[a]);
    }
#pragma unroll
    for (int a = 0; a < kAhead; ++a) {
#pragma unroll
      for (int j = 0; j < 4; ++j) count(v[a][j], j < cnt[a]);
    }
  }
  __syncthreads();
  uint32_t* __restrict__ row = hist + k * kMaxBins;
  for (int e = threadIdx.x; e < NB; e += kThreads) {
    const uint32_t c = sh[e];
    if (c) atomicAdd(&row[e], c);
  }
}

// ------------------------------------------------------------------ scan
// One workgroup per client. Lane t owns the PER bins below NB - 1 - t * PER; the slice sums are
// prefix-summed through LDS, then every lane runs fjsparse::scan_slice over its own bins.
template <int LEVEL>
__global__ __launch_bounds__(kThreads) void k_topk_scan(uint32_t c, uint32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ prefix, uint32_t* __restrict__ rank,
                                                        uint32_t* __restrict__ thr, int32_t* __restrict__ sent) {
  constexpr int NB = LEVEL == 0 ? 2048 : 1024, PER = NB / kThreads;
  __shared__ uint32_t sums[kThreads];
  __shared__ int found;
  const int64_t k = blockIdx.x;
  const int t = threadIdx.x;
  uint32_t* __restrict__ row = hist + k * kMaxBins;
  const uint32_t r = LEVEL ? rank[k] : c;
  const uint32_t pre = LEVEL ? prefix[k] : 0u;
  const int lo = NB - (t + 1) * PER;  // this lane's bins: lo .. lo + PER - 1
  uint32_t h[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    h[j] = row[lo + j];
    row[lo + j] = 0;  // the next level, and the next call, find the row zeroed
    sum += h[j];
  }
  if (t == 0) found = 0;
  sums[t] = sum;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {  // inclusive prefix sum over the lanes (bins from the top)
    const uint32_t add = t >= d ? sums[t - d] : 0u;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  Pick p = {0, 0u, 0u, 0u};
  scan_slice(h, PER - 1, PER, sums[t] - sum, r, &p);
  if (p.found) found = 1;
  __syncthreads();
  if (!found && t == 0) {  // unreachable for 1 <= c <= P (the counts are exact): keep the state defined
    p.found = 1;
    p.digit = 0;
    p.rank = 1;
    p.ge = r;
  } else if (p.found) {
    p.digit += (uint32_t)lo;
  }
  if (p.found) {
    if (LEVEL < 2) {
      prefix[k] = (LEVEL ? (pre << 10) : 0u) | p.digit;
      rank[k] = p.rank;
    } else {
      const uint32_t T = threshold(pre, p);
      thr[k] = T;
      sent[k] = (int32_t)sent_count(c, r, T, p, p.ge - (r - p.rank));
    }
  }
}

// ------------------------------------------------------------------ masked fold
template <class ROWS, bool VEC>
__global__ __launch_bounds__(kThreads) void k_topk_fold(ROWS rows, int64_t K, const float* __restrict__ w,
                                                        const uint32_t* __restrict__ thr, float scale) {
  const int64_t tile = blockIdx.x;
  int64_t leaf, n, i0;
  rows.locate(tile / kTilesPerChunk, &leaf, &n, &i0);
  const int64_t i = i0 + (tile % kTilesPerChunk) * kFoldTile + threadIdx.x * 4;
  if (i >= n) return;
  const int cnt = n - i >= 4 ? 4 : (int)(n - i);
  auto term = [](uint32_t b, uint32_t T, float wk) {
    const float x = key(b) >= T ? __uint_as_float(b) : 0.0f;  // a kept -0 passes verbatim
    return __fmul_rn(x, wk);
  };
  float acc[4];
  {  // client 0: s = t_0, as the exact fold starts
    uint32_t v[4];
    load4<VEC>(rows.row(0, leaf), i, cnt, v);
    const uint32_t T = thr[0];
    const float w0 = w[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = term(v[j], T, w0);
  }
  constexpr int U = 8;
  int64_t k = 1;
  for (; k + U <= K; k += U) {
    uint32_t v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) load4<VEC>(rows.row(k + u, leaf), i, cnt, v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t T = thr[k + u];
      const float wk = w[k + u];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], term(v[u][j], T, wk));
    }
  }
  for (; k < K; ++k) {
    uint32_t v[4];
    load4<VEC>(rows.row(k, leaf), i, cnt, v);
    const uint32_t T = thr[k];
    const float wk = w[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], term(v[j], T, wk));
  }
  float* __restrict__ y = rows.out(leaf);
  if (VEC && cnt == 4) {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __float_as_uint(__fmul_rn(acc[j], scale));
    *reinterpret_cast<u32x4*>(y + i) = o;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) y[i + j] = __fmul_rn(acc[j], scale);
  }
}

// ------------------------------------------------------------------ launchers
struct Ws {
  uint32_t *hist, *prefix, *rank;
};

Ws carve(void* ws, int64_t K) {
  uint32_t* h = static_cast<uint32_t*>(ws);
  return Ws{h, h + K * kMaxBins, h + K * kMaxBins + K};
}

template <int LEVEL, class ROWS>
void launch_level(const ROWS& rows, bool vec, int64_t K, int64_t nchunks, uint32_t c, const Ws& ws, float* thr,
                  int32_t* sent, hipStream_t s) {
  const dim3 grid((unsigned)nchunks, (unsigned)K);
  if (vec) hipLaunchKernelGGL((k_topk_hist<LEVEL, ROWS, true>), grid, dim3(kThreads), 0, s, rows, ws.prefix, ws.hist);
  else hipLaunchKernelGGL((k_topk_hist<LEVEL, ROWS, false>), grid, dim3(kThreads), 0, s, rows, ws.prefix, ws.hist);
  hipLaunchKernelGGL((k_topk_scan<LEVEL>), dim3((unsigned)K), dim3(kThreads), 0, s, c, ws.hist, ws.prefix, ws.rank,
                     reinterpret_cast<uint32_t*>(thr), sent);
}

template <class ROWS>
int run_select(const ROWS& rows, bool vec, int64_t K, int64_t nchunks, int64_t c, float* thr, int32_t* sent,
               void* ws_dev, hipStream_t s) {
  const Ws ws = carve(ws_dev, K);
  if (hipMemsetAsync(ws.hist, 0, (size_t)K * kMaxBins * sizeof(uint32_t), s) != hipSuccess)
    return launched("topk: zeroing the histograms");
  launch_level<0>(rows, vec, K, nchunks, (uint32_t)c, ws, thr, sent, s);
  launch_level<1>(rows, vec, K, nchunks, (uint32_t)c, ws, thr, sent, s);
  launch_level<2>(rows, vec, K, nchunks, (uint32_t)c, ws, thr, sent, s);
  return launched("k_topk_hist / k_topk_scan");
}

template <class ROWS>
int run_fold(const ROWS& rows, bool vec, int64_t K, int64_t nchunks, const float* w, const float* thr, float scale,
             hipStream_t s) {
  const dim3 grid((unsigned)(nchunks * kTilesPerChunk));
  const uint32_t* t = reinterpret_cast<const uint32_t*>(thr);
  if (vec) hipLaunchKernelGGL((k_topk_fold<ROWS, true>), grid, dim3(kThreads), 0, s, rows, K, w, t, scale);
  else hipLaunchKernelGGL((k_topk_fold<ROWS, false>), grid, dim3(kThreads), 0, s, rows, K, w, t, scale);
  return launched("k_topk_fold");
}

// What every entry checks before any launch. P == 0 is the caller's to skip (nothing to launch).
int check_common(const char* what, int in_dtype, int64_t K, int64_t P, int64_t c, const void* thr, const void* sent,
                 const void* ws, int64_t ws_bytes) {
  if (in_dtype != FJAGG_F32) return refuse(FJAGG_EUNSUPPORTED, "%s: float32 deltas only", what);
  if (K < 1) return refuse(FJAGG_EINVAL, "%s: K must be >= 1 (got %lld)", what, (long long)K);
  if (K > kMaxClients)
    return refuse(FJAGG_EUNSUPPORTED, "%s: K <= %d clients (got %lld)", what, kMaxClients, (long long)K);
  if (P < 0) return refuse(FJAGG_EINVAL, "%s: P must be >= 0 (got %lld)", what, (long long)P);
  if (P >= (1ll << 31)) return refuse(FJAGG_EUNSUPPORTED, "%s: P < 2^31 elements per client (got %lld)", what, (long long)P);
  if (P == 0) return FJAGG_OK;
  if (c < 1 || c > P)
    return refuse(FJAGG_EINVAL, "%s: the keep count must be in [1, P = %lld] (got %lld)", what, (long long)P, (long long)c);
  if (!thr || !sent || !ws) return refuse(FJAGG_EINVAL, "%s: null pointer argument", what);
  if (ws_bytes < fjcomp_topk_workspace_bytes(K))
    return refuse(FJAGG_EINVAL, "%s: workspace too small (need %lld bytes)", what, (long long)fjcomp_topk_workspace_bytes(K));
  return FJAGG_OK;
}

int check_dense(const char* what, const void* x, int64_t ld, int64_t K, int64_t P) {
  if (!x) return refuse(FJAGG_EINVAL, "%s: null pointer argument", what);
  if (K > 1 && ld < P) return refuse(FJAGG_EINVAL, "%s: ld = %lld < P = %lld", what, (long long)ld, (long long)P);
  return FJAGG_OK;
}

int check_ptrs(const char* what, const void* in_ptrs, int64_t L, const void* leaf_n, const void* chunk_prefix,
               int64_t nchunks, int64_t P, int flags) {
  if (flags & ~FJAGG_UNALIGNED) return refuse(FJAGG_EUNSUPPORTED, "%s: unsupported flags 0x%x", what, flags & ~FJAGG_UNALIGNED);
  if (L < 1) return refuse(FJAGG_EINVAL, "%s: L must be >= 1 (got %lld)", what, (long long)L);
  if (!in_ptrs || !leaf_n || !chunk_prefix) return refuse(FJAGG_EINVAL, "%s: null table", what);
  // the chunks of L leaves holding P elements: at least ceil(P / chunk), at most one partial chunk per leaf more
  const int64_t least = (P + kChunk - 1) / kChunk;
  if (nchunks < least || nchunks > P / kChunk + L)
    return refuse(FJAGG_EINVAL, "%s: nchunks = %lld is not the chunk count of %lld elements in %lld leaves", what,
                  (long long)nchunks, (long long)P, (long long)L);
  return FJAGG_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int64_t fjcomp_topk_workspace_bytes(int64_t K) {
  if (K < 1) return 0;
  return K * (int64_t)(kMaxBins + 2) * (int64_t)sizeof(uint32_t);
}

int fjcomp_topk_select_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t c,
                             float* thresholds_dev, int32_t* sent_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  const char* what = "topk_select_dense";
  if (int rc = check_common(what, in_dtype, K, P, c, thresholds_dev, sent_dev, ws_dev, ws_bytes)) return rc;
  if (P == 0) return FJAGG_OK;
  if (int rc = check_dense(what, x_dev, ld, K, P)) return rc;
  const DenseRows rows{static_cast<const float*>(x_dev), K > 1 ? ld : P, P, nullptr};
  const bool vec = aligned16(x_dev) && (K == 1 || ld % 4 == 0);
  return run_select(rows, vec, K, (P + kChunk - 1) / kChunk, c, thresholds_dev, sent_dev, ws_dev,
                    reinterpret_cast<hipStream_t>(stream));
}

int fjcomp_topk_select_ptrs(int in_dtype, const float* const* in_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                            const int64_t* chunk_prefix, int64_t nchunks, int64_t P, int64_t c, float* thresholds_dev,
                            int32_t* sent_dev, void* ws_dev, int64_t ws_bytes, int flags, void* stream) {
  const char* what = "topk_select_ptrs";
  if (int rc = check_common(what, in_dtype, K, P, c, thresholds_dev, sent_dev, ws_dev, ws_bytes)) return rc;
  if (P == 0) return FJAGG_OK;
  if (int rc = check_ptrs(what, in_ptrs, L, leaf_n, chunk_prefix, nchunks, P, flags)) return rc;
  const PtrRows rows{in_ptrs, nullptr, leaf_n, chunk_prefix, L};
  return run_select(rows, !(flags & FJAGG_UNALIGNED), K, nchunks, c, thresholds_dev, sent_dev, ws_dev,
                    reinterpret_cast<hipStream_t>(stream));
}

int fjcomp_topk_mean_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t c,
                           const float* w_dev, float scale, float* out_dev, float* thresholds_dev, int32_t* sent_dev,
                           void* ws_dev, int64_t ws_bytes, void* stream) {
  const char* what = "topk_mean_dense";
  if (int rc = check_common(what, in_dtype, K, P, c, thresholds_dev, sent_dev, ws_dev, ws_bytes)) return rc;
  if (P == 0) return FJAGG_OK;
  if (int rc = check_dense(what, x_dev, ld, K, P)) return rc;
  if (!w_dev || !out_dev) return refuse(FJAGG_EINVAL, "%s: null pointer argument", what);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const DenseRows rows{static_cast<const float*>(x_dev), K > 1 ? ld : P, P, out_dev};
  const bool vec = aligned16(x_dev) && (K == 1 || ld % 4 == 0);
  const int64_t nchunks = (P + kChunk - 1) / kChunk;
  if (int rc = run_select(rows, vec, K, nchunks, c, thresholds_dev, sent_dev, ws_dev, s)) return rc;
  return run_fold(rows, vec && aligned16(out_dev), K, nchunks, w_dev, thresholds_dev, scale, s);
}

int fjcomp_topk_mean_ptrs(int in_dtype, const float* const* in_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                          const int64_t* chunk_prefix, int64_t nchunks, int64_t P, int64_t c, const float* w_dev,
                          float scale, float* const* out_ptrs, float* thresholds_dev, int32_t* sent_dev, void* ws_dev,
                          int64_t ws_bytes, int flags, void* stream) {
  const char* what = "topk_mean_ptrs";
  if (int rc = check_common(what, in_dtype, K, P, c, thresholds_dev, sent_dev, ws_dev, ws_bytes)) return rc;
  if (P == 0) return FJAGG_OK;
  if (int rc = check_ptrs(what, in_ptrs, L, leaf_n, chunk_prefix, nchunks, P, flags)) return rc;
  if (!w_dev || !out_ptrs) return refuse(FJAGG_EINVAL, "%s: null pointer argument", what);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const PtrRows rows{in_ptrs, out_ptrs, leaf_n, chunk_prefix, L};
  const bool vec = !(flags & FJAGG_UNALIGNED);
  if (int rc = run_select(rows, vec, K, nchunks, c, thresholds_dev, sent_dev, ws_dev, s)) return rc;
  return run_fold(rows, vec, K, nchunks, w_dev, thresholds_dev, scale, s);
}

}  // extern "C"
