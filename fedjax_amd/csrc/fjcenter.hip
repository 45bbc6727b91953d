// fjcenter.hip — centered clipping (Karimireddy, He and Jaggi, ICML 2021): the robust mean
// clipped around the previous round's aggregate (include/fjagg.h: fjagg_l2sq_rows_centered,
// fjagg_center_fold_dense / _ptrs, fjagg_center_clip_dense / _ptrs). One iteration from centre v:
//
//   d_k[p] = fl(x_k[p] - v[p]);  q_k = sum_p fl(d_k[p]^2)        (the norm pass, k_l2sq_rows' order)
//   n_k, c_k = fjagg_clip_scales(q, tau)
//   t_k[p] = c_k > 0 ? fl(c_k d_k[p]) : +0;  s = +0;  s = fl(s + t_k[p]), k = 0 .. K-1
//   v'[p]  = fl(v[p] + fl(s f32(1/K)))
//
// Both passes stream the deltas once; the centre (P floats) is re-read per client by the norm
// pass and once per lane by the fold, which keeps its centre unit in registers over the whole
// client loop and writes v' for its own columns only: out may be the centre itself. The factors
// are formed on the device, so a whole round of L iterations issues 4L launches and never visits
// the host. Float32 only; no FMA (the library is built with contraction off).
#include "fjagg_dev.h"

// The thread-local message behind fjagg_last_error() (defined in fjagg.hip), under a name of this
// file's and declared __thread as fjrobust.hip declares it: the buffer has a constant initialiser,
// and through fjagg_dev.h's hidden thread_local declaration every access would first call the
// buffer's (absent) dynamic-initialisation function through a hidden weak reference, which a
// shared library resolves to its load address, not to null. This file therefore uses neither that
// declaration nor the header's fail() and check_launch().
extern __attribute__((visibility("hidden"))) __thread char center_err[512] __asm__("fjagg_g_err");

namespace {

int refuse(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(center_err, sizeof(center_err), fmt, ap);
  va_end(ap);
  return code;
}

int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(FJAGG_EHIP, "%s: %s", what, hipGetErrorString(e));
  return FJAGG_OK;
}

constexpr int kCenterMaxClients = 4096;
constexpr int64_t kCenterMaxRowBytes = 1ll << 30;
constexpr int64_t kNormPer = 64 * 1024;  // elements per norm block: fjagg_l2sq_rows' partition
constexpr int kMaxGridY = 65535;

// ------------------------------------------------------------------ norm pass
// Block blockIdx.x of one row: the squares of fl(x[e] - v[e]) over elements [b*per, (b+1)*per) of
// the row's n, in k_l2sq_rows' order exactly (eight loads of each operand in flight per lane, the
// lane sums ascending, the fixed shuffle tree, the four wave sums in order), so a zero centre gives
// fjagg_l2sq_rows' bits: x - (+0) is x. NT: the deltas are loaded non-temporal, so a stream larger
// than the cache does not evict the centre, which every row of a leaf re-reads (with temporal loads
// the pass measured 10 % over k_l2sq_rows on the 1024 x 4 Mi slab, with them it is level: DESIGN 3p).
template <bool NT>
__device__ __forceinline__ void l2sq_centered_block(const uint8_t* __restrict__ x, const uint8_t* __restrict__ v,
                                                    int64_t n, int64_t per, float* __restrict__ slot) {
  const int64_t e0 = (int64_t)blockIdx.x * per;
  const int64_t e1 = (e0 + per < n) ? e0 + per : n;
  float s = 0.f;
  int64_t e = e0 + threadIdx.x;
  constexpr int kAhead = 8;
  for (; e + (kAhead - 1) * (int64_t)kThreads < e1; e += kAhead * (int64_t)kThreads) {
    float a[kAhead], c[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j)
      a[j] = __uint_as_float(load_unit_ptr<FJAGG_F32, 1, NT>(x + (e + j * (int64_t)kThreads) * 4));
#pragma unroll
    for (int j = 0; j < kAhead; ++j)
      c[j] = __uint_as_float(load_unit_ptr<FJAGG_F32, 1, false>(v + (e + j * (int64_t)kThreads) * 4));
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const float d = __fsub_rn(a[j], c[j]);
      s = __fadd_rn(s, __fmul_rn(d, d));
    }
  }
  for (; e < e1; e += kThreads) {
    const float d = __fsub_rn(__uint_as_float(load_unit_ptr<FJAGG_F32, 1, NT>(x + e * 4)),
                              __uint_as_float(load_unit_ptr<FJAGG_F32, 1, false>(v + e * 4)));
    s = __fadd_rn(s, __fmul_rn(d, d));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
  __shared__ float red[kThreads / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int i = 1; i < kThreads / 64; ++i) t = __fadd_rn(t, red[i]);
    *slot = t;
  }
}

// Rows from tables: row r = r0 + blockIdx.y is at ptrs[r], has ns[r % mod] elements and its centre
// at cen[r % mod]. mod = R: one entry per row (fjagg_l2sq_rows_centered's image); mod = L: the
// rows are a [K, L] leaf table and the sizes and centres are per leaf (the plan image of a fold).
template <bool NT>
__global__ __launch_bounds__(kThreads) void k_l2sq_rows_centered(const int64_t* __restrict__ ptrs,
                                                                 const int64_t* __restrict__ ns,
                                                                 const int64_t* __restrict__ cen, int64_t mod,
                                                                 int64_t r0, int64_t per, float* __restrict__ ws) {
  const int64_t r = r0 + blockIdx.y, l = r % mod;
  l2sq_centered_block<NT>(reinterpret_cast<const uint8_t*>(ptrs[r]), reinterpret_cast<const uint8_t*>(cen[l]), ns[l],
                      per, ws + r * gridDim.x + blockIdx.x);
}

// Rows of a dense slab: row r = k*L + l is leaf l of client k, elements [off[l], off[l] + n[l]) of
// slab row k and of the centre (tab = off[L] | n[L]; no table: one leaf, the whole row).
template <bool NT>
__global__ __launch_bounds__(kThreads) void k_l2sq_slab_centered(const uint8_t* __restrict__ x, int64_t ld_bytes,
                                                                 int64_t P, const int64_t* __restrict__ tab,
                                                                 int64_t L, const uint8_t* __restrict__ cen,
                                                                 int64_t r0, int64_t per, float* __restrict__ ws) {
  const int64_t r = r0 + blockIdx.y, k = r / L, l = r - k * L;
  const int64_t off = tab ? tab[l] : 0, n = tab ? tab[L + l] : P;
  l2sq_centered_block<NT>(x + k * ld_bytes + off * 4, cen + off * 4, n, per, ws + r * gridDim.x + blockIdx.x);
}

// out[g] = the nb partials of rows [g*rows_per_group, (g+1)*rows_per_group), added in order from
// +0 (fjagg_l2sq_rows' combine); its correctly rounded root when take_sqrt (via f64).
__global__ void k_center_groups(const float* __restrict__ ws, int64_t nb, int64_t G, int64_t rows_per_group,
                                int take_sqrt, float* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  float s = 0.f;
  for (int64_t i = 0; i < rows_per_group * nb; ++i) s = __fadd_rn(s, ws[g * rows_per_group * nb + i]);
  out[g] = take_sqrt ? (float)__dsqrt_rn((double)s) : s;
}

// ------------------------------------------------------------------ fold pass
// Each lane folds E units of V elements: unit j sits at byte offset off[j] of every client row, of
// the centre and of the output (a lane past its range holds a clamped, in-bounds offset and stores
// nothing). The centre unit is loaded once and stays in registers; U clients' row loads
// (buffer-resource, 32-bit lane offsets) are issued before the first is consumed, and the next
// group's row bases are fetched under them as in the shared fold. c[k] is uniform over the wave: a
// scalar load, and the test c_k > 0 a scalar one. A client with c_k NaN, 0 or negative adds +0:
// the select is on the value, so its loaded bits (NaN, inf) never reach the sum.
template <int V, int E, int U, bool NT, class RowFn>
__device__ __forceinline__ void center_fold(RowFn row, uint32_t row_bytes, int K, const uint32_t (&off)[E],
                                            const bool (&valid)[E], const float* __restrict__ c,
                                            const uint8_t* cen, uint8_t* out, float inv_k) {
  using Raw = typename Unit<FJAGG_F32, V>::Raw;
  float cv[E][V], acc[E][V];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    decode<FJAGG_F32, AccF, V>(load_unit_ptr<FJAGG_F32, V, false>(cen + off[j]), cv[j]);
#pragma unroll
    for (int i = 0; i < V; ++i) acc[j][i] = 0.f;
  }
  auto add_client = [&](const Raw(&v)[E], float ck) {
    const bool use = ck > 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      float t[V];
      decode<FJAGG_F32, AccF, V>(v[j], t);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float d = __fsub_rn(t[i], cv[j][i]);
        acc[j][i] = __fadd_rn(acc[j][i], use ? __fmul_rn(ck, d) : 0.f);
      }
    }
  };
  int k = 0;
  const uint8_t* nxt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) nxt[u] = row(u < K ? u : K - 1);
  for (; k + U <= K; k += U) {
    Raw v[U][E];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const auto r = row_rsrc(nxt[u], row_bytes);
#pragma unroll
      for (int j = 0; j < E; ++j) v[u][j] = load_unit<FJAGG_F32, V, NT>(r, off[j]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kn = k + U + u;
      nxt[u] = row(kn < K ? kn : K - 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) add_client(v[u], c[k + u]);
  }
  for (; k < K; ++k) {
    const auto r = row_rsrc(row(k), row_bytes);
    Raw v[E];
#pragma unroll
    for (int j = 0; j < E; ++j) v[j] = load_unit<FJAGG_F32, V, NT>(r, off[j]);
    add_client(v, c[k]);
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    if (!valid[j]) continue;
    unsigned b[V];
#pragma unroll
    for (int i = 0; i < V; ++i) b[i] = __float_as_uint(__fadd_rn(cv[j][i], __fmul_rn(acc[j][i], inv_k)));
    store_unit<FJAGG_F32, V>(out + off[j], b);
  }
}

// Units [u0, u1) of V elements of every row, of the centre and of the output, kThreads*E at a time.
template <int V, int E, int U, bool NT, class RowFn>
__device__ __forceinline__ void center_walk(RowFn row, uint32_t row_bytes, int K, int64_t u0, int64_t u1,
                                            const float* __restrict__ c, const uint8_t* cen, uint8_t* out,
                                            float inv_k) {
  for (int64_t g = u0; g < u1; g += (int64_t)kThreads * E) {
    uint32_t off[E];
    bool valid[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
      int64_t u = g + j * kThreads + threadIdx.x;
      valid[j] = u < u1;
      if (!valid[j]) u = u1 - 1;  // keep the loads in bounds; the store is skipped
      off[j] = (uint32_t)(u * (V * 4));
    }
    center_fold<V, E, U, NT>(row, row_bytes, K, off, valid, c, cen, out, inv_k);
  }
}

// The fold's shape, the dense default of the shared fold: eight units per lane, four clients in
// flight (32 loads per lane: 32 x 16 B with 16-byte units, 224 VGPRs, two waves a SIMD). Four units
// per lane measured 10 % slower on the 1024 x 4 Mi slab. Eight clients in flight would
// spill SGPRs on the pytree path (eight row descriptors and eight prefetched bases).
template <int V> struct CenterShape {
  static constexpr int E = 8, U = 4;
};

// Dense slab: client k's row at x + k*ld_bytes, P = nunits*V + tail_n elements. Workgroup b folds
// units [b*kThreads*E, (b+1)*kThreads*E); one more workgroup folds the tail_n < V tail elements.
template <int V, bool NT>
__global__ __launch_bounds__(kThreads) void k_center_dense(const uint8_t* __restrict__ x, int64_t ld_bytes, int K,
                                                           int64_t nunits, int tail_n, const float* __restrict__ c,
                                                           const uint8_t* cen, uint8_t* out, float inv_k) {
  constexpr int E = CenterShape<V>::E, U = CenterShape<V>::U;
  auto row = [=](int k) { return x + k * ld_bytes; };
  const uint32_t row_bytes = (uint32_t)((nunits * V + tail_n) * 4);
  const int64_t per = (int64_t)kThreads * E, nfull = (nunits + per - 1) / per, b = blockIdx.x;
  if (b >= nfull) {
    const int64_t e0 = nunits * V;
    center_walk<1, 1, CenterShape<1>::U, NT>(row, row_bytes, K, e0, e0 + tail_n, c, cen, out, inv_k);
    return;
  }
  const int64_t u0 = b * per;
  center_walk<V, E, U, NT>(row, row_bytes, K, u0, u0 + per < nunits ? u0 + per : nunits, c, cen, out, inv_k);
}

// Pytree path over the plan image of fjagg_ptrs_plan_leaves (in_ptrs[K*L] | out_ptrs[L] | leaf_n[L]
// | blocks[2*nblk]) and L centre pointers at cptrs. Plan entry blockIdx.x names a range of one
// leaf: V-element units (V = 4, or 1 for a plan made with FJAGG_UNALIGNED), single elements with
// the element flag, or the leaf's tail past its last whole unit.
template <bool NT>
__global__ __launch_bounds__(kThreads) void k_center_ptrs(const int64_t* __restrict__ img, int L, int K, int V,
                                                          const int64_t* __restrict__ cptrs,
                                                          const float* __restrict__ c, float inv_k) {
  const int64_t* in_ptrs = img;
  const int64_t* out_ptrs = img + (int64_t)K * L;
  const int64_t* leaf_n = out_ptrs + L;
  const int64_t* blk = leaf_n + L + 2 * (int64_t)blockIdx.x;
  const int64_t be = blk[0];
  const int leaf = (int)((be >> 40) & 0x3fffff);
  const bool tail = (be >> 62) & 1;
  const bool elem = ((uint64_t)be >> 63) != 0;
  const int64_t u0 = be & ((1ll << 40) - 1), u1 = blk[1];
  const int64_t n = leaf_n[leaf];
  const uint8_t* cen = reinterpret_cast<const uint8_t*>(cptrs[leaf]);
  uint8_t* out = reinterpret_cast<uint8_t*>(out_ptrs[leaf]);
  const int64_t* lp = in_ptrs + leaf;
  auto row = [=](int k) { return reinterpret_cast<const uint8_t*>(lp[(int64_t)k * L]); };
  const uint32_t row_bytes = row_range(n * 4);
  if (!tail && !elem && V == 4) {
    const int64_t nu = n / 4;
    center_walk<4, CenterShape<4>::E, CenterShape<4>::U, NT>(row, row_bytes, K, u0, u1 < nu ? u1 : nu, c, cen, out,
                                                             inv_k);
    return;
  }
  const int64_t e0 = tail ? n / V * V : (elem ? u0 : u0 * V);
  int64_t e1 = tail ? n : (elem ? u1 : u1 * V);
  if (e1 > n) e1 = n;
  center_walk<1, CenterShape<1>::E, CenterShape<1>::U, NT>(row, row_bytes, K, e0, e1, c, cen, out, inv_k);
}

// ------------------------------------------------------------------ host side
int center_check(int in_dtype, int64_t K, int flags, int allowed) {
  if (in_dtype != FJAGG_F32) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: float32 deltas, centre and output only");
  if (flags & ~allowed)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: unsupported flags 0x%x", flags & ~allowed);
  if (K < 1 || K > kCenterMaxClients)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: 1 <= K <= %d clients (got %lld)", kCenterMaxClients,
                (long long)K);
  return FJAGG_OK;
}

int dense_check(const void* x, int64_t ld, int64_t K, int64_t P, const void* center, const void* out) {
  if (P < 1 || ld < P)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P,
                (long long)ld);
  if (P * 4 > kCenterMaxRowBytes) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: rows <= 1 GiB");
  if (!x || !center || !out) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: null pointer argument");
  const uintptr_t a = reinterpret_cast<uintptr_t>(center), b = reinterpret_cast<uintptr_t>(out);
  if (a != b && a < b + (uintptr_t)P * 4 && b < a + (uintptr_t)P * 4)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: out may be the centre itself, not overlap it in part");
  // the fold's workgroups read every row while others store their columns of out: an out inside
  // the slab's extent [x, x + ((K-1)*ld + P)*4) would be read half written (the centre is only
  // read, so it may be a row of the slab)
  const unsigned __int128 x0 = reinterpret_cast<uintptr_t>(x),
                          x1 = x0 + ((unsigned __int128)(K - 1) * (uint64_t)ld + (uint64_t)P) * 4;
  if (b < x1 && x0 < (unsigned __int128)b + (uint64_t)P * 4)
    return refuse(FJAGG_EUNSUPPORTED,
                  "centered clipping: out overlaps the deltas (the slab's rows are read while out is written)");
  return FJAGG_OK;
}

int plan_check(const void* image, int L, int64_t nblk) {
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: null pointer argument");
  return FJAGG_OK;
}

int round_check(float tau, int64_t iterations, const void* distances, const void* factors) {
  if (!(tau > 0.f) || tau > 3.402823466e38f)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: tau must be finite and > 0");
  if (iterations < 1)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: iterations >= 1 (got %lld)", (long long)iterations);
  if (!distances || !factors) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: null pointer argument");
  return FJAGG_OK;
}

inline int64_t norm_blocks(int64_t max_n) { return max_n > 0 ? (max_n + kNormPer - 1) / kNormPer : 1; }
inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }
inline float inverse_count(int64_t K) { return (float)(1.0 / (double)K); }

// the table form of the norm pass over rows [0, R), at most kMaxGridY rows a launch
int launch_norm_rows(const int64_t* ptrs, const int64_t* ns, const int64_t* cen, int64_t mod, int64_t R, int64_t nb,
                     float* ws, bool nt, hipStream_t s) {
  for (int64_t r0 = 0; r0 < R; r0 += kMaxGridY) {
    const int64_t nr = R - r0 < kMaxGridY ? R - r0 : kMaxGridY;
    const dim3 grid((unsigned)nb, (unsigned)nr);
    if (nt)
      hipLaunchKernelGGL(k_l2sq_rows_centered<true>, grid, dim3(kThreads), 0, s, ptrs, ns, cen, mod, r0, kNormPer, ws);
    else
      hipLaunchKernelGGL(k_l2sq_rows_centered<false>, grid, dim3(kThreads), 0, s, ptrs, ns, cen, mod, r0, kNormPer, ws);
    if (int rc = launched("k_l2sq_rows_centered")) return rc;
  }
  return FJAGG_OK;
}

int launch_norm_slab(const uint8_t* x, int64_t ldb, int64_t P, const int64_t* tab, int64_t L, const uint8_t* cen,
                     int64_t R, int64_t nb, float* ws, bool nt, hipStream_t s) {
  for (int64_t r0 = 0; r0 < R; r0 += kMaxGridY) {
    const int64_t nr = R - r0 < kMaxGridY ? R - r0 : kMaxGridY;
    const dim3 grid((unsigned)nb, (unsigned)nr);
    if (nt)
      hipLaunchKernelGGL(k_l2sq_slab_centered<true>, grid, dim3(kThreads), 0, s, x, ldb, P, tab, L, cen, r0, kNormPer,
                         ws);
    else
      hipLaunchKernelGGL(k_l2sq_slab_centered<false>, grid, dim3(kThreads), 0, s, x, ldb, P, tab, L, cen, r0, kNormPer,
                         ws);
    if (int rc = launched("k_l2sq_slab_centered")) return rc;
  }
  return FJAGG_OK;
}

int launch_groups(const float* ws, int64_t nb, int64_t G, int64_t rows_per_group, int take_sqrt, float* out,
                  hipStream_t s) {
  hipLaunchKernelGGL(k_center_groups, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, ws, nb, G, rows_per_group,
                     take_sqrt, out);
  return launched("k_center_groups");
}

// 16-byte units where every row, the centre and the output allow it, element units otherwise
int launch_fold_dense(const uint8_t* x, int64_t ld, int K, int64_t P, const float* c, const uint8_t* cen, uint8_t* out,
                      bool nt, hipStream_t s) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cen) |
                         reinterpret_cast<uintptr_t>(out) | (uintptr_t)(K > 1 ? ld * 4 : 0);
  const float inv_k = inverse_count(K);
  if ((bits & 15) == 0) {
    const int64_t nunits = P / 4, per = (int64_t)kThreads * CenterShape<4>::E;
    const int tail_n = (int)(P % 4);
    const dim3 grid((unsigned)((nunits + per - 1) / per + (tail_n ? 1 : 0)));
    if (nt)
      hipLaunchKernelGGL((k_center_dense<4, true>), grid, dim3(kThreads), 0, s, x, ld * 4, K, nunits, tail_n, c, cen,
                         out, inv_k);
    else
      hipLaunchKernelGGL((k_center_dense<4, false>), grid, dim3(kThreads), 0, s, x, ld * 4, K, nunits, tail_n, c, cen,
                         out, inv_k);
  } else {
    const int64_t per = (int64_t)kThreads * CenterShape<1>::E;
    const dim3 grid((unsigned)((P + per - 1) / per));
    if (nt)
      hipLaunchKernelGGL((k_center_dense<1, true>), grid, dim3(kThreads), 0, s, x, ld * 4, K, P, 0, c, cen, out, inv_k);
    else
      hipLaunchKernelGGL((k_center_dense<1, false>), grid, dim3(kThreads), 0, s, x, ld * 4, K, P, 0, c, cen, out,
                         inv_k);
  }
  return launched("k_center_dense");
}

int launch_fold_ptrs(const int64_t* img, int L, int K, int64_t nblk, int V, const int64_t* cptrs, const float* c,
                     bool nt, hipStream_t s) {
  const float inv_k = inverse_count(K);
  if (nt)
    hipLaunchKernelGGL((k_center_ptrs<true>), dim3((unsigned)nblk), dim3(kThreads), 0, s, img, L, K, V, cptrs, c,
                       inv_k);
  else
    hipLaunchKernelGGL((k_center_ptrs<false>), dim3((unsigned)nblk), dim3(kThreads), 0, s, img, L, K, V, cptrs, c,
                       inv_k);
  return launched("k_center_ptrs");
}

}  // namespace

extern "C" {

int fjagg_l2sq_rows_centered(int in_dtype, const int64_t* image_dev, int64_t R, int64_t max_n, int64_t rows_per_group,
                             int take_sqrt, float* out_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  center_err[0] = 0;
  if (in_dtype != FJAGG_F32) return refuse(FJAGG_EUNSUPPORTED, "centered norms: float32 rows and centres only");
  if (R < 1 || max_n < 0 || rows_per_group < 1 || R % rows_per_group)
    return refuse(FJAGG_EUNSUPPORTED, "centered norms: bad row grouping (R=%lld, rows_per_group=%lld)", (long long)R,
                (long long)rows_per_group);
  if (max_n * 4 > kCenterMaxRowBytes) return refuse(FJAGG_EUNSUPPORTED, "centered norms: rows <= 1 GiB");
  const int64_t nb = norm_blocks(max_n), need = R * nb * 4;
  if (!ws_dev || ws_bytes < need || !image_dev || !out_dev)
    return refuse(FJAGG_EUNSUPPORTED, "centered norms: need %lld workspace bytes and no null pointer", (long long)need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(ws_dev);
  if (int rc = launch_norm_rows(image_dev, image_dev + R, image_dev + 2 * R, R, R, nb, ws, false, s)) return rc;
  return launch_groups(ws, nb, R / rows_per_group, rows_per_group, take_sqrt, out_dev, s);
}

int fjagg_center_fold_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const float* c_dev,
                            const void* center_dev, void* out_dev, int flags, void* stream) {
  center_err[0] = 0;
  if (int rc = center_check(in_dtype, K, flags, FJAGG_NONTEMPORAL)) return rc;
  if (int rc = dense_check(x_dev, ld, K, P, center_dev, out_dev)) return rc;
  if (!c_dev) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: null pointer argument");
  return launch_fold_dense(reinterpret_cast<const uint8_t*>(x_dev), ld, (int)K, P, c_dev,
                           reinterpret_cast<const uint8_t*>(center_dev), reinterpret_cast<uint8_t*>(out_dev),
                           (flags & FJAGG_NONTEMPORAL) != 0, reinterpret_cast<hipStream_t>(stream));
}

int fjagg_center_fold_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, const float* c_dev,
                           int flags, void* stream) {
  center_err[0] = 0;
  if (int rc = center_check(in_dtype, K, flags, FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (int rc = plan_check(image_dev, L, nblk)) return rc;
  if (!c_dev) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: null pointer argument");
  const int64_t* cptrs = image_dev + K * L + 2 * (int64_t)L + 2 * nblk;
  return launch_fold_ptrs(image_dev, L, (int)K, nblk, (flags & FJAGG_UNALIGNED) ? 1 : 4, cptrs, c_dev,
                          (flags & FJAGG_NONTEMPORAL) != 0, reinterpret_cast<hipStream_t>(stream));
}

int64_t fjagg_center_clip_workspace_bytes(int64_t K, int64_t L, int64_t max_n) {
  if (K < 1 || L < 1 || max_n < 0) return 0;
  return round16(K * 4) + K * L * norm_blocks(max_n) * 4;
}

int fjagg_center_clip_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                            const int64_t* leaf_tab_dev, int64_t L, int64_t max_n, float tau, int64_t iterations,
                            const void* center_dev, void* out_dev, float* distances_dev, float* factors_dev,
                            void* ws_dev, int64_t ws_bytes, int flags, void* stream) {
  center_err[0] = 0;
  if (int rc = center_check(in_dtype, K, flags, FJAGG_NONTEMPORAL)) return rc;
  if (int rc = dense_check(x_dev, ld, K, P, center_dev, out_dev)) return rc;
  if (int rc = round_check(tau, iterations, distances_dev, factors_dev)) return rc;
  if (L < 1 || L >= (1 << 22) || (!leaf_tab_dev && L != 1) || max_n < 0 || max_n > P)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: bad leaf table (L=%lld, max_n=%lld)", (long long)L,
                (long long)max_n);
  if (!leaf_tab_dev) max_n = P;
  const int64_t need = fjagg_center_clip_workspace_bytes(K, L, max_n);
  if (!ws_dev || ws_bytes < need)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: needs %lld workspace bytes", (long long)need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* x = reinterpret_cast<const uint8_t*>(x_dev);
  uint8_t* out = reinterpret_cast<uint8_t*>(out_dev);
  float* q = reinterpret_cast<float*>(ws_dev);
  float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(ws_dev) + round16(K * 4));
  const int64_t nb = norm_blocks(max_n);
  const bool nt = (flags & FJAGG_NONTEMPORAL) != 0;
  for (int64_t l = 0; l < iterations; ++l) {
    const uint8_t* cen = l == 0 ? reinterpret_cast<const uint8_t*>(center_dev) : out;
    if (int rc = launch_norm_slab(x, ld * 4, P, leaf_tab_dev, L, cen, K * L, nb, part, nt, s)) return rc;
    if (int rc = launch_groups(part, nb, K, L, 0, q, s)) return rc;
    if (int rc = fjagg_clip_scales(q, K, tau, distances_dev + l * K, factors_dev + l * K, stream)) return rc;
    if (int rc = launch_fold_dense(x, ld, (int)K, P, factors_dev + l * K, cen, out, nt, s)) return rc;
  }
  return FJAGG_OK;
}

int fjagg_center_clip_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t max_n,
                           float tau, int64_t iterations, float* distances_dev, float* factors_dev, void* ws_dev,
                           int64_t ws_bytes, int flags, void* stream) {
  center_err[0] = 0;
  if (int rc = center_check(in_dtype, K, flags, FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (int rc = plan_check(image_dev, L, nblk)) return rc;
  if (int rc = round_check(tau, iterations, distances_dev, factors_dev)) return rc;
  if (max_n < 0 || max_n * 4 > kCenterMaxRowBytes) return refuse(FJAGG_EUNSUPPORTED, "centered clipping: rows <= 1 GiB");
  const int64_t need = fjagg_center_clip_workspace_bytes(K, L, max_n);
  if (!ws_dev || ws_bytes < need)
    return refuse(FJAGG_EUNSUPPORTED, "centered clipping: needs %lld workspace bytes", (long long)need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* q = reinterpret_cast<float*>(ws_dev);
  float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(ws_dev) + round16(K * 4));
  const int64_t* out_ptrs = image_dev + K * L;
  const int64_t* leaf_n = out_ptrs + L;
  const int64_t* center_ptrs = leaf_n + L + 2 * nblk;
  const int64_t nb = norm_blocks(max_n);
  const bool nt = (flags & FJAGG_NONTEMPORAL) != 0;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;
  for (int64_t l = 0; l < iterations; ++l) {
    const int64_t* cptrs = l == 0 ? center_ptrs : out_ptrs;
    if (int rc = launch_norm_rows(image_dev, leaf_n, cptrs, L, K * L, nb, part, nt, s)) return rc;
    if (int rc = launch_groups(part, nb, K, L, 0, q, s)) return rc;
    if (int rc = fjagg_clip_scales(q, K, tau, distances_dev + l * K, factors_dev + l * K, stream)) return rc;
    if (int rc = launch_fold_ptrs(image_dev, L, (int)K, nblk, V, cptrs, factors_dev + l * K, nt, s)) return rc;
  }
  return FJAGG_OK;
}

}  // extern "C"
