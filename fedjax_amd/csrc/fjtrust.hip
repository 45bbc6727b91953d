// fjtrust.hip — FLTrust (Cao, Fang, Liu and Gong, NDSS 2021): the trust-weighted mean of the client
// deltas against a server delta g (include/fjagg.h: fjagg_dotsq_rows, fjagg_dotsq_dense,
// fjagg_fltrust_select, fjagg_fltrust_dense / _ptrs). A round:
//
//   q_s = sum fl(g[p]^2)                                          fjagg_l2sq_rows itself
//   a_k = sum fl(x_k[p] g[p]);  q_k = sum fl(x_k[p]^2)            the row pass, ONE read of x_k
//   cos_k, ts_k, c_k, T, r and the member tables                  fjtrust_dev.h, one workgroup
//   y = +0;  s = +0; s = fl(s + fl(x_m[p] c_m)), m in the tables; y[p] = fl(s r)
//                                                                 fjagg_wsum_group_*_dev, G = 1
//
// The row pass is l2sq_centered_block's shape with two accumulators: eight loads of each operand in
// flight per lane, the deltas non-temporal so the stream does not evict g (which every client
// re-reads), both lane sums ascending and reduced by k_l2sq_rows' tree, two partials per (row,
// block). q_k therefore has fjagg_l2sq_rows' bits and a_k its order. A client with c_k = 0 is not
// in the tables, so the fold never loads it. Nothing visits the host or synchronises. Float32 only;
// no FMA (the library is built with contraction off).
#include "fjagg_dev.h"
#include "fjtrust_dev.h"

// fjagg_last_error()'s thread-local buffer under a name of this file's (see fjcenter.hip for why
// fjagg_dev.h's declaration, fail() and check_launch() are not used here).
extern __attribute__((visibility("hidden"))) __thread char trust_err[512] __asm__("fjagg_g_err");

namespace {

int refuse(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(trust_err, sizeof(trust_err), fmt, ap);
  va_end(ap);
  return code;
}

int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(FJAGG_EHIP, "%s: %s", what, hipGetErrorString(e));
  return FJAGG_OK;
}

constexpr int kTrustMaxClients = fjtrust::kMaxClients;
constexpr int64_t kTrustMaxRowBytes = 1ll << 30;
constexpr int64_t kDotPer = 64 * 1024;  // elements per block: fjagg_l2sq_rows' partition
constexpr int kMaxGridY = 65535;
constexpr int kSelectThreads = 1024;
constexpr int kSelectPer = kTrustMaxClients / kSelectThreads;  // clients a lane of the select owns

// ------------------------------------------------------------------ row pass
// Block blockIdx.x of one row: sa = sum fl(x[e] g[e]) and sq = sum fl(x[e]^2) over elements
// [b*per, (b+1)*per) of the row's n, each in k_l2sq_rows' order exactly: lane t adds elements
// t, t + 256, ... ascending from +0, then the xor shuffle tree 32 .. 1, then the four wave sums in
// order. NT: the deltas are loaded non-temporal; g never is.
template <bool NT>
__device__ __forceinline__ void dotsq_block(const uint8_t* __restrict__ x, const uint8_t* __restrict__ g, int64_t n,
                                            int64_t per, float* __restrict__ slot_a, float* __restrict__ slot_q) {
  const int64_t e0 = (int64_t)blockIdx.x * per;
  const int64_t e1 = (e0 + per < n) ? e0 + per : n;
  float sa = 0.f, sq = 0.f;
  int64_t e = e0 + threadIdx.x;
  constexpr int kAhead = 8;
  for (; e + (kAhead - 1) * (int64_t)kThreads < e1; e += kAhead * (int64_t)kThreads) {
    float a[kAhead], c[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j)
      a[j] = __uint_as_float(load_unit_ptr<FJAGG_F32, 1, NT>(x + (e + j * (int64_t)kThreads) * 4));
#pragma unroll
    for (int j = 0; j < kAhead; ++j)
      c[j] = __uint_as_float(load_unit_ptr<FJAGG_F32, 1, false>(g + (e + j * (int64_t)kThreads) * 4));
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      sa = __fadd_rn(sa, __fmul_rn(a[j], c[j]));
      sq = __fadd_rn(sq, __fmul_rn(a[j], a[j]));
    }
  }
  for (; e < e1; e += kThreads) {
    const float a = __uint_as_float(load_unit_ptr<FJAGG_F32, 1, NT>(x + e * 4));
    const float c = __uint_as_float(load_unit_ptr<FJAGG_F32, 1, false>(g + e * 4));
    sa = __fadd_rn(sa, __fmul_rn(a, c));
    sq = __fadd_rn(sq, __fmul_rn(a, a));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa = __fadd_rn(sa, __shfl_xor(sa, o, 64));
    sq = __fadd_rn(sq, __shfl_xor(sq, o, 64));
  }
  __shared__ float red[2][kThreads / 64];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sa;
    red[1][threadIdx.x >> 6] = sq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = red[0][0], tq = red[1][0];
#pragma unroll
    for (int i = 1; i < kThreads / 64; ++i) {
      ta = __fadd_rn(ta, red[0][i]);
      tq = __fadd_rn(tq, red[1][i]);
    }
    *slot_a = ta;
    *slot_q = tq;
  }
}

// Rows from tables: row r = r0 + blockIdx.y is at ptrs[r], has ns[r % mod] elements and its shared
// vector at ref[r % mod]. mod = R: one entry per row (fjagg_dotsq_rows' image); mod = L: the rows
// are a [K, L] leaf table with sizes and server leaves per leaf. The dot partials are ws[0 .. R*nb),
// the square partials ws[R*nb .. 2*R*nb), nb = gridDim.x.
template <bool NT>
__global__ __launch_bounds__(kThreads) void k_dotsq_rows(const int64_t* __restrict__ ptrs,
                                                         const int64_t* __restrict__ ns,
                                                         const int64_t* __restrict__ ref, int64_t mod, int64_t r0,
                                                         int64_t R, int64_t per, float* __restrict__ ws) {
  const int64_t r = r0 + blockIdx.y, l = r % mod;
  float* slot = ws + r * gridDim.x + blockIdx.x;
  dotsq_block<NT>(reinterpret_cast<const uint8_t*>(ptrs[r]), reinterpret_cast<const uint8_t*>(ref[l]), ns[l], per,
                  slot, slot + R * gridDim.x);
}

// Rows of a dense slab: row r = k*L + l is leaf l of client k, elements [off[l], off[l] + n[l]) of
// slab row k and of g (tab = off[L] | n[L]; no table: one leaf, the whole row).
template <bool NT>
__global__ __launch_bounds__(kThreads) void k_dotsq_slab(const uint8_t* __restrict__ x, int64_t ld_bytes, int64_t P,
                                                         const int64_t* __restrict__ tab, int64_t L,
                                                         const uint8_t* __restrict__ g, int64_t r0, int64_t R,
                                                         int64_t per, float* __restrict__ ws) {
  const int64_t r = r0 + blockIdx.y, k = r / L, l = r - k * L;
  const int64_t off = tab ? tab[l] : 0, n = tab ? tab[L + l] : P;
  float* slot = ws + r * gridDim.x + blockIdx.x;
  dotsq_block<NT>(x + k * ld_bytes + off * 4, g + off * 4, n, per, slot, slot + R * gridDim.x);
}

// dot[g] / sq[g] = the partials of rows [g*rows_per_group, (g+1)*rows_per_group), nb each, added in
// order from +0 (fjtrust::combine: fjagg_l2sq_rows' combine)
__global__ void k_dotsq_groups(const float* __restrict__ ws, int64_t nb, int64_t G, int64_t rows_per_group,
                               float* __restrict__ dot, float* __restrict__ sq) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int64_t n = rows_per_group * nb;
  dot[g] = fjtrust::combine(ws + g * n, n);
  sq[g] = fjtrust::combine(ws + G * n + g * n, n);
}

// ------------------------------------------------------------------ selection
// ONE workgroup of 1024 lanes; lane t owns the clients [t*kSelectPer, (t+1)*kSelectPer) below K, so a
// lane's members are consecutive in the member order and an exclusive scan of the lanes' member
// counts places them. Lane 0 alone adds T, in client order. Every order entry written is a client
// index k < K or the pad 0.
__global__ __launch_bounds__(kSelectThreads) void k_fltrust_select(
    const float* __restrict__ dot, const float* __restrict__ sq, const float* __restrict__ server_sq, int K,
    double* __restrict__ cos_out, double* __restrict__ trust_out, float* __restrict__ factors_out,
    float* __restrict__ norms_out, float* __restrict__ server_norm_out, double* __restrict__ total_out,
    int32_t* __restrict__ count_out, int32_t* __restrict__ order, int32_t* __restrict__ seg,
    float* __restrict__ wperm, float* __restrict__ gscale) {
  __shared__ double ts[kTrustMaxClients];
  __shared__ int scan[2][kSelectThreads];
  const int t = threadIdx.x, k0 = t * kSelectPer;
  const float qs = server_sq[0];
  float c[kSelectPer];
  int mine = 0;
#pragma unroll
  for (int i = 0; i < kSelectPer; ++i) {
    const int k = k0 + i;
    c[i] = 0.0f;
    if (k < K) {
      const float q = sq[k];
      const fjtrust::Trust tr = fjtrust::trust_of(dot[k], q, qs);
      c[i] = tr.c;
      ts[k] = tr.ts;
      cos_out[k] = tr.cos;
      trust_out[k] = tr.ts;
      factors_out[k] = tr.c;
      norms_out[k] = fjtrust::norm_of(q);
      mine += tr.c > 0.0f;
    }
  }
  scan[0][t] = mine;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < kSelectThreads; d <<= 1) {  // inclusive Hillis-Steele scan, double-buffered
    const int v = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0);
    scan[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  const int count = scan[cur][kSelectThreads - 1];
  int p = scan[cur][t] - mine;
#pragma unroll
  for (int i = 0; i < kSelectPer; ++i)
    if (c[i] > 0.0f) {  // (only a k < K has c > 0)
      order[p] = k0 + i;
      wperm[p] = c[i];
      ++p;
    }
  for (int j = count + t; j < K; j += kSelectThreads) {
    order[j] = 0;
    wperm[j] = 0.0f;
  }
  if (t == 0) {
    const double T = fjtrust::trust_total(ts, K);
    *total_out = T;
    *count_out = count;
    *server_norm_out = fjtrust::norm_of(qs);
    seg[0] = 0;
    seg[1] = count;
    gscale[0] = fjtrust::total_scale(T);
  }
}

// ------------------------------------------------------------------ small helpers of the drivers
// fjagg_l2sq_rows' image ptrs[L] | n[L] of the server delta's leaves inside a dense vector
__global__ void k_server_image(const uint8_t* g, int64_t P, const int64_t* __restrict__ tab, int64_t L,
                               int64_t* __restrict__ img) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  img[l] = (int64_t)reinterpret_cast<uintptr_t>(g + (tab ? tab[l] : 0) * 4);
  img[L + l] = tab ? tab[L + l] : P;
}

// y[0 .. n) = +0 (a kernel, so a graph replay zeroes too)
__global__ __launch_bounds__(kThreads) void k_zero_dense(float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) y[i] = 0.f;
}

// every leaf blockIdx.y of a plan image: out_ptrs[l][0 .. leaf_n[l]) = +0
__global__ __launch_bounds__(kThreads) void k_zero_leaves(const int64_t* __restrict__ out_ptrs,
                                                          const int64_t* __restrict__ leaf_n) {
  float* y = reinterpret_cast<float*>(out_ptrs[blockIdx.y]);
  const int64_t n = leaf_n[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) y[i] = 0.f;
}

// slot j < count of the group image gets client order[j]'s L leaf pointers: fjselect.hip's gather over
// the same word rule (fjselect::gather_member_word) with the whole table as the bound, launched from
// here because fjagg_gather_member_ptrs refuses more than 1024 clients
__global__ __launch_bounds__(kThreads) void k_gather_trusted(const int64_t* __restrict__ all, int L, int K,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ seg,
                                                             int64_t* __restrict__ group) {
  int count = seg[1] - seg[0];
  if (count > K) count = K;
  const int64_t n = (int64_t)count * L;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads)
    fjselect::gather_member_word(all, L, K, order, idx, group);
}

// ------------------------------------------------------------------ host side
inline int64_t dot_blocks(int64_t max_n) { return max_n > 0 ? (max_n + kDotPer - 1) / kDotPer : 1; }
inline int64_t round16(int64_t b) { return (b + 15) & ~(int64_t)15; }

int launch_rows(const int64_t* ptrs, const int64_t* ns, const int64_t* ref, int64_t mod, int64_t R, int64_t nb,
                float* ws, bool nt, hipStream_t s) {
  for (int64_t r0 = 0; r0 < R; r0 += kMaxGridY) {
    const int64_t nr = R - r0 < kMaxGridY ? R - r0 : kMaxGridY;
    const dim3 grid((unsigned)nb, (unsigned)nr);
    if (nt)
      hipLaunchKernelGGL(k_dotsq_rows<true>, grid, dim3(kThreads), 0, s, ptrs, ns, ref, mod, r0, R, kDotPer, ws);
    else
      hipLaunchKernelGGL(k_dotsq_rows<false>, grid, dim3(kThreads), 0, s, ptrs, ns, ref, mod, r0, R, kDotPer, ws);
    if (int rc = launched("k_dotsq_rows")) return rc;
  }
  return FJAGG_OK;
}

int launch_slab(const uint8_t* x, int64_t ldb, int64_t P, const int64_t* tab, int64_t L, const uint8_t* g, int64_t R,
                int64_t nb, float* ws, bool nt, hipStream_t s) {
  for (int64_t r0 = 0; r0 < R; r0 += kMaxGridY) {
    const int64_t nr = R - r0 < kMaxGridY ? R - r0 : kMaxGridY;
    const dim3 grid((unsigned)nb, (unsigned)nr);
    if (nt)
      hipLaunchKernelGGL(k_dotsq_slab<true>, grid, dim3(kThreads), 0, s, x, ldb, P, tab, L, g, r0, R, kDotPer, ws);
    else
      hipLaunchKernelGGL(k_dotsq_slab<false>, grid, dim3(kThreads), 0, s, x, ldb, P, tab, L, g, r0, R, kDotPer, ws);
    if (int rc = launched("k_dotsq_slab")) return rc;
  }
  return FJAGG_OK;
}

int launch_groups(const float* ws, int64_t nb, int64_t G, int64_t rows_per_group, float* dot, float* sq,
                  hipStream_t s) {
  hipLaunchKernelGGL(k_dotsq_groups, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, ws, nb, G, rows_per_group, dot,
                     sq);
  return launched("k_dotsq_groups");
}

int launch_select(const float* dot, const float* sq, const float* server_sq, int64_t K, double* cosv, double* trust,
                  float* factors, float* norms, float* server_norm, double* total, int32_t* count, int32_t* order,
                  int32_t* seg, float* wperm, float* gscale, hipStream_t s) {
  hipLaunchKernelGGL(k_fltrust_select, dim3(1), dim3(kSelectThreads), 0, s, dot, sq, server_sq, (int)K, cosv, trust,
                     factors, norms, server_norm, total, count, order, seg, wperm, gscale);
  return launched("k_fltrust_select");
}

int common_check(const char* what, int in_dtype, int64_t K, int flags, int allowed) {
  if (in_dtype != FJAGG_F32) return refuse(FJAGG_EUNSUPPORTED, "%s: float32 deltas, server delta and output only", what);
  if (flags & ~allowed) return refuse(FJAGG_EUNSUPPORTED, "%s: unsupported flags 0x%x", what, flags & ~allowed);
  if (K < 1 || K > kTrustMaxClients)
    return refuse(FJAGG_EUNSUPPORTED, "%s: 1 <= K <= %d clients (got %lld)", what, kTrustMaxClients, (long long)K);
  return FJAGG_OK;
}

// the dense slab x[K][ld], its shared vector g[P] and, when given, an output y[P] that must touch
// neither (the fold's workgroups read every row while others store their columns of y)
int dense_check(const char* what, const void* x, int64_t ld, int64_t K, int64_t P, const void* g, const void* y,
                bool with_out) {
  if (P < 1 || ld < P)
    return refuse(FJAGG_EUNSUPPORTED, "%s: need 1 <= P <= ld (P=%lld, ld=%lld)", what, (long long)P, (long long)ld);
  if (P * 4 > kTrustMaxRowBytes) return refuse(FJAGG_EUNSUPPORTED, "%s: rows <= 1 GiB", what);
  if (!x || !g || (with_out && !y)) return refuse(FJAGG_EUNSUPPORTED, "%s: null pointer argument", what);
  if (!with_out) return FJAGG_OK;
  const uintptr_t a = reinterpret_cast<uintptr_t>(g), b = reinterpret_cast<uintptr_t>(y);
  if (a < b + (uintptr_t)P * 4 && b < a + (uintptr_t)P * 4)
    return refuse(FJAGG_EUNSUPPORTED, "%s: out overlaps the server delta", what);
  const unsigned __int128 x0 = reinterpret_cast<uintptr_t>(x),
                          x1 = x0 + ((unsigned __int128)(K - 1) * (uint64_t)ld + (uint64_t)P) * 4;
  if (b < x1 && x0 < (unsigned __int128)b + (uint64_t)P * 4)
    return refuse(FJAGG_EUNSUPPORTED, "%s: out overlaps the deltas (the slab's rows are read while out is written)",
                  what);
  return FJAGG_OK;
}

int leaf_table_check(const char* what, const int64_t* tab, int64_t L, int64_t* max_n, int64_t P) {
  if (L < 1 || L > kMaxGridY || (!tab && L != 1) || *max_n < 0 || *max_n > P)
    return refuse(FJAGG_EUNSUPPORTED, "%s: bad leaf table (1 <= L <= %d, 0 <= max_n <= P; L=%lld, max_n=%lld)", what,
                  kMaxGridY, (long long)L, (long long)*max_n);
  if (!tab) *max_n = P;
  return FJAGG_OK;
}

// the workspace of a whole round, carved in this order (every piece 16-byte aligned)
struct RoundWs {
  float *dot, *sq, *server_sq, *wperm, *gscale, *part;
  int32_t *order, *seg;
  int64_t* simg;
  int64_t bytes;
};
RoundWs carve(void* ws, int64_t K, int64_t L, int64_t max_n) {
  RoundWs w;
  const uintptr_t p = reinterpret_cast<uintptr_t>(ws);  // (null: only the size is wanted)
  int64_t at = 0;
  auto take = [&](int64_t bytes) {
    const uintptr_t q = p + (uintptr_t)at;
    at += round16(bytes);
    return q;
  };
  w.dot = reinterpret_cast<float*>(take(K * 4));
  w.sq = reinterpret_cast<float*>(take(K * 4));
  w.server_sq = reinterpret_cast<float*>(take(4));
  w.order = reinterpret_cast<int32_t*>(take(K * 4));
  w.seg = reinterpret_cast<int32_t*>(take(8));
  w.wperm = reinterpret_cast<float*>(take(K * 4));
  w.gscale = reinterpret_cast<float*>(take(4));
  w.simg = reinterpret_cast<int64_t*>(take(2 * L * 8));
  w.part = reinterpret_cast<float*>(take(2 * K * L * dot_blocks(max_n) * 4));
  w.bytes = at;
  return w;
}

int outputs_check(const char* what, const void* a, const void* b, const void* c, const void* d, const void* e,
                  const void* f, const void* g) {
  if (!a || !b || !c || !d || !e || !f || !g) return refuse(FJAGG_EUNSUPPORTED, "%s: null pointer argument", what);
  return FJAGG_OK;
}

// the dense output y[P] must touch neither the workspace nor a diagnostics buffer: the selection and
// the zeroing kernel write them while later launches read the tables
int out_apart_check(const char* what, const void* y, int64_t P, const void* ws, int64_t ws_bytes, int64_t K,
                    const void* cosv, const void* trust, const void* factors, const void* norms,
                    const void* server_norm, const void* total, const void* count) {
  const uintptr_t y0 = reinterpret_cast<uintptr_t>(y), y1 = y0 + (uintptr_t)P * 4;
  const struct {
    const void* p;
    int64_t bytes;
  } other[] = {{ws, ws_bytes}, {cosv, K * 8}, {trust, K * 8}, {factors, K * 4}, {norms, K * 4},
               {server_norm, 4},  {total, 8},   {count, 4}};
  for (const auto& o : other) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(o.p);
    if (a < y1 && y0 < a + (uintptr_t)o.bytes)
      return refuse(FJAGG_EUNSUPPORTED, "%s: out overlaps the workspace or a diagnostics buffer", what);
  }
  return FJAGG_OK;
}

int workspace_check(const char* what, const void* ws, int64_t ws_bytes, int64_t need) {
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15))
    return refuse(FJAGG_EUNSUPPORTED, "%s: needs %lld workspace bytes, 16-byte aligned (got %lld)", what,
                  (long long)need, (long long)ws_bytes);
  return FJAGG_OK;
}

}  // namespace

extern "C" {

int64_t fjagg_dotsq_rows_workspace_bytes(int64_t R, int64_t max_n) {
  if (R < 1 || max_n < 0) return 0;
  return 2 * R * dot_blocks(max_n) * 4;
}

int fjagg_dotsq_rows(int in_dtype, const int64_t* image_dev, int64_t R, int64_t max_n, int64_t rows_per_group,
                     float* dot_dev, float* sq_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  trust_err[0] = 0;
  const char* what = "dot and square rows";
  if (in_dtype != FJAGG_F32) return refuse(FJAGG_EUNSUPPORTED, "%s: float32 rows and shared vectors only", what);
  if (R < 1 || max_n < 0 || rows_per_group < 1 || R % rows_per_group)
    return refuse(FJAGG_EUNSUPPORTED, "%s: bad row grouping (R=%lld, rows_per_group=%lld)", what, (long long)R,
                  (long long)rows_per_group);
  if (max_n * 4 > kTrustMaxRowBytes) return refuse(FJAGG_EUNSUPPORTED, "%s: rows <= 1 GiB", what);
  const int64_t nb = dot_blocks(max_n), need = 2 * R * nb * 4;
  if (!ws_dev || ws_bytes < need || !image_dev || !dot_dev || !sq_dev)
    return refuse(FJAGG_EUNSUPPORTED, "%s: need %lld workspace bytes and no null pointer", what, (long long)need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(ws_dev);
  if (int rc = launch_rows(image_dev, image_dev + R, image_dev + 2 * R, R, R, nb, ws, false, s)) return rc;
  return launch_groups(ws, nb, R / rows_per_group, rows_per_group, dot_dev, sq_dev, s);
}

int fjagg_dotsq_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const int64_t* leaf_tab_dev,
                      int64_t L, int64_t max_n, const void* ref_dev, float* dot_dev, float* sq_dev, void* ws_dev,
                      int64_t ws_bytes, int flags, void* stream) {
  trust_err[0] = 0;
  const char* what = "dot and square rows";
  if (int rc = common_check(what, in_dtype, K, flags, FJAGG_NONTEMPORAL)) return rc;
  if (int rc = dense_check(what, x_dev, ld, K, P, ref_dev, nullptr, false)) return rc;
  if (int rc = leaf_table_check(what, leaf_tab_dev, L, &max_n, P)) return rc;
  const int64_t nb = dot_blocks(max_n), need = 2 * K * L * nb * 4;
  if (!ws_dev || ws_bytes < need || !dot_dev || !sq_dev)
    return refuse(FJAGG_EUNSUPPORTED, "%s: need %lld workspace bytes and no null pointer", what, (long long)need);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(ws_dev);
  if (int rc = launch_slab(reinterpret_cast<const uint8_t*>(x_dev), ld * 4, P, leaf_tab_dev, L,
                           reinterpret_cast<const uint8_t*>(ref_dev), K * L, nb, ws, (flags & FJAGG_NONTEMPORAL) != 0,
                           s))
    return rc;
  return launch_groups(ws, nb, K, L, dot_dev, sq_dev, s);
}

int fjagg_fltrust_select(const float* dot_dev, const float* sq_dev, const float* server_sq_dev, int64_t K,
                         double* cos_dev, double* trust_dev, float* factors_dev, float* norms_dev,
                         float* server_norm_dev, double* total_dev, int32_t* count_dev, int32_t* order_dev,
                         int32_t* seg_dev, float* wperm_dev, float* gscale_dev, void* stream) {
  trust_err[0] = 0;
  const char* what = "fltrust select";
  if (K < 1 || K > kTrustMaxClients)
    return refuse(FJAGG_EUNSUPPORTED, "%s: 1 <= K <= %d clients (got %lld)", what, kTrustMaxClients, (long long)K);
  if (!dot_dev || !sq_dev || !server_sq_dev || !order_dev || !seg_dev || !wperm_dev || !gscale_dev)
    return refuse(FJAGG_EUNSUPPORTED, "%s: null pointer argument", what);
  if (int rc = outputs_check(what, cos_dev, trust_dev, factors_dev, norms_dev, server_norm_dev, total_dev, count_dev))
    return rc;
  return launch_select(dot_dev, sq_dev, server_sq_dev, K, cos_dev, trust_dev, factors_dev, norms_dev, server_norm_dev,
                       total_dev, count_dev, order_dev, seg_dev, wperm_dev, gscale_dev,
                       reinterpret_cast<hipStream_t>(stream));
}

int64_t fjagg_fltrust_workspace_bytes(int64_t K, int64_t L, int64_t max_n) {
  if (K < 1 || L < 1 || max_n < 0) return 0;
  return carve(nullptr, K, L, max_n).bytes;
}

int fjagg_fltrust_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const int64_t* leaf_tab_dev,
                        int64_t L, int64_t max_n, const void* server_dev, void* out_dev, double* cos_dev,
                        double* trust_dev, float* factors_dev, float* norms_dev, float* server_norm_dev,
                        double* total_dev, int32_t* count_dev, void* ws_dev, int64_t ws_bytes, int flags, void* stream) {
  trust_err[0] = 0;
  const char* what = "fltrust";
  if (int rc = common_check(what, in_dtype, K, flags, FJAGG_NONTEMPORAL)) return rc;
  if (int rc = dense_check(what, x_dev, ld, K, P, server_dev, out_dev, true)) return rc;
  if (int rc = leaf_table_check(what, leaf_tab_dev, L, &max_n, P)) return rc;
  if (int rc = outputs_check(what, cos_dev, trust_dev, factors_dev, norms_dev, server_norm_dev, total_dev, count_dev))
    return rc;
  if (int rc = workspace_check(what, ws_dev, ws_bytes, fjagg_fltrust_workspace_bytes(K, L, max_n))) return rc;
  if (int rc = out_apart_check(what, out_dev, P, ws_dev, fjagg_fltrust_workspace_bytes(K, L, max_n), K, cos_dev, trust_dev,
                               factors_dev, norms_dev, server_norm_dev, total_dev, count_dev))
    return rc;
  const RoundWs w = carve(ws_dev, K, L, max_n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint8_t* x = reinterpret_cast<const uint8_t*>(x_dev);
  const uint8_t* g = reinterpret_cast<const uint8_t*>(server_dev);
  const int64_t nb = dot_blocks(max_n);
  const bool nt = (flags & FJAGG_NONTEMPORAL) != 0;
  // the server norm: fjagg_l2sq_rows over the server delta's leaves (its partials fit the row pass's)
  hipLaunchKernelGGL(k_server_image, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, s, g, P, leaf_tab_dev, L, w.simg);
  if (int rc = launched("k_server_image")) return rc;
  if (int rc = fjagg_l2sq_rows(FJAGG_F32, w.simg, L, max_n, L, 0, w.server_sq, w.part, L * nb * 4, stream)) return rc;
  if (int rc = launch_slab(x, ld * 4, P, leaf_tab_dev, L, g, K * L, nb, w.part, nt, s)) return rc;
  if (int rc = launch_groups(w.part, nb, K, L, w.dot, w.sq, s)) return rc;
  if (int rc = launch_select(w.dot, w.sq, w.server_sq, K, cos_dev, trust_dev, factors_dev, norms_dev, server_norm_dev,
                             total_dev, count_dev, w.order, w.seg, w.wperm, w.gscale, s))
    return rc;
  int64_t zb = (P + kThreads - 1) / kThreads;
  if (zb > 4096) zb = 4096;
  hipLaunchKernelGGL(k_zero_dense, dim3((unsigned)zb), dim3(kThreads), 0, s, reinterpret_cast<float*>(out_dev), P);
  if (int rc = launched("k_zero_dense")) return rc;
  return fjagg_wsum_group_dense_dev(FJAGG_F32, x_dev, ld, K, P, K, w.order, w.seg, w.wperm, w.gscale, out_dev,
                                    FJAGG_SCALE | (flags & FJAGG_NONTEMPORAL), stream);
}

int fjagg_fltrust_ptrs(int in_dtype, const int64_t* image_all_dev, int64_t* image_group_dev, int L, int64_t K,
                       int64_t nblk, int64_t max_n, double* cos_dev, double* trust_dev, float* factors_dev,
                       float* norms_dev, float* server_norm_dev, double* total_dev, int32_t* count_dev, void* ws_dev,
                       int64_t ws_bytes, int flags, void* stream) {
  trust_err[0] = 0;
  const char* what = "fltrust";
  if (int rc = common_check(what, in_dtype, K, flags, FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L > kMaxGridY)
    return refuse(FJAGG_EUNSUPPORTED, "%s: bad plan (nblk=%lld, 1 <= L <= %d, got %d)", what, (long long)nblk,
                  kMaxGridY, L);
  if (max_n < 0 || max_n * 4 > kTrustMaxRowBytes) return refuse(FJAGG_EUNSUPPORTED, "%s: rows <= 1 GiB", what);
  if (!image_all_dev || !image_group_dev) return refuse(FJAGG_EUNSUPPORTED, "%s: null pointer argument", what);
  if (int rc = outputs_check(what, cos_dev, trust_dev, factors_dev, norms_dev, server_norm_dev, total_dev, count_dev))
    return rc;
  if (int rc = workspace_check(what, ws_dev, ws_bytes, fjagg_fltrust_workspace_bytes(K, L, max_n))) return rc;
  const RoundWs w = carve(ws_dev, K, L, max_n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t* server_img = image_all_dev + K * L;  // server_ptrs[L] | leaf_n[L]: fjagg_l2sq_rows' image
  const int64_t* out_ptrs = image_group_dev + K * L;
  const int64_t nb = dot_blocks(max_n);
  const bool nt = (flags & FJAGG_NONTEMPORAL) != 0;
  if (int rc = fjagg_l2sq_rows(FJAGG_F32, server_img, L, max_n, L, 0, w.server_sq, w.part, (int64_t)L * nb * 4, stream))
    return rc;
  if (int rc = launch_rows(image_all_dev, server_img + L, server_img, L, K * L, nb, w.part, nt, s)) return rc;
  if (int rc = launch_groups(w.part, nb, K, L, w.dot, w.sq, s)) return rc;
  if (int rc = launch_select(w.dot, w.sq, w.server_sq, K, cos_dev, trust_dev, factors_dev, norms_dev, server_norm_dev,
                             total_dev, count_dev, w.order, w.seg, w.wperm, w.gscale, s))
    return rc;
  if (max_n > 0) {
    int64_t zb = (max_n + kThreads - 1) / kThreads;
    if (zb > 1024) zb = 1024;
    hipLaunchKernelGGL(k_zero_leaves, dim3((unsigned)zb, (unsigned)L), dim3(kThreads), 0, s, out_ptrs, out_ptrs + L);
    if (int rc = launched("k_zero_leaves")) return rc;
  }
  int64_t gb = (K * L + kThreads - 1) / kThreads;
  if (gb > 1024) gb = 1024;
  hipLaunchKernelGGL(k_gather_trusted, dim3((unsigned)gb), dim3(kThreads), 0, s, image_all_dev, L, (int)K, w.order, w.seg,
                     image_group_dev);
  if (int rc = launched("k_gather_trusted")) return rc;
  return fjagg_wsum_group_ptrs_dev(FJAGG_F32, image_group_dev, L, K, K, nblk, w.seg, w.wperm, w.gscale,
                                   FJAGG_SCALE | (flags & (FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)), stream);
}

}  // extern "C"
