// fjrobust.hip — coordinate-wise trimmed mean and median over the client axis
// (include/fjagg.h: fjagg_trim_dense, fjagg_trim_ptrs; Yin et al., ICML 2018) and the mean
// around the median (fjagg_meamed_dense, fjagg_meamed_ptrs; Xie et al. 2018), Bulyan's second
// stage, also with its counts and row table read from device memory (fjagg_meamed_dense_dev,
// fjagg_meamed_ptrs_dev), where fjagg_bulyan_select wrote them. The trimmed mean and median also
// run over the means of buckets of s clients (fjagg_trim_bucket_dense, fjagg_trim_bucket_ptrs;
// Karimireddy, He and Jaggi, ICLR 2022), which lifts the client limit to 4096.
//
// Not a fold: every coordinate needs two order statistics of its K client values. One lane
// owns one column (fjrobust_dev.h has the per-column routine and the reasons for its shape):
// a wave reads 256 contiguous bytes of each client's row with 4-byte loads, so float32's own
// alignment is all a row needs, and writes one result per lane. The kernels are instantiated
// for a padded client count N = 16 / 32 / 64 / 128, chosen from K at launch; N = 16 sorts in
// registers alone, the wider ones stage their keys in N x 256 B of LDS per wave.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjagg.h"
#include "fjrobust_dev.h"

// The thread-local message behind fjagg_last_error() (defined in fjagg.hip). Declared __thread:
// the buffer has a constant initialiser, so no dynamic-initialisation wrapper stands between
// this file and it.
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

constexpr int64_t kTrimMaxRowBytes = 1ll << 30;
constexpr int kTrimMaxClients = 128;
constexpr int kBucketMaxClients = 4096;  // fjagg_trim_bucket_*: clients behind at most 128 buckets
constexpr int kMeamedMaxSlabRows = 1024;  // the Gram pass's client limit: Bulyan selects among so many

// Workgroup size per width: 256 lanes while the tile stays at 32 KiB, one wave above that
// (16 KiB at N = 64, 32 KiB at N = 128: five workgroups of a CU's 160 KiB). 256 lanes at every
// width (a 128 KiB tile at N = 128, one wave a SIMD) measured the same rate: DESIGN 3l.
template <int N> struct TrimShape { static constexpr int TPB = N <= 32 ? 256 : 64; };

// 4 bytes through a GLOBAL (address space 1) pointer: global_load / global_store, counted in
// vmcnt only, so the LDS waits of the sort do not wait for them (fjagg_dev.h load16_global).
typedef __attribute__((address_space(1))) uint32_t gu32;
template <bool NT>
__device__ __forceinline__ uint32_t load_bits(const uint32_t* p, uint32_t lane_off) {
  // p is uniform over the wave (an SGPR base), lane_off the lane's element offset from it: one
  // offset VGPR serves every client's load
  const gu32* g = (const gu32*)(reinterpret_cast<uintptr_t>(p)) + lane_off;
  if constexpr (NT) return __builtin_nontemporal_load(g);
  else return *g;
}
__device__ __forceinline__ void store_bits(uint32_t* p, uint32_t v) { *(gu32*)(reinterpret_cast<uintptr_t>(p)) = v; }

template <int N, int TPB>
__device__ __forceinline__ fjrobust::KeyPair* lane_tile() {
  if constexpr (N == 16) {
    return nullptr;
  } else {
    __shared__ fjrobust::KeyPair tile[(N / 2) * TPB];
    return tile + threadIdx.x;
  }
}

// Dense slab: client k's row at x + k*ld, columns [0, P). Lanes past P redo column P-1 and
// store nothing.
template <int N, bool NT>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_trim_dense(const uint32_t* __restrict__ x, int64_t ld, int K,
                                                                   int64_t P, int t, float scale, int do_scale,
                                                                   uint32_t* __restrict__ out) {
  constexpr int TPB = TrimShape<N>::TPB;
  const int64_t col0 = (int64_t)blockIdx.x * TPB, col = col0 + threadIdx.x;
  const bool valid = col < P;
  const uint32_t off = valid ? threadIdx.x : (uint32_t)(P - 1 - col0);
  const uint32_t* base = x + col0;
  auto load = [=](int k) { return load_bits<NT>(base + (int64_t)k * ld, off); };
  const uint32_t y = fjrobust::trim_column<N, TPB>(load, K, t, do_scale != 0, scale, lane_tile<N, TPB>());
  if (valid) store_bits(out + col, y);
}

// Pytree path over the plan image of fjagg_ptrs_plan_leaves (fjagg.hip k_ptrs: in_ptrs[K*L] |
// out_ptrs[L] | leaf_n[L] | blocks[2*nblk]). Plan entry blockIdx.x names an element range of one
// leaf — V-element units (V = 4, or 1 for a plan made with FJAGG_UNALIGNED), single elements
// with the element flag, or the leaf's tail past its last whole unit — and the 256 / TPB
// workgroups blockIdx.y of that entry walk it 256 columns at a time, as one 256-lane workgroup
// of the fold would.
template <int N, bool NT, class Column>
__device__ __forceinline__ void ptrs_walk(const int64_t* __restrict__ img, int L, int K, int V, Column column) {
  constexpr int TPB = TrimShape<N>::TPB;
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
  const int64_t e0 = tail ? n / V * V : (elem ? u0 : u0 * V);
  int64_t e1 = tail ? n : (elem ? u1 : u1 * V);
  if (e1 > n) e1 = n;
  uint32_t* ob = reinterpret_cast<uint32_t*>(out_ptrs[leaf]);
  fjrobust::KeyPair* tile = lane_tile<N, TPB>();
  for (int64_t g = e0 + (int64_t)blockIdx.y * TPB; g < e1; g += 256) {
    const int64_t col = g + threadIdx.x;
    const bool valid = col < e1;
    const uint32_t off = valid ? threadIdx.x : (uint32_t)(e1 - 1 - g);
    auto load = [=](int k) {
      return load_bits<NT>(reinterpret_cast<const uint32_t*>(in_ptrs[(int64_t)k * L + leaf]) + g, off);
    };
    const uint32_t y = column(load, tile);
    if (valid) store_bits(ob + col, y);
  }
}

template <int N, bool NT>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_trim_ptrs(const int64_t* __restrict__ img, int L, int K, int V,
                                                                  int t, float scale, int do_scale) {
  ptrs_walk<N, NT>(img, L, K, V, [=](auto load, fjrobust::KeyPair* tile) {
    return fjrobust::trim_column<N, TrimShape<N>::TPB>(load, K, t, do_scale != 0, scale, tile);
  });
}

// Bucketing (fjagg_trim_bucket_*): the same column routine over B = ceil(K / s) bucket means, each
// formed from s client loads where the routine asks for it (fjrobust_dev.h BucketLoad), so the
// sort reads every delta once and the sum once more, with no B x P temporary. The client table
// is int32 in device memory (null: the identity, the kernels' HP = false, so that no branch
// stands between the table reads); its index is uniform over the wave, so an entry is a scalar
// load, and BucketLoad clamps it into [0, K) before an address is formed.
struct BucketArgs {
  const int32_t* perm;
  int K, s, B;
  float inv_s, inv_last;
};
template <bool HP>
__device__ __forceinline__ auto bucket_table(const int32_t* __restrict__ perm) {
  return [=](int m) {
    if constexpr (HP) return perm[m];
    else return (int32_t)m;
  };
}

template <int N, bool NT, bool HP>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_trim_bucket_dense(const uint32_t* __restrict__ x, int64_t ld,
                                                                          int64_t P, const BucketArgs b, int t,
                                                                          float scale, int do_scale,
                                                                          uint32_t* __restrict__ out) {
  constexpr int TPB = TrimShape<N>::TPB;
  const int64_t col0 = (int64_t)blockIdx.x * TPB, col = col0 + threadIdx.x;
  const bool valid = col < P;
  const uint32_t off = valid ? threadIdx.x : (uint32_t)(P - 1 - col0);
  const uint32_t* base = x + col0;
  auto load = [=](int k) { return load_bits<NT>(base + (int64_t)k * ld, off); };
  auto bucket = fjrobust::bucket_load(load, bucket_table<HP>(b.perm), b.K, b.s, b.inv_s, b.inv_last);
  const uint32_t y = fjrobust::trim_column<N, TPB>(bucket, b.B, t, do_scale != 0, scale, lane_tile<N, TPB>());
  if (valid) store_bits(out + col, y);
}

template <int N, bool NT, bool HP>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_trim_bucket_ptrs(const int64_t* __restrict__ img, int L, int V,
                                                                         const BucketArgs b, int t, float scale,
                                                                         int do_scale) {
  ptrs_walk<N, NT>(img, L, b.K, V, [=](auto load, fjrobust::KeyPair* tile) {
    auto bucket = fjrobust::bucket_load(load, bucket_table<HP>(b.perm), b.K, b.s, b.inv_s, b.inv_last);
    return fjrobust::trim_column<N, TrimShape<N>::TPB>(bucket, b.B, t, do_scale != 0, scale, tile);
  });
}

// The mean around the median (fjrobust_dev.h around_median_column) over the same two layouts.
// Dense: participating client k is slab row rows.r[k]. The table travels in the kernel
// arguments and k is uniform over the wave, so a row's index is a scalar load from the argument
// segment: nothing is uploaded and no row outside the table is ever addressed.
constexpr int kMeamedMaxClients = 128;
struct MeamedRows {
  int32_t r[kMeamedMaxClients];
};

template <int N, bool NT>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_meamed_dense(const uint32_t* __restrict__ x, int64_t ld, int M,
                                                                     int64_t P, int keep, float scale, int do_scale,
                                                                     uint32_t* __restrict__ out,
                                                                     const MeamedRows rows) {
  constexpr int TPB = TrimShape<N>::TPB;
  const int64_t col0 = (int64_t)blockIdx.x * TPB, col = col0 + threadIdx.x;
  const bool valid = col < P;
  const uint32_t off = valid ? threadIdx.x : (uint32_t)(P - 1 - col0);
  const uint32_t* base = x + col0;
  const int32_t* rt = rows.r;
  auto load = [=](int k) { return load_bits<NT>(base + (int64_t)rt[k] * ld, off); };
  const uint32_t y =
      fjrobust::around_median_column<N, TPB>(load, M, keep, do_scale != 0, scale, lane_tile<N, TPB>());
  if (valid) store_bits(out + col, y);
}

template <int N, bool NT>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_meamed_ptrs(const int64_t* __restrict__ img, int L, int K,
                                                                    int V, int keep, float scale, int do_scale) {
  ptrs_walk<N, NT>(img, L, K, V, [=](auto load, fjrobust::KeyPair* tile) {
    return fjrobust::around_median_column<N, TrimShape<N>::TPB>(load, K, keep, do_scale != 0, scale, tile);
  });
}

// The same column routine with M, keep, scale and the row table read from device memory, where a
// select kernel wrote them (fjagg_bulyan_select): all uniform over the grid. The width N comes
// from the caller's bound M_max <= N. No address is formed from an unchecked table value: the
// count is clamped into [0, M_max], keep into [0, count], every row index into [0, K_rows), so a
// stale table can give a wrong result but never an access outside the slab. keep < 1 stores +0
// and loads no client row.
struct MeamedDevTables {
  int M, keep;
  float scale;
};
__device__ __forceinline__ MeamedDevTables meamed_tables(const int32_t* __restrict__ count_dev,
                                                         const int32_t* __restrict__ keep_dev,
                                                         const float* __restrict__ scale_dev, int M_max) {
  int M = count_dev[0], keep = keep_dev[0];
  M = M < 0 ? 0 : (M > M_max ? M_max : M);
  keep = keep < 0 ? 0 : (keep > M ? M : keep);
  return MeamedDevTables{M, keep, scale_dev[0]};
}

template <int N, bool NT>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_meamed_dense_dev(
    const uint32_t* __restrict__ x, int64_t ld, int K_rows, int M_max, int64_t P,
    const int32_t* __restrict__ rows_dev, const int32_t* __restrict__ count_dev,
    const int32_t* __restrict__ keep_dev, const float* __restrict__ scale_dev, int do_scale,
    uint32_t* __restrict__ out) {
  constexpr int TPB = TrimShape<N>::TPB;
  const int64_t col0 = (int64_t)blockIdx.x * TPB, col = col0 + threadIdx.x;
  const bool valid = col < P;
  const MeamedDevTables tb = meamed_tables(count_dev, keep_dev, scale_dev, M_max);
  if (tb.keep < 1) {  // uniform over the grid
    if (valid) store_bits(out + col, 0u);
    return;
  }
  const uint32_t off = valid ? threadIdx.x : (uint32_t)(P - 1 - col0);
  const uint32_t* base = x + col0;
  auto load = [=](int k) {  // k < M <= M_max: inside the table; the row clamped into the slab
    int r = rows_dev[k];
    r = r < 0 ? 0 : (r >= K_rows ? K_rows - 1 : r);
    return load_bits<NT>(base + (int64_t)r * ld, off);
  };
  const uint32_t y =
      fjrobust::around_median_column<N, TPB>(load, tb.M, tb.keep, do_scale != 0, tb.scale, lane_tile<N, TPB>());
  if (valid) store_bits(out + col, y);
}

// The image is laid out for M_max members; k_gather_rows has filled every slot.
template <int N, bool NT>
__global__ __launch_bounds__(TrimShape<N>::TPB) void k_meamed_ptrs_dev(
    const int64_t* __restrict__ img, int L, int M_max, int V, const int32_t* __restrict__ count_dev,
    const int32_t* __restrict__ keep_dev, const float* __restrict__ scale_dev, int do_scale) {
  const MeamedDevTables tb = meamed_tables(count_dev, keep_dev, scale_dev, M_max);
  ptrs_walk<N, NT>(img, L, M_max, V, [=](auto load, fjrobust::KeyPair* tile) {
    if (tb.keep < 1) return 0u;  // uniform: +0, nothing loaded
    return fjrobust::around_median_column<N, TrimShape<N>::TPB>(load, tb.M, tb.keep, do_scale != 0, tb.scale, tile);
  });
}

// Slot j of the group image (in_ptrs[M_max*L]) gets the L leaf pointers of client rows_dev[j],
// clamped into [0, K), from all = in_ptrs[K*L]. The select kernel repeats its last row past the
// count, so EVERY slot holds a client's pointers, whatever the count turns out to be.
__global__ __launch_bounds__(256) void k_gather_rows(const int64_t* __restrict__ all, int L, int K,
                                                     const int32_t* __restrict__ rows_dev, int M_max,
                                                     int64_t* __restrict__ group) {
  const int64_t n = (int64_t)M_max * L;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const int64_t j = idx / L, l = idx - j * L;
    int r = rows_dev[j];
    r = r < 0 ? 0 : (r >= K ? K - 1 : r);
    group[idx] = all[(int64_t)r * L + l];
  }
}

// what every column aggregate refuses for its dtype and flags
int flags_check(const char* who, int in_dtype, int flags, int allowed) {
  if (in_dtype != FJAGG_F32) return fail(FJAGG_EUNSUPPORTED, "%s: float32 deltas and output only", who);
  if (flags & FJAGG_ACCUMULATE)
    return fail(FJAGG_EUNSUPPORTED, "%s: order statistics do not accumulate (no FJAGG_ACCUMULATE)", who);
  if (flags & FJAGG_NARROW) return fail(FJAGG_EUNSUPPORTED, "%s: no FJAGG_NARROW plans", who);
  if (flags & FJAGG_HOST_TABLES)
    return fail(FJAGG_EUNSUPPORTED, "%s: device plan only (no FJAGG_HOST_TABLES)", who);
  if (flags & FJAGG_ZEROED_WS) return fail(FJAGG_EUNSUPPORTED, "%s: no norms (no FJAGG_ZEROED_WS)", who);
  if (flags & FJAGG_UNBALANCED) return fail(FJAGG_EUNSUPPORTED, "%s: no FJAGG_UNBALANCED", who);
  if (flags & ~allowed) return fail(FJAGG_EUNSUPPORTED, "%s: unsupported flags 0x%x", who, flags & ~allowed);
  return FJAGG_OK;
}

// what both aggregates refuse: the dtype, the flags and the client count
int column_check(const char* who, int in_dtype, int64_t K, int flags, int allowed) {
  if (int rc = flags_check(who, in_dtype, flags, allowed)) return rc;
  if (K < 1) return fail(FJAGG_EINVAL, "K must be >= 1 (got %lld)", (long long)K);
  if (K > kTrimMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "%s: K <= %d clients (got %lld)", who, kTrimMaxClients, (long long)K);
  return FJAGG_OK;
}

// fjagg_trim_bucket_*: the dtype and flags of fjagg_trim_*, then s, K, the bucket count B and t
int bucket_check(int in_dtype, int64_t K, int64_t s, int64_t t, int flags, int allowed) {
  if (int rc = flags_check("bucketed trimmed mean", in_dtype, flags, allowed)) return rc;
  if (s < 1) return fail(FJAGG_EINVAL, "bucketed trimmed mean: bucket size s >= 1 (got %lld)", (long long)s);
  if (K < 1) return fail(FJAGG_EINVAL, "K must be >= 1 (got %lld)", (long long)K);
  if (K > kBucketMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "bucketed trimmed mean: K <= %d clients (got %lld)", kBucketMaxClients,
                (long long)K);
  const int64_t B = (K + s - 1) / s;
  if (B > kTrimMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "bucketed trimmed mean: B = ceil(K / s) <= %d buckets (got %lld of K=%lld, s=%lld)",
                kTrimMaxClients, (long long)B, (long long)K, (long long)s);
  if (t < 0 || 2 * t >= B)
    return fail(FJAGG_EINVAL, "bucketed trimmed mean: need 0 <= 2t < B (t=%lld, B=%lld)", (long long)t, (long long)B);
  return FJAGG_OK;
}

int trim_check(int in_dtype, int64_t K, int64_t t, int flags, int allowed) {
  if (int rc = column_check("trimmed mean", in_dtype, K, flags, allowed)) return rc;
  if (t < 0 || 2 * t >= K)
    return fail(FJAGG_EINVAL, "trimmed mean: need 0 <= 2t < K (t=%lld, K=%lld)", (long long)t, (long long)K);
  return FJAGG_OK;
}

int meamed_check(int in_dtype, int64_t M, int64_t keep, int flags, int allowed) {
  if (int rc = column_check("mean around median", in_dtype, M, flags, allowed)) return rc;
  if (keep < 1 || keep > M)
    return fail(FJAGG_EINVAL, "mean around median: need 1 <= keep <= M (keep=%lld, M=%lld)", (long long)keep,
                (long long)M);
  return FJAGG_OK;
}

template <int N, bool NT>
int launch_trim_dense(const uint32_t* x, int64_t ld, int K, int64_t P, int t, float scale, int ds, uint32_t* y,
                      hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)((P + TPB - 1) / TPB));
  hipLaunchKernelGGL((k_trim_dense<N, NT>), grid, dim3(TPB), 0, s, x, ld, K, P, t, scale, ds, y);
  return check_launch("k_trim_dense");
}

template <int N, bool NT>
int launch_trim_ptrs(const int64_t* img, int L, int K, int64_t nblk, int V, int t, float scale, int ds,
                     hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)nblk, 256 / TPB);
  hipLaunchKernelGGL((k_trim_ptrs<N, NT>), grid, dim3(TPB), 0, s, img, L, K, V, t, scale, ds);
  return check_launch("k_trim_ptrs");
}

template <int N, bool NT>
int launch_trim_bucket_dense(const uint32_t* x, int64_t ld, int64_t P, const BucketArgs& b, int t, float scale, int ds,
                             uint32_t* y, hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)((P + TPB - 1) / TPB));
  if (b.perm) hipLaunchKernelGGL((k_trim_bucket_dense<N, NT, true>), grid, dim3(TPB), 0, s, x, ld, P, b, t, scale, ds, y);
  else hipLaunchKernelGGL((k_trim_bucket_dense<N, NT, false>), grid, dim3(TPB), 0, s, x, ld, P, b, t, scale, ds, y);
  return check_launch("k_trim_bucket_dense");
}

template <int N, bool NT>
int launch_trim_bucket_ptrs(const int64_t* img, int L, int64_t nblk, int V, const BucketArgs& b, int t, float scale,
                            int ds, hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)nblk, 256 / TPB);
  if (b.perm) hipLaunchKernelGGL((k_trim_bucket_ptrs<N, NT, true>), grid, dim3(TPB), 0, s, img, L, V, b, t, scale, ds);
  else hipLaunchKernelGGL((k_trim_bucket_ptrs<N, NT, false>), grid, dim3(TPB), 0, s, img, L, V, b, t, scale, ds);
  return check_launch("k_trim_bucket_ptrs");
}

// K clients in buckets of s (checked): the counts and the two inverses, formed as the trimmed
// mean's scale is (f32 of the double quotient). s > K is one bucket of K.
BucketArgs bucket_args(const int32_t* perm_dev, int64_t K, int64_t s) {
  if (s > K) s = K;
  const int64_t B = (K + s - 1) / s, n_last = K - (B - 1) * s;
  return BucketArgs{perm_dev, (int)K, (int)s, (int)B, (float)(1.0 / (double)s), (float)(1.0 / (double)n_last)};
}

template <int N, bool NT>
int launch_meamed_dense(const uint32_t* x, int64_t ld, int K, int64_t P, int keep, float scale, int ds, uint32_t* y,
                        const MeamedRows& rows, hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)((P + TPB - 1) / TPB));
  hipLaunchKernelGGL((k_meamed_dense<N, NT>), grid, dim3(TPB), 0, s, x, ld, K, P, keep, scale, ds, y, rows);
  return check_launch("k_meamed_dense");
}

template <int N, bool NT>
int launch_meamed_ptrs(const int64_t* img, int L, int K, int64_t nblk, int V, int keep, float scale, int ds,
                       hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)nblk, 256 / TPB);
  hipLaunchKernelGGL((k_meamed_ptrs<N, NT>), grid, dim3(TPB), 0, s, img, L, K, V, keep, scale, ds);
  return check_launch("k_meamed_ptrs");
}

struct MeamedDevArgs {
  const int32_t *rows, *count, *keep;
  const float* scale;
};

template <int N, bool NT>
int launch_meamed_dense_dev(const uint32_t* x, int64_t ld, int K_rows, int M_max, int64_t P, const MeamedDevArgs& t,
                            int ds, uint32_t* y, hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)((P + TPB - 1) / TPB));
  hipLaunchKernelGGL((k_meamed_dense_dev<N, NT>), grid, dim3(TPB), 0, s, x, ld, K_rows, M_max, P, t.rows, t.count,
                     t.keep, t.scale, ds, y);
  return check_launch("k_meamed_dense_dev");
}

template <int N, bool NT>
int launch_meamed_ptrs_dev(const int64_t* img, int L, int M_max, int64_t nblk, int V, const MeamedDevArgs& t, int ds,
                           hipStream_t s) {
  constexpr int TPB = TrimShape<N>::TPB;
  const dim3 grid((unsigned)nblk, 256 / TPB);
  hipLaunchKernelGGL((k_meamed_ptrs_dev<N, NT>), grid, dim3(TPB), 0, s, img, L, M_max, V, t.count, t.keep, t.scale, ds);
  return check_launch("k_meamed_ptrs_dev");
}

// fjagg_meamed_*'s refusals with M_max in place of M (keep is the device's)
int meamed_dev_check(int in_dtype, int64_t K_rows, int64_t M_max, int flags, int allowed) {
  if (int rc = column_check("mean around median", in_dtype, M_max, flags, allowed)) return rc;
  if (K_rows < 1 || K_rows > kMeamedMaxSlabRows)
    return fail(K_rows < 1 ? FJAGG_EINVAL : FJAGG_EUNSUPPORTED,
                "mean around median: a slab of 1 <= K_rows <= %d rows (got %lld)", kMeamedMaxSlabRows, (long long)K_rows);
  if (M_max > K_rows)
    return fail(FJAGG_EINVAL, "mean around median: M_max <= K_rows (M_max=%lld, K_rows=%lld)", (long long)M_max,
                (long long)K_rows);
  return FJAGG_OK;
}

}  // namespace

#define FJ_TRIM_WIDTH(FN, NTV, ...)                \
  (K <= 16   ? FN<16, NTV>(__VA_ARGS__)                \
   : K <= 32 ? FN<32, NTV>(__VA_ARGS__)                \
   : K <= 64 ? FN<64, NTV>(__VA_ARGS__)                \
             : FN<128, NTV>(__VA_ARGS__))

extern "C" {

int fjagg_trim_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t t, float scale,
                     void* out_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = trim_check(in_dtype, K, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kTrimMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "trimmed mean: rows <= 1 GiB");
  if (!x_dev || !out_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t* x = reinterpret_cast<const uint32_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, tt = (int)t;
  return (flags & FJAGG_NONTEMPORAL) ? FJ_TRIM_WIDTH(launch_trim_dense, true, x, ld, k, P, tt, scale, ds, y, s)
                                     : FJ_TRIM_WIDTH(launch_trim_dense, false, x, ld, k, P, tt, scale, ds, y, s);
}

int fjagg_trim_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t t, float scale,
                    int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = trim_check(in_dtype, K, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, tt = (int)t;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  return (flags & FJAGG_NONTEMPORAL) ? FJ_TRIM_WIDTH(launch_trim_ptrs, true, image_dev, L, k, nblk, V, tt, scale, ds, s)
                                     : FJ_TRIM_WIDTH(launch_trim_ptrs, false, image_dev, L, k, nblk, V, tt, scale, ds, s);
}

int fjagg_trim_bucket_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const int32_t* perm_dev,
                            int64_t s, int64_t t, float scale, void* out_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = bucket_check(in_dtype, K, s, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kTrimMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "bucketed trimmed mean: rows <= 1 GiB");
  if (!x_dev || !out_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const uint32_t* x = reinterpret_cast<const uint32_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const BucketArgs b = bucket_args(perm_dev, K, s);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, tt = (int)t;
  K = b.B;  // the width's bound
  return (flags & FJAGG_NONTEMPORAL) ? FJ_TRIM_WIDTH(launch_trim_bucket_dense, true, x, ld, P, b, tt, scale, ds, y, st)
                                     : FJ_TRIM_WIDTH(launch_trim_bucket_dense, false, x, ld, P, b, tt, scale, ds, y, st);
}

int fjagg_trim_bucket_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk,
                           const int32_t* perm_dev, int64_t s, int64_t t, float scale, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = bucket_check(in_dtype, K, s, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const BucketArgs b = bucket_args(perm_dev, K, s);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, tt = (int)t;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  K = b.B;  // the width's bound
  return (flags & FJAGG_NONTEMPORAL)
             ? FJ_TRIM_WIDTH(launch_trim_bucket_ptrs, true, image_dev, L, nblk, V, b, tt, scale, ds, st)
             : FJ_TRIM_WIDTH(launch_trim_bucket_ptrs, false, image_dev, L, nblk, V, b, tt, scale, ds, st);
}

int fjagg_meamed_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K_rows, int64_t P, const int32_t* rows_host,
                       int64_t M, int64_t keep, float scale, void* out_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = meamed_check(in_dtype, M, keep, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (K_rows < 1 || K_rows > kMeamedMaxSlabRows)
    return fail(K_rows < 1 ? FJAGG_EINVAL : FJAGG_EUNSUPPORTED,
                "mean around median: a slab of 1 <= K_rows <= %d rows (got %lld)", kMeamedMaxSlabRows, (long long)K_rows);
  if (M > K_rows)
    return fail(FJAGG_EINVAL, "mean around median: M <= K_rows (M=%lld, K_rows=%lld)", (long long)M, (long long)K_rows);
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kTrimMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "mean around median: rows <= 1 GiB");
  if (!x_dev || !out_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  MeamedRows rows;
  for (int k = 0; k < kMeamedMaxClients; ++k) {
    // entries past M are never read; they repeat the last row so that every entry is a row of the slab
    const int64_t r = k < M ? (rows_host ? (int64_t)rows_host[k] : (int64_t)k) : (int64_t)rows.r[M - 1];
    if (r < 0 || r >= K_rows || (k > 0 && k < M && r <= rows.r[k - 1]))
      return fail(FJAGG_EINVAL,
                  "mean around median: rows must be strictly ascending in [0, K_rows) (rows[%d]=%lld, K_rows=%lld)", k,
                  (long long)r, (long long)K_rows);
    rows.r[k] = (int32_t)r;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t* x = reinterpret_cast<const uint32_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, K = (int)M, kp = (int)keep;
  return (flags & FJAGG_NONTEMPORAL) ? FJ_TRIM_WIDTH(launch_meamed_dense, true, x, ld, K, P, kp, scale, ds, y, rows, s)
                                     : FJ_TRIM_WIDTH(launch_meamed_dense, false, x, ld, K, P, kp, scale, ds, y, rows, s);
}

int fjagg_meamed_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t keep, float scale,
                      int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = meamed_check(in_dtype, K, keep, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, kp = (int)keep;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  return (flags & FJAGG_NONTEMPORAL)
             ? FJ_TRIM_WIDTH(launch_meamed_ptrs, true, image_dev, L, k, nblk, V, kp, scale, ds, s)
             : FJ_TRIM_WIDTH(launch_meamed_ptrs, false, image_dev, L, k, nblk, V, kp, scale, ds, s);
}

int fjagg_meamed_dense_dev(int in_dtype, const void* x_dev, int64_t ld, int64_t K_rows, int64_t P, int64_t M_max,
                           const int32_t* rows_dev, const int32_t* count_dev, const int32_t* keep_dev,
                           const float* scale_dev, void* out_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = meamed_dev_check(in_dtype, K_rows, M_max, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kTrimMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "mean around median: rows <= 1 GiB");
  if (!x_dev || !out_dev || !rows_dev || !count_dev || !keep_dev || !scale_dev)
    return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t* x = reinterpret_cast<const uint32_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const MeamedDevArgs t{rows_dev, count_dev, keep_dev, scale_dev};
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, K = (int)M_max, kr = (int)K_rows;  // K: the width's bound
  return (flags & FJAGG_NONTEMPORAL) ? FJ_TRIM_WIDTH(launch_meamed_dense_dev, true, x, ld, kr, K, P, t, ds, y, s)
                                     : FJ_TRIM_WIDTH(launch_meamed_dense_dev, false, x, ld, kr, K, P, t, ds, y, s);
}

int fjagg_meamed_ptrs_dev(int in_dtype, const int64_t* image_all_dev, int64_t* image_group_dev, int L, int64_t K_rows,
                          int64_t M_max, int64_t nblk, const int32_t* rows_dev, const int32_t* count_dev,
                          const int32_t* keep_dev, const float* scale_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = meamed_dev_check(in_dtype, K_rows, M_max, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED))
    return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_all_dev || !image_group_dev || !rows_dev || !count_dev || !keep_dev || !scale_dev)
    return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int64_t blocks = (M_max * L + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)blocks), dim3(256), 0, s, image_all_dev, L, (int)K_rows, rows_dev,
                     (int)M_max, image_group_dev);
  if (int rc = check_launch("k_gather_rows")) return rc;
  const MeamedDevArgs t{rows_dev, count_dev, keep_dev, scale_dev};
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, K = (int)M_max;  // K: the width's bound
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  const int64_t* img = image_group_dev;
  return (flags & FJAGG_NONTEMPORAL) ? FJ_TRIM_WIDTH(launch_meamed_ptrs_dev, true, img, L, K, nblk, V, t, ds, s)
                                     : FJ_TRIM_WIDTH(launch_meamed_ptrs_dev, false, img, L, K, nblk, V, t, ds, s);
}

}  // extern "C"
