// fjtrimsel16.hip — coordinate-wise trimmed mean and median of BFLOAT16 deltas for up to 1024
// clients, by rank selection over 16-bit keys (include/fjagg.h: fjagg_trim_select16_dense,
// fjagg_trim_select16_ptrs). The rule and its bits are fjtrimsel.hip's on the values
// upcast to float32 (bits << 16, exact); the sum and the output are float32. What differs is the
// key: bfloat16's total order lives in 16 bits (fjtrimsel::key16_of), so the descent is 16 steps
// and a key takes two bytes of LDS. A workgroup of kWaves = 8 waves owns a tile of kCols = 64
// consecutive columns of all K clients, as 16-bit keys in LDS in client order, in three phases:
//
//   load     wave w, lane c (the column) streams the rows 128 i + 16 w + j, j = 0 .. 15, with
//            2-byte loads: a wave reads one 128-byte segment of a row, bfloat16's own alignment is
//            all a row needs, and the 16 loads are in flight before the first key is written.
//   select   a WAVE takes a column (wave w the columns w, w + 8, ..): lane l holds the keys of the
//            clients l, l + 64, .. zero-extended in NI = 2 / 4 / 8 / 16 registers, and a question
//            of the descent is one compare and one ballot a register, masked by "client index
//            < K": 0xFFFF, the +NaN 0x7FFF, is a key like any other. The same ballots compact
//            the kept keys into the column's slots 0 .. K-2t-1, in client order.
//   sum      lane q < 8 of wave w adds the K - 2t compacted values of column w + 8 q, turning
//            each key back into float32 bits as it reads: fjtrimsel::chain_sum's dependent chain.
//
// The tile's pitch is 65 halfwords: 64 NI rows of 130 bytes, 16.25 / 32.5 / 65 / 130 KiB, twice the
// columns of fjtrimsel.hip's tile in the same LDS. At 1024 clients one workgroup fits a CU either
// way; its 8 waves put two on every SIMD, so one wave's compares issue under the other's ballot
// sums. A wave's register fill reads 64 consecutive rows of one column: halfword 65 r + c is word
// 65 m + (c >> 1) for r = 2 m and 65 m + 32 + ((c + 1) >> 1) for r = 2 m + 1, m = 0 .. 31: all 64
// banks once. Slots past K are never written and never counted.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjagg.h"
#include "fjtrimsel_dev.h"

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
constexpr int kCols = 64;    // columns of a tile: a wave's lanes
constexpr int kPitch = 65;   // halfwords between two clients' rows of the tile
constexpr int kWaves = 8;    // waves of a workgroup
constexpr int kTPB = 64 * kWaves;
constexpr int kWalk = 4;     // workgroups that share a plan entry, kCols columns each a turn

// 2 bytes through a GLOBAL (address space 1) pointer
typedef __attribute__((address_space(1))) uint16_t gu16;
typedef __attribute__((address_space(1))) uint32_t gu32;
template <bool NT>
__device__ __forceinline__ uint32_t load_bits(const uint16_t* p, uint32_t lane_off) {
  const gu16* g = (const gu16*)(reinterpret_cast<uintptr_t>(p)) + lane_off;
  if constexpr (NT) return __builtin_nontemporal_load(g);
  else return *g;
}
__device__ __forceinline__ void store_bits(uint32_t* p, uint32_t v) { *(gu32*)(reinterpret_cast<uintptr_t>(p)) = v; }

__device__ __forceinline__ int popc64(uint64_t m) { return __builtin_popcountll(m); }
// the number of set bits of m below this lane
__device__ __forceinline__ int rank_in(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One tile: columns [0, ncols) of the K rows that row(k) names (a pointer to client k's value of
// the tile's first column, 0 <= k < K), results to out[0 .. ncols). 1 <= ncols <= kCols,
// 1 <= K <= 64 NI, 0 <= 2t < K. Every lane of the workgroup calls it; it ends with the tile free.
template <int NI, bool NT, class Row>
__device__ __forceinline__ void select_tile(uint16_t* tile, Row row, int K, int t, int ncols, bool do_scale,
                                            float scale, uint32_t* out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // ---- load: lanes past ncols redo the last column, rows past K the last row; neither is written
  const uint32_t cc = lane < ncols ? lane : ncols - 1;
#pragma unroll 1
  for (int k0 = 16 * w; k0 < K; k0 += 16 * kWaves) {  // k0 differs by wave: no barrier inside
    uint32_t v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = load_bits<NT>(row(k0 + j < K ? k0 + j : K - 1), cc);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (k0 + j < K && lane < ncols) tile[(k0 + j) * kPitch + lane] = (uint16_t)fjtrimsel::key16_of(v[j]);
  }
  __syncthreads();
  // ---- select and compact: a wave a column
#pragma unroll 1
  for (int col = w; col < ncols; col += kWaves) {
    uint16_t* colp = tile + col;
    uint32_t r[NI];
    uint64_t in[NI];  // the lanes of register i that hold a client: a compare's ballot is masked by it
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int k = 64 * i + lane;
      in[i] = __builtin_amdgcn_ballot_w64(k < K);
      r[i] = colp[(k < K ? k : K - 1) * kPitch];
    }
    auto count2 = [&](uint32_t a, uint32_t b, int& na, int& nb2) {
      na = 0;
      nb2 = 0;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        na += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] < a));
        nb2 += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] < b));
      }
    };
    auto count_eq = [&](uint32_t u) {
      int n = 0;
#pragma unroll
      for (int i = 0; i < NI; ++i) n += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] == u));
      return n;
    };
    const fjtrimsel::Cuts cuts = fjtrimsel::select_cuts<16>(count2, count_eq, K, t);
    // client order is register-major, lane-minor: the running indices are ballot prefixes
    int baseL = 0, baseU = 0, baseKept = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const uint64_t mL = in[i] & __builtin_amdgcn_ballot_w64(r[i] == cuts.L);
      const uint64_t mU = in[i] & __builtin_amdgcn_ballot_w64(r[i] == cuts.U);
      const bool keep = 64 * i + lane < K && fjtrimsel::kept(r[i], cuts, baseL + rank_in(mL), baseU + rank_in(mU));
      const uint64_t mK = __builtin_amdgcn_ballot_w64(keep);
      // slot <= the client's own index, and the wave holds every key of the column already
      if (keep) colp[(baseKept + rank_in(mK)) * kPitch] = (uint16_t)r[i];
      baseL += popc64(mL);
      baseU += popc64(mU);
      baseKept += popc64(mK);
    }
  }
  __syncthreads();
  // ---- sum: K - 2t values a column, kCols / kWaves lanes a wave
  const int mycol = w + kWaves * lane;
  if (lane < kCols / kWaves && mycol < ncols) {
    const uint16_t* colp = tile + mycol;
    const uint32_t y = fjtrimsel::chain_sum([=](int j) { return fjtrimsel::float_bits_of_key16(colp[j * kPitch]); },
                                            K - 2 * t, do_scale, scale);
    store_bits(out + mycol, y);
  }
  __syncthreads();
}

template <int NI>
__device__ __forceinline__ uint16_t* the_tile() {
  __shared__ uint16_t tile[NI * 64 * kPitch];
  return tile;
}

// Dense slab: client k's row at x + k*ld, columns [0, P); workgroup b has the columns 64 b ..
template <int NI, bool NT>
__global__ __launch_bounds__(kTPB) void k_trim_select16_dense(const uint16_t* __restrict__ x, int64_t ld, int K,
                                                               int64_t P, int t, float scale, int do_scale,
                                                               uint32_t* __restrict__ out) {
  const int64_t col0 = (int64_t)blockIdx.x * kCols;
  const int ncols = P - col0 < kCols ? (int)(P - col0) : kCols;
  const uint16_t* base = x + col0;
  select_tile<NI, NT>(the_tile<NI>(), [=](int k) { return base + (int64_t)k * ld; }, K, t, ncols, do_scale != 0, scale,
                      out + col0);
}

// Pytree path over the plan image of fjagg_ptrs_plan_leaves for bfloat16 leaves (unit V = 8
// elements, 1 with FJAGG_UNALIGNED), decoded as fjtrimsel.hip's k_trim_select_ptrs decodes its
// own: plan entry blockIdx.x names an element range of one leaf, and the kWalk workgroups
// blockIdx.y of that entry walk it 256 columns at a time, 64 each. Output leaves are float32.
template <int NI, bool NT>
__global__ __launch_bounds__(kTPB) void k_trim_select16_ptrs(const int64_t* __restrict__ img, int L, int K, int V,
                                                              int t, float scale, int do_scale) {
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
  uint16_t* tile = the_tile<NI>();
  for (int64_t g = e0 + (int64_t)blockIdx.y * kCols; g < e1; g += kWalk * kCols) {  // uniform over the workgroup
    const int ncols = e1 - g < kCols ? (int)(e1 - g) : kCols;
    auto row = [=](int k) { return reinterpret_cast<const uint16_t*>(in_ptrs[(int64_t)k * L + leaf]) + g; };
    select_tile<NI, NT>(tile, row, K, t, ncols, do_scale != 0, scale, ob + g);
  }
}

// fjtrimsel.hip's select_check with bfloat16 in place of float32
int select_check(int in_dtype, int64_t K, int64_t t, int flags, int allowed) {
  const char* who = "trimmed mean by 16-bit selection";
  if (in_dtype != FJAGG_BF16) return fail(FJAGG_EUNSUPPORTED, "%s: bfloat16 deltas and float32 output only", who);
  if (flags & FJAGG_ACCUMULATE)
    return fail(FJAGG_EUNSUPPORTED, "%s: order statistics do not accumulate (no FJAGG_ACCUMULATE)", who);
  if (flags & FJAGG_NARROW) return fail(FJAGG_EUNSUPPORTED, "%s: no FJAGG_NARROW plans", who);
  if (flags & FJAGG_HOST_TABLES) return fail(FJAGG_EUNSUPPORTED, "%s: device plan only (no FJAGG_HOST_TABLES)", who);
  if (flags & FJAGG_ZEROED_WS) return fail(FJAGG_EUNSUPPORTED, "%s: no norms (no FJAGG_ZEROED_WS)", who);
  if (flags & FJAGG_UNBALANCED) return fail(FJAGG_EUNSUPPORTED, "%s: no FJAGG_UNBALANCED", who);
  if (flags & ~allowed) return fail(FJAGG_EUNSUPPORTED, "%s: unsupported flags 0x%x", who, flags & ~allowed);
  if (K < 1) return fail(FJAGG_EINVAL, "K must be >= 1 (got %lld)", (long long)K);
  if (K > fjtrimsel::kMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "%s: K <= %d clients (got %lld)", who, fjtrimsel::kMaxClients, (long long)K);
  if (t < 0 || 2 * t >= K)
    return fail(FJAGG_EINVAL, "%s: need 0 <= 2t < K (t=%lld, K=%lld)", who, (long long)t, (long long)K);
  return FJAGG_OK;
}

template <int NI, bool NT>
int launch_dense(const uint16_t* x, int64_t ld, int K, int64_t P, int t, float scale, int ds, uint32_t* y,
                 hipStream_t s) {
  const dim3 grid((unsigned)((P + kCols - 1) / kCols));
  hipLaunchKernelGGL((k_trim_select16_dense<NI, NT>), grid, dim3(kTPB), 0, s, x, ld, K, P, t, scale, ds, y);
  return check_launch("k_trim_select16_dense");
}

template <int NI, bool NT>
int launch_ptrs(const int64_t* img, int L, int K, int64_t nblk, int V, int t, float scale, int ds, hipStream_t s) {
  const dim3 grid((unsigned)nblk, kWalk);
  hipLaunchKernelGGL((k_trim_select16_ptrs<NI, NT>), grid, dim3(kTPB), 0, s, img, L, K, V, t, scale, ds);
  return check_launch("k_trim_select16_ptrs");
}

}  // namespace

// registers a lane: the tile is 64 NI rows of 130 bytes, 16.25 / 32.5 / 65 / 130 KiB
#define FJ_SELECT_WIDTH(FN, NTV, ...)          \
  (K <= 128   ? FN<2, NTV>(__VA_ARGS__)        \
   : K <= 256 ? FN<4, NTV>(__VA_ARGS__)        \
   : K <= 512 ? FN<8, NTV>(__VA_ARGS__)        \
              : FN<16, NTV>(__VA_ARGS__))

extern "C" {

int fjagg_trim_select16_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t t,
                              float scale, void* out_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = select_check(in_dtype, K, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 2 > kMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "trimmed mean by 16-bit selection: rows <= 1 GiB");
  if (!x_dev || !out_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint16_t* x = reinterpret_cast<const uint16_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, tt = (int)t;
  return (flags & FJAGG_NONTEMPORAL) ? FJ_SELECT_WIDTH(launch_dense, true, x, ld, k, P, tt, scale, ds, y, s)
                                     : FJ_SELECT_WIDTH(launch_dense, false, x, ld, k, P, tt, scale, ds, y, s);
}

int fjagg_trim_select16_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t t,
                             float scale, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = select_check(in_dtype, K, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, tt = (int)t;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 8;  // the plan's unit for bfloat16 (fjagg_ptrs_plan_leaves)
  return (flags & FJAGG_NONTEMPORAL) ? FJ_SELECT_WIDTH(launch_ptrs, true, image_dev, L, k, nblk, V, tt, scale, ds, s)
                                     : FJ_SELECT_WIDTH(launch_ptrs, false, image_dev, L, k, nblk, V, tt, scale, ds, s);
}

}  // extern "C"
