// fjtrimsel.hip — coordinate-wise trimmed mean and median for up to 1024 clients by rank
// selection in an LDS tile (include/fjagg.h: fjagg_trim_select_dense, fjagg_trim_select_ptrs;
// DESIGN 3v). The arithmetic is fjagg_trim_*'s (fjrobust.hip), word for word; what differs is
// who holds a column. There a lane owns a column and sorts it, which stops at 128 clients. Here
// a 256-lane workgroup owns a tile of kCols = 32 consecutive columns of all K clients, as uint32
// keys in LDS in client order, and works on it in three phases:
//
//   load     lane (wave w, half h, column c) streams the rows 64 i + 32 h + 8 w + j, j = 0 .. 7,
//            with 4-byte loads: a half-wave reads one 128-byte segment of a row, and the 16 loads
//            of two blocks of 64 rows are in flight before the first key is written.
//   select   a WAVE takes a column (wave w the columns w, w + 4, ..): lane l holds the keys of
//            the clients l, l + 64, .. in NI = 2 / 4 / 8 / 16 registers, and a question of the
//            descent (fjtrimsel_dev.h), "how many keys are below v", is one compare and one
//            ballot a register, summed on the scalar unit. L, U and the cuts are then uniform
//            over the wave. The same ballots give every client its running index among the
//            L- and U-valued and among the kept, and the kept values go back into the column's
//            slots 0 .. K-2t-1 as float bits, still in client order.
//   sum      lane q < 8 of wave w adds the K - 2t compacted values of column w + 4 q: the
//            dependent chain the contract prescribes, one add a value.
//
// The tile's pitch is 33 words. A wave's register fill reads 64 consecutive rows of one column,
// 33 l mod 64: 64 banks. The load phase writes rows r (h = 0) and r + 32 (h = 1), 32 columns
// each: 33 * 32 = 32 mod 64, two disjoint runs of 32 banks. The chain's 8 lanes read 8 banks.
// Slots past K are never written and never counted: the register fill reads client K-1 again
// there and every ballot carries "client index < K".
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
constexpr int kCols = 32;    // columns of a tile
constexpr int kPitch = 33;   // words between two clients' rows of the tile
constexpr int kTPB = 256;

// 4 bytes through a GLOBAL (address space 1) pointer, as fjrobust.hip's
typedef __attribute__((address_space(1))) uint32_t gu32;
template <bool NT>
__device__ __forceinline__ uint32_t load_bits(const uint32_t* p, uint32_t lane_off) {
  const gu32* g = (const gu32*)(reinterpret_cast<uintptr_t>(p)) + lane_off;
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
__device__ __forceinline__ void select_tile(uint32_t* tile, Row row, int K, int t, int ncols, bool do_scale,
                                            float scale, uint32_t* out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  // ---- load: lanes past ncols redo the last column, rows past K the last row; neither is written
  const uint32_t cc = c < ncols ? c : ncols - 1;
  const int nb = (K + 63) >> 6;
#pragma unroll 1
  for (int i0 = 0; i0 < nb; i0 += 2) {
    uint32_t v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = 64 * (i0 + (j >> 3)) + 32 * h + 8 * w + (j & 7);
      v[j] = load_bits<NT>(row(k < K ? k : K - 1), cc);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = 64 * (i0 + (j >> 3)) + 32 * h + 8 * w + (j & 7);
      if (k < K && c < ncols) tile[k * kPitch + c] = fjrobust::key_of(v[j]);
    }
  }
  __syncthreads();
  // ---- select and compact: a wave a column
#pragma unroll 1
  for (int col = w; col < ncols; col += 4) {
    uint32_t* colp = tile + col;
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
    const fjtrimsel::Cuts cuts = fjtrimsel::select_cuts(count2, count_eq, K, t);
    // client order is register-major, lane-minor: the running indices are ballot prefixes
    int baseL = 0, baseU = 0, baseKept = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const uint64_t mL = in[i] & __builtin_amdgcn_ballot_w64(r[i] == cuts.L);
      const uint64_t mU = in[i] & __builtin_amdgcn_ballot_w64(r[i] == cuts.U);
      const bool keep = 64 * i + lane < K && fjtrimsel::kept(r[i], cuts, baseL + rank_in(mL), baseU + rank_in(mU));
      const uint64_t mK = __builtin_amdgcn_ballot_w64(keep);
      // slot <= the client's own index, and the wave holds every key of the column already
      if (keep) colp[(baseKept + rank_in(mK)) * kPitch] = fjrobust::bits_of(r[i]);
      baseL += popc64(mL);
      baseU += popc64(mU);
      baseKept += popc64(mK);
    }
  }
  __syncthreads();
  // ---- sum: K - 2t values a column, 8 lanes a wave
  const int mycol = w + 4 * lane;
  if (lane < 8 && mycol < ncols) {
    const uint32_t* colp = tile + mycol;
    const uint32_t y = fjtrimsel::chain_sum([=](int j) { return colp[j * kPitch]; }, K - 2 * t, do_scale, scale);
    store_bits(out + mycol, y);
  }
  __syncthreads();
}

template <int NI>
__device__ __forceinline__ uint32_t* the_tile() {
  __shared__ uint32_t tile[NI * 64 * kPitch];
  return tile;
}

// Dense slab: client k's row at x + k*ld, columns [0, P); workgroup b has the columns 32 b ..
template <int NI, bool NT>
__global__ __launch_bounds__(kTPB) void k_trim_select_dense(const uint32_t* __restrict__ x, int64_t ld, int K, int64_t P,
                                                             int t, float scale, int do_scale,
                                                             uint32_t* __restrict__ out) {
  const int64_t col0 = (int64_t)blockIdx.x * kCols;
  const int ncols = P - col0 < kCols ? (int)(P - col0) : kCols;
  const uint32_t* base = x + col0;
  select_tile<NI, NT>(the_tile<NI>(), [=](int k) { return base + (int64_t)k * ld; }, K, t, ncols, do_scale != 0, scale,
                      out + col0);
}

// Pytree path over the plan image fjagg_trim_ptrs takes, decoded as fjrobust.hip's ptrs_walk
// decodes it: plan entry blockIdx.x names an element range of one leaf, and the 8 workgroups
// blockIdx.y of that entry walk it 256 columns at a time, 32 each.
template <int NI, bool NT>
__global__ __launch_bounds__(kTPB) void k_trim_select_ptrs(const int64_t* __restrict__ img, int L, int K, int V, int t,
                                                            float scale, int do_scale) {
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
  uint32_t* tile = the_tile<NI>();
  for (int64_t g = e0 + (int64_t)blockIdx.y * kCols; g < e1; g += 256) {  // uniform over the workgroup
    const int ncols = e1 - g < kCols ? (int)(e1 - g) : kCols;
    auto row = [=](int k) { return reinterpret_cast<const uint32_t*>(in_ptrs[(int64_t)k * L + leaf]) + g; };
    select_tile<NI, NT>(tile, row, K, t, ncols, do_scale != 0, scale, ob + g);
  }
}

int select_check(int in_dtype, int64_t K, int64_t t, int flags, int allowed) {
  const char* who = "trimmed mean by selection";
  if (in_dtype != FJAGG_F32) return fail(FJAGG_EUNSUPPORTED, "%s: float32 deltas and output only", who);
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
int launch_dense(const uint32_t* x, int64_t ld, int K, int64_t P, int t, float scale, int ds, uint32_t* y,
                 hipStream_t s) {
  const dim3 grid((unsigned)((P + kCols - 1) / kCols));
  hipLaunchKernelGGL((k_trim_select_dense<NI, NT>), grid, dim3(kTPB), 0, s, x, ld, K, P, t, scale, ds, y);
  return check_launch("k_trim_select_dense");
}

template <int NI, bool NT>
int launch_ptrs(const int64_t* img, int L, int K, int64_t nblk, int V, int t, float scale, int ds, hipStream_t s) {
  const dim3 grid((unsigned)nblk, 256 / kCols);
  hipLaunchKernelGGL((k_trim_select_ptrs<NI, NT>), grid, dim3(kTPB), 0, s, img, L, K, V, t, scale, ds);
  return check_launch("k_trim_select_ptrs");
}

}  // namespace

// registers a lane: the tile is 64 NI rows of 132 bytes, 16.5 / 33 / 66 / 132 KiB
#define FJ_SELECT_WIDTH(FN, NTV, ...)          \
  (K <= 128   ? FN<2, NTV>(__VA_ARGS__)        \
   : K <= 256 ? FN<4, NTV>(__VA_ARGS__)        \
   : K <= 512 ? FN<8, NTV>(__VA_ARGS__)        \
              : FN<16, NTV>(__VA_ARGS__))

extern "C" {

int fjagg_trim_select_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t t, float scale,
                            void* out_dev, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = select_check(in_dtype, K, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "trimmed mean by selection: rows <= 1 GiB");
  if (!x_dev || !out_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t* x = reinterpret_cast<const uint32_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, tt = (int)t;
  return (flags & FJAGG_NONTEMPORAL) ? FJ_SELECT_WIDTH(launch_dense, true, x, ld, k, P, tt, scale, ds, y, s)
                                     : FJ_SELECT_WIDTH(launch_dense, false, x, ld, k, P, tt, scale, ds, y, s);
}

int fjagg_trim_select_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t t,
                           float scale, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = select_check(in_dtype, K, t, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, tt = (int)t;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  return (flags & FJAGG_NONTEMPORAL) ? FJ_SELECT_WIDTH(launch_ptrs, true, image_dev, L, k, nblk, V, tt, scale, ds, s)
                                     : FJ_SELECT_WIDTH(launch_ptrs, false, image_dev, L, k, nblk, V, tt, scale, ds, s);
}

}  // extern "C"
