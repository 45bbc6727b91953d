// fjmeamedsel.hip — the mean around the median for up to 1024 participating clients by rank
// selection in an LDS tile (include/fjagg.h: fjagg_meamed_select_dense, fjagg_meamed_select_ptrs;
// DESIGN 3w). The arithmetic is fjagg_meamed_*'s (fjrobust.hip), word for word; the column rule is
// fjmeamedsel_dev.h's. The tile is fjtrimsel.hip's: a 256-lane workgroup owns kCols = 32 consecutive
// columns of all K participating clients, as uint32 keys in LDS in client order at a pitch of 33
// words, and works on it in three phases:
//
//   load     lane (wave w, half h, column c) streams the rows 64 i + 32 h + 8 w + j, j = 0 .. 7,
//            with 4-byte loads, 16 of them in flight before the first key is written. With a row
//            table the 16 table entries are read first, clamped into the slab, and then the rows.
//   select   a WAVE takes a column: lane l holds the keys of the clients l, l + 64, .. in NI =
//            2 / 4 / 8 / 16 registers. The median's descent runs over ballots of them. Then every
//            lane turns its NI keys into NI sided distances, in registers: the 1024-client tile
//            is 132 KiB, there is no room for a second one, and a distance is one subtract. The
//            descent for D* runs over ballots of those, the two-rank descent for L and U over the
//            keys again. med, D*, the window's start and the cuts are uniform over the wave. The
//            kept values are compacted into the column's slots 0 .. beta-1 in client order.
//   sum      lane q < 8 of wave w adds the beta compacted values of column w + 4 q.
//
// Slots past K are never written and never counted: the register fill reads client K-1 again
// there and every ballot is masked by "client index < K".
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjagg.h"
#include "fjmeamedsel_dev.h"

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
constexpr int kCols = 32;   // columns of a tile
constexpr int kPitch = 33;  // words between two clients' rows of the tile
constexpr int kTPB = 256;

// 4 bytes through a GLOBAL (address space 1) pointer, as fjtrimsel.hip's
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

// A column in a wave's registers, as fjmeamedsel_dev.h asks for it: register i of lane l is client
// 64 i + l. Every count is a compare and a ballot a register, summed on the scalar unit.
template <int NI>
struct WaveColumn {
  uint32_t key[NI];
  uint32_t sided[NI];
  uint64_t in[NI];  // the lanes of register i that hold a client: every ballot is masked by it

  __device__ __forceinline__ void fill(const uint32_t* colp, int K, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int k = 64 * i + lane;
      in[i] = __builtin_amdgcn_ballot_w64(k < K);
      key[i] = colp[(k < K ? k : K - 1) * kPitch];
      sided[i] = fjmeamedsel::kNoSide;
    }
  }
  __device__ __forceinline__ static int below(const uint32_t (&r)[NI], const uint64_t (&in)[NI], uint32_t v) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) n += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] < v));
    return n;
  }
  __device__ __forceinline__ static int equal(const uint32_t (&r)[NI], const uint64_t (&in)[NI], uint32_t v) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) n += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] == v));
    return n;
  }
  __device__ __forceinline__ static void below2(const uint32_t (&r)[NI], const uint64_t (&in)[NI], uint32_t a,
                                                uint32_t b, int& na, int& nb) {
    na = 0;
    nb = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      na += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] < a));
      nb += popc64(in[i] & __builtin_amdgcn_ballot_w64(r[i] < b));
    }
  }
  __device__ __forceinline__ int keys_below(uint32_t v) const { return below(key, in, v); }
  __device__ __forceinline__ void keys_below2(uint32_t a, uint32_t b, int& na, int& nb) const {
    below2(key, in, a, b, na, nb);
  }
  __device__ __forceinline__ int keys_equal(uint32_t v) const { return equal(key, in, v); }
  __device__ __forceinline__ void place(uint32_t med_key) {
    const float med = fjrobust::as_float(fjrobust::bits_of(med_key));
#pragma unroll
    for (int i = 0; i < NI; ++i) sided[i] = fjmeamedsel::sided_distance(key[i], med_key, med);
  }
  __device__ __forceinline__ void sided_below2(uint32_t a, uint32_t b, int& na, int& nb) const {
    below2(sided, in, a, b, na, nb);
  }
  __device__ __forceinline__ int sided_equal(uint32_t v) const { return equal(sided, in, v); }
};

// One tile: columns [0, ncols) of the K rows that row(k) names (a pointer to participating client
// k's value of the tile's first column, 0 <= k < K), results to out[0 .. ncols). 1 <= ncols <= kCols,
// 1 <= K <= 64 NI, 1 <= beta <= K. Every lane of the workgroup calls it; it ends with the tile free.
template <int NI, bool NT, class Row>
__device__ __forceinline__ void meamed_tile(uint32_t* tile, Row row, int K, int beta, int ncols, bool do_scale,
                                            float scale, uint32_t* out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  // ---- load: lanes past ncols redo the last column, rows past K the last row; neither is written
  const uint32_t cc = c < ncols ? c : ncols - 1;
  const int nb = (K + 63) >> 6;
#pragma unroll 1
  for (int i0 = 0; i0 < nb; i0 += 2) {
    const uint32_t* p[16];
    uint32_t v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = 64 * (i0 + (j >> 3)) + 32 * h + 8 * w + (j & 7);
      p[j] = row(k < K ? k : K - 1);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = load_bits<NT>(p[j], cc);
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
    WaveColumn<NI> wc;
    wc.fill(colp, K, lane);
    int a;
    const fjtrimsel::Cuts cuts = fjmeamedsel::window_cuts(wc, K, beta, &a);
    // client order is register-major, lane-minor: the running indices are ballot prefixes
    int baseL = 0, baseU = 0, baseKept = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const uint64_t mL = wc.in[i] & __builtin_amdgcn_ballot_w64(wc.key[i] == cuts.L);
      const uint64_t mU = wc.in[i] & __builtin_amdgcn_ballot_w64(wc.key[i] == cuts.U);
      const bool keep =
          64 * i + lane < K && fjtrimsel::kept(wc.key[i], cuts, baseL + rank_in(mL), baseU + rank_in(mU));
      const uint64_t mK = __builtin_amdgcn_ballot_w64(keep);
      // slot <= the client's own index, and the wave holds every key of the column already
      if (keep) colp[(baseKept + rank_in(mK)) * kPitch] = fjrobust::bits_of(wc.key[i]);
      baseL += popc64(mL);
      baseU += popc64(mU);
      baseKept += popc64(mK);
    }
  }
  __syncthreads();
  // ---- sum: beta values a column, 8 lanes a wave
  const int mycol = w + 4 * lane;
  if (lane < 8 && mycol < ncols) {
    const uint32_t* colp = tile + mycol;
    const uint32_t y = fjtrimsel::chain_sum([=](int j) { return colp[j * kPitch]; }, beta, do_scale, scale);
    store_bits(out + mycol, y);
  }
  __syncthreads();
}

template <int NI>
__device__ __forceinline__ uint32_t* the_tile() {
  __shared__ uint32_t tile[NI * 64 * kPitch];
  return tile;
}

// Dense slab: participating client k is slab row k or, with TABLE, row rows[k] clamped into
// [0, K_rows): a stale table can give a wrong result but never an address outside the slab.
// Workgroup b has the columns 32 b ..
template <int NI, bool NT, bool TABLE>
__global__ __launch_bounds__(kTPB) void k_meamed_select_dense(const uint32_t* __restrict__ x, int64_t ld, int K_rows,
                                                               const int32_t* __restrict__ rows, int K, int64_t P,
                                                               int beta, float scale, int do_scale,
                                                               uint32_t* __restrict__ out) {
  const int64_t col0 = (int64_t)blockIdx.x * kCols;
  const int ncols = P - col0 < kCols ? (int)(P - col0) : kCols;
  const uint32_t* base = x + col0;
  auto row = [=](int k) {
    int r = k;
    if constexpr (TABLE) r = fjrobust::clamp_index(rows[k], K_rows);
    return base + (int64_t)r * ld;
  };
  meamed_tile<NI, NT>(the_tile<NI>(), row, K, beta, ncols, do_scale != 0, scale, out + col0);
}

// Pytree path over the plan image fjagg_meamed_ptrs takes, decoded as k_trim_select_ptrs decodes
// it: plan entry blockIdx.x names an element range of one leaf, and the 8 workgroups blockIdx.y
// of that entry walk it 256 columns at a time, 32 each.
template <int NI, bool NT>
__global__ __launch_bounds__(kTPB) void k_meamed_select_ptrs(const int64_t* __restrict__ img, int L, int K, int V,
                                                              int beta, float scale, int do_scale) {
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
    meamed_tile<NI, NT>(tile, row, K, beta, ncols, do_scale != 0, scale, ob + g);
  }
}

// fjtrimsel.hip's select_check with the keep count in place of the trim count
int select_check(int in_dtype, int64_t M, int64_t keep, int flags, int allowed) {
  const char* who = "mean around median by selection";
  if (in_dtype != FJAGG_F32) return fail(FJAGG_EUNSUPPORTED, "%s: float32 deltas and output only", who);
  if (flags & FJAGG_ACCUMULATE)
    return fail(FJAGG_EUNSUPPORTED, "%s: order statistics do not accumulate (no FJAGG_ACCUMULATE)", who);
  if (flags & FJAGG_NARROW) return fail(FJAGG_EUNSUPPORTED, "%s: no FJAGG_NARROW plans", who);
  if (flags & FJAGG_HOST_TABLES) return fail(FJAGG_EUNSUPPORTED, "%s: device plan only (no FJAGG_HOST_TABLES)", who);
  if (flags & FJAGG_ZEROED_WS) return fail(FJAGG_EUNSUPPORTED, "%s: no norms (no FJAGG_ZEROED_WS)", who);
  if (flags & FJAGG_UNBALANCED) return fail(FJAGG_EUNSUPPORTED, "%s: no FJAGG_UNBALANCED", who);
  if (flags & ~allowed) return fail(FJAGG_EUNSUPPORTED, "%s: unsupported flags 0x%x", who, flags & ~allowed);
  if (M < 1) return fail(FJAGG_EINVAL, "M must be >= 1 (got %lld)", (long long)M);
  if (M > fjmeamedsel::kMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "%s: M <= %d participating clients (got %lld)", who, fjmeamedsel::kMaxClients,
                (long long)M);
  if (keep < 1 || keep > M)
    return fail(FJAGG_EINVAL, "%s: need 1 <= keep <= M (keep=%lld, M=%lld)", who, (long long)keep, (long long)M);
  return FJAGG_OK;
}

template <int NI, bool NT>
int launch_dense(const uint32_t* x, int64_t ld, int K_rows, const int32_t* rows, int K, int64_t P, int beta,
                 float scale, int ds, uint32_t* y, hipStream_t s) {
  const dim3 grid((unsigned)((P + kCols - 1) / kCols));
  if (rows)
    hipLaunchKernelGGL((k_meamed_select_dense<NI, NT, true>), grid, dim3(kTPB), 0, s, x, ld, K_rows, rows, K, P, beta,
                       scale, ds, y);
  else
    hipLaunchKernelGGL((k_meamed_select_dense<NI, NT, false>), grid, dim3(kTPB), 0, s, x, ld, K_rows, rows, K, P, beta,
                       scale, ds, y);
  return check_launch("k_meamed_select_dense");
}

template <int NI, bool NT>
int launch_ptrs(const int64_t* img, int L, int K, int64_t nblk, int V, int beta, float scale, int ds, hipStream_t s) {
  const dim3 grid((unsigned)nblk, 256 / kCols);
  hipLaunchKernelGGL((k_meamed_select_ptrs<NI, NT>), grid, dim3(kTPB), 0, s, img, L, K, V, beta, scale, ds);
  return check_launch("k_meamed_select_ptrs");
}

}  // namespace

// registers a lane: the tile is 64 NI rows of 132 bytes, 16.5 / 33 / 66 / 132 KiB
#define FJ_SELECT_WIDTH(FN, NTV, ...)          \
  (K <= 128   ? FN<2, NTV>(__VA_ARGS__)        \
   : K <= 256 ? FN<4, NTV>(__VA_ARGS__)        \
   : K <= 512 ? FN<8, NTV>(__VA_ARGS__)        \
              : FN<16, NTV>(__VA_ARGS__))

extern "C" {

int fjagg_meamed_select_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K_rows, int64_t P,
                              const int32_t* rows_dev, int64_t M, int64_t keep, float scale, void* out_dev, int flags,
                              void* stream) {
  g_err[0] = 0;
  const char* who = "mean around median by selection";
  if (int rc = select_check(in_dtype, M, keep, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL)) return rc;
  if (K_rows < 1 || K_rows > fjmeamedsel::kMaxClients)
    return fail(K_rows < 1 ? FJAGG_EINVAL : FJAGG_EUNSUPPORTED, "%s: a slab of 1 <= K_rows <= %d rows (got %lld)", who,
                fjmeamedsel::kMaxClients, (long long)K_rows);
  if (M > K_rows || (!rows_dev && M != K_rows))
    return fail(FJAGG_EINVAL, "%s: M <= K_rows, and M == K_rows without a row table (M=%lld, K_rows=%lld)", who,
                (long long)M, (long long)K_rows);
  if (P < 1 || ld < P) return fail(FJAGG_EINVAL, "need 1 <= P <= ld (P=%lld, ld=%lld)", (long long)P, (long long)ld);
  if (P * 4 > kMaxRowBytes) return fail(FJAGG_EUNSUPPORTED, "%s: rows <= 1 GiB", who);
  if (!x_dev || !out_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t* x = reinterpret_cast<const uint32_t*>(x_dev);
  uint32_t* y = reinterpret_cast<uint32_t*>(out_dev);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, K = (int)M, kr = (int)K_rows, kp = (int)keep;
  return (flags & FJAGG_NONTEMPORAL)
             ? FJ_SELECT_WIDTH(launch_dense, true, x, ld, kr, rows_dev, K, P, kp, scale, ds, y, s)
             : FJ_SELECT_WIDTH(launch_dense, false, x, ld, kr, rows_dev, K, P, kp, scale, ds, y, s);
}

int fjagg_meamed_select_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t keep,
                             float scale, int flags, void* stream) {
  g_err[0] = 0;
  if (int rc = select_check(in_dtype, K, keep, flags, FJAGG_SCALE | FJAGG_NONTEMPORAL | FJAGG_UNALIGNED)) return rc;
  if (nblk < 1 || nblk > 0x7fffffff || L < 1 || L >= (1 << 22))
    return fail(FJAGG_EINVAL, "bad plan (nblk=%lld, L=%d)", (long long)nblk, L);
  if (!image_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ds = (flags & FJAGG_SCALE) ? 1 : 0, k = (int)K, kp = (int)keep;
  const int V = (flags & FJAGG_UNALIGNED) ? 1 : 4;  // the plan's unit (fjagg_ptrs_plan_leaves)
  return (flags & FJAGG_NONTEMPORAL) ? FJ_SELECT_WIDTH(launch_ptrs, true, image_dev, L, k, nblk, V, kp, scale, ds, s)
                                     : FJ_SELECT_WIDTH(launch_ptrs, false, image_dev, L, k, nblk, V, kp, scale, ds, s);
}

}  // extern "C"
