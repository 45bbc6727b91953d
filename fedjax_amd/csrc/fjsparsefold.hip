// fjsparsefold.hip — tree_mean folded straight from top-k clients' transmitted form
// (include/fjcomp.h: fjcomp_sparse_fold). Client k sends n_k sorted (int32 index, float32 value)
// pairs; per output coordinate i
//
//   s = +0;  for every client k that sent i, in client order: s = fl(s + fl(v * w_k));  y[i] = fl(s * scale)
//
// the multiply and the add separate (built with contraction off). For finite weights that is the
// masked fold of fjsparse.hip wherever its result is not a zero; where every term of a
// coordinate is a zero and the first is -0 the masked fold gives -0 and this one +0.
//
// The OUTPUT is partitioned, never the input, so the result takes no atomics:
//
//   workgroup   kWaves = 4 waves own kGroupTile = 4096 consecutive coordinates;
//   wave        owns kWaveTile = 1024 of them as a private float tile in LDS. No wave touches
//               another's tile: the kernel has no barrier at all.
//
// A wave takes the clients 64 at a time. Lane j binary-searches client base + j's index list for
// the tile's [lo, hi): 64 searches in flight, each about log2(n_k) dependent loads. A wave prefix
// sum over the 64 segment lengths flattens the segments into one list ordered by (client,
// index), whose per-client bookkeeping (running ends, segment pointers, weight) sits in LDS. The
// wave walks that list 64 entries a round: a lane finds its client by a 6-step search of the
// running ends, loads index and value and forms fl(v * w). The adds must reach a coordinate in
// client order, and the entries of one client never collide (its indices strictly increase), so a
// round retires its entries client group by client group: while any lane is pending, the lowest
// pending lane's client is the lowest pending client (the list is ordered), and exactly its lanes
// do the LDS read-add-write. The minimum always retires, so the loop ends; nothing in it depends
// on timing, so two runs give the same bits.
//
// Memory safety: an entry is applied only if lo <= idx < hi, which is also what keeps the LDS
// address inside the tile; a count is clamped to [0, P] and a segment to the tile's length
// before either sizes a loop. Valid lists (strictly increasing, in [0, P)) never meet a clamp; an
// unsorted list or a stray index gives an unspecified result, in bounds.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjcomp.h"

extern __attribute__((visibility("hidden"))) __thread char sparsefold_err[512] __asm__("fjagg_g_err");

static_assert(FJCOMP_SPARSE_WAVE_TILE * 4 == FJCOMP_SPARSE_GROUP_TILE, "a workgroup is four wave tiles");

namespace {

constexpr int kWaves = 4;
constexpr int kWaveTile = FJCOMP_SPARSE_WAVE_TILE;  // floats of LDS a wave accumulates in
constexpr int kGroupTile = FJCOMP_SPARSE_GROUP_TILE;
constexpr int kLanes = 64;

int refuse(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(sparsefold_err, sizeof(sparsefold_err), fmt, ap);
  va_end(ap);
  return code;
}

// Everything one wave keeps in LDS: its tile and the 64 clients of the batch in hand.
struct WaveLds {
  float tile[kWaveTile];
  const int32_t* idx[kLanes];  // the client's segment: its first entry inside [lo, hi)
  const float* val[kLanes];
  int end[kLanes];             // running end of the segments: the inclusive prefix sum of their lengths
  float w[kLanes];
};

// The LDS traffic of one wave is issued in program order; this keeps the compiler from moving
// a lane's LDS access across a point where another lane of the wave wrote.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The first position of idx[0 .. n) that holds a value >= x (n if none): reads stay inside [0, n)
// whatever the list holds.
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ idx, int n, int64_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)idx[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kWaves * kLanes) void k_sparse_fold(const int32_t* const* __restrict__ idx_ptrs,
                                                                 const float* const* __restrict__ val_ptrs,
                                                                 const int64_t* __restrict__ counts, int K, int64_t P,
                                                                 const float* __restrict__ w, float scale,
                                                                 float* __restrict__ out) {
  __shared__ WaveLds lds[kWaves];
  const int lane = threadIdx.x & (kLanes - 1);
  WaveLds& me = lds[threadIdx.x / kLanes];
  const int64_t lo = (int64_t)blockIdx.x * kGroupTile + (int64_t)(threadIdx.x / kLanes) * kWaveTile;
  if (lo >= P) return;  // the whole wave: no barrier follows
  const int64_t hi = lo + kWaveTile < P ? lo + kWaveTile : P;
  const int width = (int)(hi - lo);
  for (int e = lane; e < kWaveTile; e += kLanes) me.tile[e] = 0.0f;
  wave_sync();

  for (int base = 0; base < K; base += kLanes) {
    const int c = base + lane;
    int len = 0;
    if (c < K) {
      int64_t n64 = counts[c];
      n64 = n64 < 0 ? 0 : (n64 > P ? P : n64);
      const int n = (int)n64;
      const int32_t* __restrict__ ip = idx_ptrs[c];
      const int b = lower_bound(ip, n, lo), e = lower_bound(ip, n, hi);
      len = e > b ? e - b : 0;
      len = len < width ? len : width;  // a strictly increasing list has at most `width` entries in the tile
      me.idx[lane] = ip + b;
      me.val[lane] = val_ptrs[c] + b;
      me.w[lane] = w[c];
    }
    int end = len;  // inclusive prefix sum over the lanes
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
      const int up = __shfl_up(end, d);
      if (lane >= d) end += up;
    }
    me.end[lane] = end;
    const int total = __shfl(end, kLanes - 1);  // <= 64 * kWaveTile
    wave_sync();

    for (int r = 0; r < total; r += kLanes) {
      const int e = r + lane;
      bool pending = false;
      int j = 0, at = 0;
      float t = 0.0f;
      if (e < total) {
        // the smallest j with end[j] > e: six steps, always inside [0, 64)
#pragma unroll
        for (int step = kLanes / 2; step > 0; step >>= 1)
          if (me.end[j + step - 1] <= e) j += step;
        const int off = e - (j ? me.end[j - 1] : 0);
        const int64_t i = me.idx[j][off];
        t = __fmul_rn(me.val[j][off], me.w[j]);
        pending = i >= lo && i < hi;  // the clamp: nothing else forms an LDS address
        at = pending ? (int)(i - lo) : 0;
      }
      uint64_t m = __ballot(pending);
      while (m) {
        const int first = __ffsll((unsigned long long)m) - 1;
        const int client = __shfl(j, first);
        if (pending && j == client) {
          me.tile[at] = __fadd_rn(me.tile[at], t);
          pending = false;
        }
        wave_sync();
        m = __ballot(pending);
      }
    }
    wave_sync();  // the next batch overwrites the client table
  }

  for (int e = lane; e < width; e += kLanes) out[lo + e] = __fmul_rn(me.tile[e], scale);
}

}  // namespace

extern "C" {

int fjcomp_sparse_fold(const int32_t* const* idx_ptrs, const float* const* val_ptrs, const int64_t* counts, int64_t K,
                       int64_t P, const float* w_dev, float scale, float* out_dev, int flags, void* stream) {
  const char* what = "sparse_fold";
  if (flags) return refuse(FJAGG_EUNSUPPORTED, "%s: unsupported flags 0x%x", what, flags);
  if (K < 1) return refuse(FJAGG_EINVAL, "%s: K must be >= 1 (got %lld)", what, (long long)K);
  if (K > FJCOMP_TOPK_MAX_CLIENTS)
    return refuse(FJAGG_EUNSUPPORTED, "%s: K <= %d clients (got %lld)", what, FJCOMP_TOPK_MAX_CLIENTS, (long long)K);
  if (P < 0) return refuse(FJAGG_EINVAL, "%s: P must be >= 0 (got %lld)", what, (long long)P);
  if (P >= (1ll << 31)) return refuse(FJAGG_EUNSUPPORTED, "%s: P < 2^31 elements per client (got %lld)", what, (long long)P);
  if (P == 0) return FJAGG_OK;
  if (!idx_ptrs || !val_ptrs || !counts) return refuse(FJAGG_EINVAL, "%s: null table", what);
  if (!w_dev || !out_dev) return refuse(FJAGG_EINVAL, "%s: null pointer argument", what);
  const unsigned grid = (unsigned)((P + kGroupTile - 1) / kGroupTile);
  hipLaunchKernelGGL(k_sparse_fold, dim3(grid), dim3(kWaves * kLanes), 0, reinterpret_cast<hipStream_t>(stream),
                     idx_ptrs, val_ptrs, counts, (int)K, P, w_dev, scale, out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(FJAGG_EHIP, "k_sparse_fold: %s", hipGetErrorString(e));
  return FJAGG_OK;
}

}  // extern "C"
