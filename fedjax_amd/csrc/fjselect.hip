// fjselect.hip — Krum's and the smoothed Weiszfeld algorithm's selection on the device
// (include/fjagg.h: fjagg_krum_select, fjagg_weiszfeld_select, fjagg_gather_member_ptrs). The
// input is the K x K float64 Gram matrix of fjgram.hip; the outputs include the member tables
// order | seg | wperm | gscale of ONE group, written where the grouped fold reads them
// (fjagg_wsum_group_*_dev), so a round is Gram -> select -> fold with no host visit.
//
// The arithmetic is fjselect_dev.h's, one index per lane and a barrier between the phases;
// every sequential sum is added by one lane. K <= 1024, float64, small and latency-bound:
//   k_krum_scores     one workgroup per row i: K keys into LDS (8 KiB), a bitonic sort, lane 0
//                     adds the first K - f - 2
//   k_krum_rank       one workgroup: ranks (score, index), writes selected, count and the tables
//   k_weiszfeld       one workgroup of 1024 lanes runs all iterations: lane k owns client k and
//                     walks column k of G (row k's bits, coalesced), a in LDS
//   k_gather_members  copies the selected clients' leaf pointers into a grouped plan image
//   k_bulyan_sort     (fjagg_bulyan_select, K <= 252) one workgroup per row: its (key, index) pairs
//                     sorted in LDS, written position-major into the workspace
//   k_bulyan_steps    one workgroup of 256 lanes runs all K - 2f steps: lane i walks row i's sorted
//                     list past the clients already chosen, then an argmin on (score bits, index);
//                     writes the row table, count, keep and scale that fjagg_meamed_*_dev read
// No floating-point atomics; two runs give the same bits.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjagg.h"
#include "fjselect_dev.h"

extern __attribute__((visibility("hidden"))) __thread char fjagg_g_err[512];
#define g_err fjagg_g_err

namespace {

using namespace fjselect;

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

constexpr int kThreads = 256;
constexpr int kWideThreads = kMaxClients;  // k_weiszfeld: one lane per client

__global__ __launch_bounds__(kThreads) void k_krum_scores(const double* __restrict__ G, int K, int n,
                                                          double* __restrict__ scores) {
  __shared__ uint64_t keys[kMaxClients];
  const int i = blockIdx.x, tid = threadIdx.x, N = pow2_at_least(K);
  const double gii = G[(int64_t)i * K + i];
  const bool ok_i = finite(gii);
  for (int t = tid; t < N; t += kThreads) keys[t] = krum_key(G, K, i, t, gii, ok_i);
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N; t += kThreads) bitonic_cx(keys, t, j, k);
      __syncthreads();
    }
  if (tid == 0) scores[i] = krum_score(keys, n, ok_i);
}

__global__ __launch_bounds__(kThreads) void k_krum_rank(const double* __restrict__ scores, int K, int m,
                                                        int64_t* __restrict__ selected, int32_t* __restrict__ count,
                                                        int32_t* __restrict__ order, int32_t* __restrict__ seg,
                                                        float* __restrict__ wperm, float* __restrict__ gscale) {
  __shared__ uint64_t sk[kMaxClients];
  __shared__ uint8_t flags[kMaxClients];
  __shared__ int total;
  const int tid = threadIdx.x;
  for (int i = tid; i < K; i += kThreads) sk[i] = bits_of(scores[i]);
  __syncthreads();
  for (int i = tid; i < K; i += kThreads) {
    const int r = krum_rank(sk, K, i);
    const bool sel = (sk[i] & kInfBits) != kInfBits && r < m;
    flags[i] = sel;
    if (sel) selected[r] = i;
  }
  __syncthreads();
  if (tid == 0) total = flags_below(flags, K);
  for (int i = tid; i < K; i += kThreads)
    if (flags[i]) order[flags_below(flags, i)] = i;
  __syncthreads();
  const int c = total;
  for (int r = tid; r < m; r += kThreads) {
    wperm[r] = 1.0f;
    if (r >= c) {
      selected[r] = -1;
      order[r] = 0;
    }
  }
  if (tid == 0) {
    *count = c;
    seg[0] = 0;
    seg[1] = c;
    gscale[0] = krum_gscale(c);
  }
}

__global__ __launch_bounds__(kWideThreads) void k_weiszfeld(
    const double* __restrict__ G, int K, const double* __restrict__ alpha, double nu, int iterations,
    double* __restrict__ a_out, double* __restrict__ d_out, float* __restrict__ a32_out, int32_t* __restrict__ count,
    int32_t* __restrict__ order, int32_t* __restrict__ seg, float* __restrict__ wperm, float* __restrict__ gscale) {
  __shared__ double a[kMaxClients], ga[kMaxClients], beta[kMaxClients];
  __shared__ float a32s[kMaxClients];
  __shared__ uint8_t ok[kMaxClients], member[kMaxClients];
  __shared__ double sums[2];
  __shared__ int total;
  const int k = threadIdx.x;
  const bool in = k < K;
  const double gkk = in ? G[(int64_t)k * K + k] : 0.0;
  const bool okk = in && finite(gkk);
  const double al = in ? (alpha ? alpha[k] : 1.0) : 0.0;
  ok[k] = okk;
  beta[k] = al;
  __syncthreads();
  if (k == 0) sums[0] = usable_sum(beta, ok, K);
  __syncthreads();
  double a_k = okk ? div_rn(al, sums[0]) : 0.0;
  double d_k = okk ? 0.0 : double_of(kInfBits);
  a[k] = a_k;
  __syncthreads();
  for (int it = 0; it < iterations; ++it) {
    ga[k] = okk ? weiszfeld_ga(G, K, k, a, ok) : 0.0;
    __syncthreads();
    if (k == 0) sums[0] = weiszfeld_q(a, ga, ok, K);
    __syncthreads();
    double b = 0.0;
    if (okk) {
      d_k = weiszfeld_distance(sums[0], ga[k], gkk);
      b = weiszfeld_beta(al, nu, d_k);
    }
    beta[k] = b;
    __syncthreads();
    if (k == 0) sums[1] = usable_sum(beta, ok, K);
    __syncthreads();
    if (okk) a_k = div_rn(b, sums[1]);
    a[k] = a_k;
    __syncthreads();
  }
  const float a32_k = (float)a_k;
  const bool mem = okk && a32_k > 0.0f;
  a32s[k] = a32_k;
  member[k] = mem;
  __syncthreads();
  if (k == 0) {
    const int c = flags_below(member, K);
    total = c;
    *count = c;
    seg[0] = 0;
    seg[1] = c;
    gscale[0] = total_gscale(member_total(a32s, member, K));
  }
  if (in) {
    a_out[k] = a_k;
    d_out[k] = d_k;
    a32_out[k] = a32_k;
  }
  if (mem) {
    const int p = flags_below(member, k);
    order[p] = k;
    wperm[p] = a32_k;
  }
  __syncthreads();
  if (in && k >= total) {
    order[k] = 0;
    wperm[k] = 0.0f;
  }
}

// slot j < count of the group image gets client order[j]'s L leaf pointers
__global__ __launch_bounds__(kThreads) void k_gather_members(const int64_t* __restrict__ all, int L, int K,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ seg, int M_max,
                                                             int64_t* __restrict__ group) {
  int count = seg[1] - seg[0];
  if (count > M_max) count = M_max;
  const int64_t n = (int64_t)count * L;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads)
    gather_member_word(all, L, K, order, idx, group);
}

// Bulyan's first launch: row i's K - 1 (key, index) pairs sorted by (key, index) in LDS and written
// position-major, position p of row i at p*K + i.
__global__ __launch_bounds__(kBulyanLanes) void k_bulyan_sort(const double* __restrict__ G, int K,
                                                              uint64_t* __restrict__ skeys,
                                                              uint8_t* __restrict__ sidx) {
  __shared__ uint64_t keys[kBulyanLanes];
  __shared__ uint8_t idx[kBulyanLanes];
  const int i = blockIdx.x, t = threadIdx.x, N = pow2_at_least(K);
  const double gii = G[(int64_t)i * K + i];
  const bool ok_i = finite(gii);
  if (t < N) {
    keys[t] = krum_key(G, K, i, t, gii, ok_i);
    idx[t] = (uint8_t)t;
  }
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (t < N) bitonic_cx_pair(keys, idx, t, j, k);
      __syncthreads();
    }
  if (t < K - 1) {  // the pads (i itself, t >= K) sort last and stay behind
    skeys[(int64_t)t * K + i] = keys[t];
    sidx[(int64_t)t * K + i] = idx[t];
  }
}

// Bulyan's second launch: ONE workgroup runs all theta steps, lane i owns client i. A step: every
// live lane adds its first c live neighbours, the wave and then the workgroup reduce (score bits,
// index) to its minimum, the winner leaves R. Every lane reads the same four wave minima, so the
// winner and the decision to stop are uniform.
__global__ __launch_bounds__(kBulyanLanes) void k_bulyan_steps(
    const double* __restrict__ G, int K, int f, const uint64_t* __restrict__ skeys, const uint8_t* __restrict__ sidx,
    int64_t* __restrict__ selected, int32_t* __restrict__ count, double* __restrict__ step_scores,
    int32_t* __restrict__ keep_out, float* __restrict__ scale_out, int32_t* __restrict__ rows) {
  constexpr int kWaves = kBulyanLanes / 64;
  __shared__ uint8_t alive[kBulyanLanes], chosen[kBulyanLanes];
  __shared__ uint64_t wave_best[kWaves];
  __shared__ int wave_who[kWaves];
  __shared__ int live0, last_row;
  const int i = threadIdx.x, theta = K - 2 * f;
  const bool ok_i = i < K && finite(G[(int64_t)i * K + i]);
  alive[i] = ok_i;
  chosen[i] = 0;
  if (i == 0) last_row = 0;
  __syncthreads();
  if (i == 0) live0 = flags_below(alive, K);
  __syncthreads();
  int n = live0, c = 0;
  bool live = ok_i;
  for (; c < theta; ++c) {
    const double s = live ? bulyan_score(skeys, sidx, K, i, bulyan_neighbours(n, f), alive) : 0.0;
    uint64_t best = bulyan_candidate(s, live);
    int who = i;
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t ob = __shfl_xor((unsigned long long)best, off);
      const int ow = __shfl_xor(who, off);
      if (bulyan_before(ob, ow, best, who)) {
        best = ob;
        who = ow;
      }
    }
    if ((i & 63) == 0) {
      wave_best[i >> 6] = best;
      wave_who[i >> 6] = who;
    }
    __syncthreads();
    best = wave_best[0];
    who = wave_who[0];
    for (int w = 1; w < kWaves; ++w)
      if (bulyan_before(wave_best[w], wave_who[w], best, who)) {
        best = wave_best[w];
        who = wave_who[w];
      }
    if (best == kPadKey) break;  // R is empty, or no score is finite (uniform)
    if (i == who) {
      selected[c] = who;
      step_scores[c] = double_of(best);
      alive[i] = 0;
      chosen[i] = 1;
      live = false;
    }
    --n;
    __syncthreads();
  }
  __syncthreads();
  if (i < K && chosen[i]) {
    const int slot = flags_below(chosen, i);
    rows[slot] = i;
    if (slot == c - 1) last_row = i;
  }
  __syncthreads();
  if (i >= c && i < theta) {
    selected[i] = -1;
    step_scores[i] = double_of(kInfBits);
    rows[i] = last_row;
  }
  if (i == 0) {
    const int keep = bulyan_keep(c, f);
    *count = c;
    *keep_out = keep;
    *scale_out = bulyan_scale(keep);
  }
}

int check_clients(const char* what, int64_t K) {
  if (K < 1) return fail(FJAGG_EINVAL, "%s: K must be >= 1 (got %lld)", what, (long long)K);
  if (K > kMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "%s: K <= %d clients (got %lld)", what, kMaxClients, (long long)K);
  return FJAGG_OK;
}

}  // namespace

extern "C" {

int fjagg_krum_select(const double* gram_dev, int64_t K, int64_t f, int64_t m, double* scores_dev,
                      int64_t* selected_dev, int32_t* count_dev, int32_t* order_dev, int32_t* seg_dev,
                      float* wperm_dev, float* gscale_dev, void* stream) {
  g_err[0] = 0;
  if (int rc = check_clients("krum select", K)) return rc;
  if (f < 0) return fail(FJAGG_EINVAL, "krum select: f must be >= 0 (got %lld)", (long long)f);
  if (f > K || K < 2 * f + 3)
    return fail(FJAGG_EINVAL, "krum select: needs K >= 2f + 3 clients (K=%lld, f=%lld)", (long long)K, (long long)f);
  if (m < 1 || m > K - f)
    return fail(FJAGG_EINVAL, "krum select: m must be in [1, K - f] = [1, %lld] (got %lld)", (long long)(K - f),
                (long long)m);
  if (!gram_dev || !scores_dev || !selected_dev || !count_dev || !order_dev || !seg_dev || !wperm_dev || !gscale_dev)
    return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_krum_scores, dim3((unsigned)K), dim3(kThreads), 0, s, gram_dev, (int)K, (int)(K - f - 2),
                     scores_dev);
  if (int rc = check_launch("k_krum_scores")) return rc;
  hipLaunchKernelGGL(k_krum_rank, dim3(1), dim3(kThreads), 0, s, scores_dev, (int)K, (int)m, selected_dev, count_dev,
                     order_dev, seg_dev, wperm_dev, gscale_dev);
  return check_launch("k_krum_rank");
}

int fjagg_weiszfeld_select(const double* gram_dev, int64_t K, const double* alpha_dev, double nu, int64_t iterations,
                           double* a_dev, double* d_dev, float* a32_dev, int32_t* count_dev, int32_t* order_dev,
                           int32_t* seg_dev, float* wperm_dev, float* gscale_dev, void* stream) {
  g_err[0] = 0;
  if (int rc = check_clients("weiszfeld select", K)) return rc;
  if (iterations < 0)
    return fail(FJAGG_EINVAL, "weiszfeld select: iterations must be >= 0 (got %lld)", (long long)iterations);
  if (iterations > 0x7fffffffll)
    return fail(FJAGG_EUNSUPPORTED, "weiszfeld select: iterations < 2^31 (got %lld)", (long long)iterations);
  if (!(nu > 0.0) || !finite(nu)) return fail(FJAGG_EINVAL, "weiszfeld select: nu must be finite and > 0 (got %g)", nu);
  if (!gram_dev || !a_dev || !d_dev || !a32_dev || !count_dev || !order_dev || !seg_dev || !wperm_dev || !gscale_dev)
    return fail(FJAGG_EINVAL, "null pointer argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_weiszfeld, dim3(1), dim3(kWideThreads), 0, s, gram_dev, (int)K, alpha_dev, nu, (int)iterations,
                     a_dev, d_dev, a32_dev, count_dev, order_dev, seg_dev, wperm_dev, gscale_dev);
  return check_launch("k_weiszfeld");
}

int64_t fjagg_bulyan_select_workspace_bytes(int64_t K) {
  if (K < 3 || K > kBulyanMaxClients) return 0;
  return K * (K - 1) * 9;  // the sorted keys (8 bytes) and their client indices (1 byte)
}

int fjagg_bulyan_select(const double* gram_dev, int64_t K, int64_t f, void* ws_dev, int64_t ws_bytes,
                        int64_t* selected_dev, int32_t* count_dev, double* step_scores_dev, int32_t* keep_dev,
                        float* scale_dev, int32_t* rows_dev, void* stream) {
  g_err[0] = 0;
  if (int rc = check_clients("bulyan select", K)) return rc;
  if (f < 0) return fail(FJAGG_EINVAL, "bulyan select: f must be >= 0 (got %lld)", (long long)f);
  if (f > K || K < 4 * f + 3)
    return fail(FJAGG_EINVAL, "bulyan select: needs K >= 4f + 3 clients (K=%lld, f=%lld)", (long long)K, (long long)f);
  if (K - 2 * f > kBulyanMaxSelected)
    return fail(FJAGG_EUNSUPPORTED, "bulyan select: K - 2f <= %d selected clients (K=%lld, f=%lld)", kBulyanMaxSelected,
                (long long)K, (long long)f);
  // K >= 4f + 3 and K - 2f <= 128: 2f <= (K - 3) / 2, so K <= 128 + (K - 3) / 2 and K <= 252 (checked again
  // because the kernels' LDS arrays and the byte indices rest on it)
  if (K > kBulyanMaxClients)
    return fail(FJAGG_EUNSUPPORTED, "bulyan select: K <= %d clients (got %lld)", kBulyanMaxClients, (long long)K);
  if (!gram_dev || !ws_dev || !selected_dev || !count_dev || !step_scores_dev || !keep_dev || !scale_dev || !rows_dev)
    return fail(FJAGG_EINVAL, "null pointer argument");
  if (ws_bytes < fjagg_bulyan_select_workspace_bytes(K) || (reinterpret_cast<uintptr_t>(ws_dev) & 7))
    return fail(FJAGG_EINVAL, "bulyan select: workspace of %lld bytes, 8-byte aligned (got %lld)",
                (long long)fjagg_bulyan_select_workspace_bytes(K), (long long)ws_bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint64_t* skeys = reinterpret_cast<uint64_t*>(ws_dev);
  uint8_t* sidx = reinterpret_cast<uint8_t*>(skeys + K * (K - 1));
  hipLaunchKernelGGL(k_bulyan_sort, dim3((unsigned)K), dim3(kBulyanLanes), 0, s, gram_dev, (int)K, skeys, sidx);
  if (int rc = check_launch("k_bulyan_sort")) return rc;
  hipLaunchKernelGGL(k_bulyan_steps, dim3(1), dim3(kBulyanLanes), 0, s, gram_dev, (int)K, (int)f, skeys, sidx,
                     selected_dev, count_dev, step_scores_dev, keep_dev, scale_dev, rows_dev);
  return check_launch("k_bulyan_steps");
}

int fjagg_gather_member_ptrs(const int64_t* image_all_dev, int L, int64_t K, const int32_t* order_dev,
                             const int32_t* seg_dev, int64_t M_max, int64_t* image_group_dev, void* stream) {
  g_err[0] = 0;
  if (int rc = check_clients("gather members", K)) return rc;
  if (L < 1) return fail(FJAGG_EINVAL, "gather members: L must be >= 1 (got %d)", L);
  if (M_max < 1 || M_max > K)
    return fail(FJAGG_EINVAL, "gather members: M_max must be in [1, K] = [1, %lld] (got %lld)", (long long)K,
                (long long)M_max);
  if (!image_all_dev || !order_dev || !seg_dev || !image_group_dev) return fail(FJAGG_EINVAL, "null pointer argument");
  int64_t blocks = (M_max * L + kThreads - 1) / kThreads;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_gather_members, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     image_all_dev, L, (int)K, order_dev, seg_dev, (int)M_max, image_group_dev);
  return check_launch("k_gather_members");
}

}  // extern "C"
