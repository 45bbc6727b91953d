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
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
    const int64_t j = idx / L, l = idx - j * L;
    const int c = order[j];
    if ((unsigned)c < (unsigned)K) group[idx] = all[(int64_t)c * L + l];
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
