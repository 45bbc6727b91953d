// fjtrust_dev.h — FLTrust's selection rule (Cao, Fang, Liu and Gong, NDSS 2021; include/fjagg.h:
// fjagg_fltrust_select) and the ordered combine of the row pass's block partials. Plain C++ that
// also compiles for the host, so the rule can be run against numpy without a GPU
// (tests/fltrust_select_host.cpp); fjtrust.hip is its only user in the library.
//
// Inputs per client k: a_k = sum fl(x_k[p] g[p]) and q_k = sum fl(x_k[p]^2), float32, both in
// fjagg_l2sq_rows' order (fjtrust.hip: dotsq_block), and q_s = sum fl(g[p]^2) from fjagg_l2sq_rows
// itself. Everything below is float64 in separate, uncontracted IEEE operations (the build has
// -ffp-contract=off on both sides), one rounding each:
//     n_k = sqrt((double)q_k);  n_s = sqrt((double)q_s)
//     cos_k = (double)a_k / (n_k n_s)
//     ts_k = cos_k > 0 ? min(cos_k, 1) : 0                      (a NaN gives 0)
//     c_k = ts_k > 0 ? (float)((ts_k n_s) / n_k) : 0
//     c_k not a finite float32 > 0: c_k = 0 and ts_k = 0
//     T = sum ts_k in client order from +0.0, sequentially;  r = T > 0 ? (float)(1.0 / T) : 0
// What follows from it: a client holding a NaN has a or q NaN and ts = 0; one holding inf or 1e30
// has q = inf, so cos is 0 or NaN and ts = 0; an all-zero client gives 0/0 and ts = 0; a client so
// small that q underflows to 0 gets c = inf, which is zeroed; a zero or non-finite server delta
// trusts nobody. The clamp at 1 matters: on clients that are exact multiples of g the float32 sums
// give cos up to 1 + 1.5e-7. A NaN diagnostic (cos, a norm) is stored as THE quiet NaN
// (0x7ff8000000000000 / 0x7fc00000): which payload a 0/0 gives differs between processors.
#pragma once
#include <stdint.h>

#include "fjselect_dev.h"

namespace fjtrust {

using fjselect::add_rn;
using fjselect::div_rn;
using fjselect::mul_rn;
using fjselect::sqrt_rn;

constexpr int kMaxClients = 4096;

FJS_HD float float_of(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float v;
  __builtin_memcpy(&v, &u, 4);
  return v;
#endif
}
FJS_HD uint32_t bits_of32(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(v);
#else
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u;
#endif
}
FJS_HD float fadd_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}

// the n partials of one client (its leaves' blocks in leaf / block order), added in order from +0:
// fjagg_l2sq_rows' combine
FJS_HD float combine(const float* part, int64_t n) {
  float s = 0.f;
  for (int64_t i = 0; i < n; ++i) s = fadd_rn(s, part[i]);
  return s;
}

// a float32 norm from its squared float32 sum: the correctly rounded root (via float64)
FJS_HD float norm_of(float q) {
  const float n = (float)sqrt_rn((double)q);
  return n == n ? n : float_of(0x7fc00000u);
}

struct Trust {
  double cos, ts;
  float c;
};

// One client's cosine, trust score and rescale factor from (a_k, q_k, q_s).
FJS_HD Trust trust_of(float a, float q, float qs) {
  Trust t;
  const double nk = sqrt_rn((double)q), ns = sqrt_rn((double)qs);
  const double cosv = div_rn((double)a, mul_rn(nk, ns));
  t.ts = cosv > 0.0 ? (cosv < 1.0 ? cosv : 1.0) : 0.0;
  t.c = t.ts > 0.0 ? (float)div_rn(mul_rn(t.ts, ns), nk) : 0.0f;
  // a finite float32 > 0: the exponent field is not all ones (that also drops a NaN)
  if (!(t.c > 0.0f) || (bits_of32(t.c) & 0x7f800000u) == 0x7f800000u) {
    t.c = 0.0f;
    t.ts = 0.0;
  }
  t.cos = cosv == cosv ? cosv : fjselect::double_of(0x7ff8000000000000ull);
  return t;
}

// T: the trust scores in client order from +0.0, sequentially (the one lane's job)
FJS_HD double trust_total(const double* ts, int K) {
  double T = 0.0;
  for (int k = 0; k < K; ++k) T = add_rn(T, ts[k]);
  return T;
}
FJS_HD float total_scale(double T) { return T > 0.0 ? (float)div_rn(1.0, T) : 0.0f; }

#if !defined(__HIP_DEVICE_COMPILE__)
// fjagg_fltrust_select's outputs from a[K], q[K] and q_s: cos[K], trust[K], factors[K], norms[K],
// *server_norm, *total, *count, order[K] (the clients with c > 0 ascending, 0 padded), seg[2],
// wperm[K] (0 padded), gscale[1].
inline void fltrust_select_host(const float* a, const float* q, float qs, int K, double* cosv, double* trust,
                                float* factors, float* norms, float* server_norm, double* total, int32_t* count,
                                int32_t* order, int32_t* seg, float* wperm, float* gscale) {
  int c = 0;
  for (int k = 0; k < K; ++k) {
    const Trust t = trust_of(a[k], q[k], qs);
    cosv[k] = t.cos;
    trust[k] = t.ts;
    factors[k] = t.c;
    norms[k] = norm_of(q[k]);
    if (t.c > 0.0f) {
      order[c] = k;
      wperm[c] = t.c;
      ++c;
    }
  }
  for (int p = c; p < K; ++p) {
    order[p] = 0;
    wperm[p] = 0.0f;
  }
  *server_norm = norm_of(qs);
  *total = trust_total(trust, K);
  *count = c;
  seg[0] = 0;
  seg[1] = c;
  gscale[0] = total_scale(*total);
}
#endif

}  // namespace fjtrust
