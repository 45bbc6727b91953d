// fjrand_dev.h — jax.random's generator on the device, shared by the compression kernels
// (fjcomp.hip) and the noise epilogue of the clipped folds (fjagg.hip): Threefry-2x32-20 with
// JAX's key schedule, and the bits -> uniform -> standard normal maps of jax.random.normal.
// Internal to the library (anonymous namespace: each translation unit gets its own copy); the
// C ABI is include/fjcomp.h.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// ------------------------------------------------------------------ threefry2x32-20
__host__ __device__ inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

#define FJ_TF_ROUND(r) \
  x0 += x1;            \
  x1 = rotl32(x1, r);  \
  x1 ^= x0;
#define FJ_TF_ROT0 FJ_TF_ROUND(13) FJ_TF_ROUND(15) FJ_TF_ROUND(26) FJ_TF_ROUND(6)
#define FJ_TF_ROT1 FJ_TF_ROUND(17) FJ_TF_ROUND(29) FJ_TF_ROUND(16) FJ_TF_ROUND(24)

// Threefry-2x32 with 20 rounds and JAX's key schedule (jax/_src/prng.py); k2 = k0 ^ k1 ^ C.
__host__ __device__ inline void threefry_k(uint32_t k0, uint32_t k1, uint32_t k2, uint32_t& x0, uint32_t& x1) {
  x0 += k0;
  x1 += k1;
  FJ_TF_ROT0 x0 += k1; x1 += k2 + 1u;
  FJ_TF_ROT1 x0 += k2; x1 += k0 + 2u;
  FJ_TF_ROT0 x0 += k0; x1 += k1 + 3u;
  FJ_TF_ROT1 x0 += k1; x1 += k2 + 4u;
  FJ_TF_ROT0 x0 += k2; x1 += k0 + 5u;
}
__host__ __device__ inline void threefry(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  threefry_k(k0, k1, k0 ^ k1 ^ 0x1BD11BDAu, x0, x1);
}

// jax.random.uniform's bits -> [0, 1): bitcast((b >> 9) | 1.0f) - 1
// ((b >> 9) | 0x3f800000) is one v_alignbit: the low word of (0x7f : b) >> 9.
__device__ inline float bits_to_unit(uint32_t b) {
  return __uint_as_float(__builtin_amdgcn_alignbit(0x7fu, b, 9u)) - 1.0f;
}

// ------------------------------------------------------------------ standard normal
// jax.random.normal's float32 draw from 32 random bits (jax/_src/random.py _normal_real):
//   u = uniform(minval = lo, maxval = 1), lo = nextafter(-1f, 0f):
//       f = bits_to_unit(b);  u = max(lo, fl(fl(f * fl(1 - lo)) + lo)),  fl(1 - lo) = 2 exactly
//   z = sqrt(2) * erfinv(u)
// u is never +-1, so z is finite. The bits and u are jax's; the last step is the f64 device
// erfinv times RN_f64(sqrt 2), rounded once to f32 (the style of div_rn / sqrt_rn in fjagg.hip):
// the correctly rounded value of the exact function up to rare ties. XLA's own f32 erf_inv
// polynomial is not reproduced.
__device__ inline float normal_from_bits(uint32_t b) {
  const float lo = -0.99999994f;  // nextafter(-1f, 0f) = -(1 - 2^-24)
  const float f = bits_to_unit(b);
  const float u = fmaxf(lo, __fadd_rn(__fmul_rn(f, 2.0f), lo));
  return (float)(1.4142135623730951 * erfinv((double)u));
}

// Element i of jax.random.normal(key, (n,)): random_bits' counter layout (the count array
// iota(n) padded to even length and split into halves of h = ceil(n / 2)): element i < h is
// y0 of the pair (i, i + h), element i >= h is y1 of the pair (i - h, i); the pad pair of an
// odd n is (h - 1, 0). One Threefry block per element (its partner's word is dropped).
__device__ inline float normal_at(uint32_t k0, uint32_t k1, uint32_t k2, int64_t i, int64_t n) {
  const int64_t h = (n + 1) >> 1;
  const bool first = i < h;
  const int64_t p = first ? i : i - h;
  uint32_t x0 = (uint32_t)p, x1 = (uint32_t)(p + h < n ? p + h : 0);
  threefry_k(k0, k1, k2, x0, x1);
  return normal_from_bits(first ? x0 : x1);
}

}  // namespace
