// fjsignvote.hip — signSGD with majority vote, from the bits the clients transmit
// (include/fjcomp.h: fjcomp_sign_pack, fjcomp_sign_vote).
//
// Client k sends one bit per coordinate (coordinate i of a leaf in byte i / 8 at bit i % 8, low
// bit first; 1 <=> the value is < 0). Per coordinate, with c the number of clients whose bit is 1:
//
//   sign mode   y = -1 if 2c > K,  +1 if 2c < K,  +0 if 2c == K
//   mean mode   y = fl(f32(K - 2c) * scale)            (K - 2c is exact; scale = f32(1 / K))
//
// Everything before the last instruction is integer work, and the count is kept BIT-SLICED
// ("vertical counters"): for one 32-bit word of a leaf, plane j is a word whose bit b is bit j of
// the count of coordinate b. Adding a client's word is then a ripple of half adders over the
// planes, a few integer operations for 32 coordinates at once.
//
// Work split:
//
//   workgroup   kWaves = 4 waves own one tile of FJCOMP_VOTE_TILE = 8192 coordinates of one leaf
//               (1024 packed bytes per client), found by find_segment over the block prefix;
//   lane        owns kWords = 4 consecutive words of the tile: one 16-byte load per client;
//   wave v      counts clients v, v + 4, v + 8, ...: at most 1024 of them, kWavePlanes = 11 planes
//               per word (44 registers), four independent load streams per tile.
//
// A wave takes its clients kGroup = 8 at a time. The eight words are first compressed with full
// adders (a ^ b ^ c, majority) into one word each of weight 1, 2, 4 and 8, and only those four are
// rippled into the planes: one ripple per group instead of eight. A missing client of the last
// group is a zero word, which adds nothing, so every K mod 8 and every K mod 4 is the same code.
// The next group's loads are issued before the current group is compressed. The client pointers
// are staged in LDS kChunk = 1024 at a time.
//
// After the client loop every wave writes its planes to LDS, word-major, and the waves swap roles:
// wave v, lane i now owns word 64 v + i of the tile. It adds the four partial counters of that
// word bit-sliced (ripple-carry over kPlanes = 13 planes: counts up to 4096), forms its 32
// outputs and stores them 16 bytes at a time. So the combine and the epilogue are split four
// ways as well. Integer addition is associative: the result does not depend on the split, there
// are no atomics, and two runs give the same bits.
//
// sign mode never extracts a count: 2c against K is c against h = K / 2, compared bit-sliced from
// the top plane down into two masks (c > h; c == h, a tie only when K is even). mean mode gathers
// the bit_length(K) planes that can be set into an integer per coordinate.
//
// Memory safety: a lane loads 16 bytes at once only when the client's pointer is 16-byte aligned
// and the 16 bytes lie inside the packed leaf; otherwise byte by byte, each byte guarded by the
// leaf's byte count, so no address past a leaf's last byte is formed into a load and bytes outside
// the leaf count as 0. Padding bits of a last byte are counted and never stored: an output is
// stored only if its coordinate is < n. LDS indices are compile-time functions of the lane.
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fjcomp.h"

extern __attribute__((visibility("hidden"))) __thread char signvote_err[512] __asm__("fjagg_g_err");

namespace {

constexpr int kLanes = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * kLanes;
constexpr int kWords = 4;                                // 32-bit words a lane loads per client
constexpr int kTileWords = kLanes * kWords;              // 256
constexpr int kTile = kTileWords * 32;                   // coordinates a workgroup owns
constexpr int kTileBytes = kTile / 8;                    // 1024
constexpr int kGroup = 8;                                // clients compressed together
constexpr int kPlanes = 13;                              // counts up to 4096
constexpr int kWavePlanes = 11;                          // a wave's share: up to 1024
constexpr int kChunk = 1024;                             // client pointers staged at a time
constexpr int kPackThreads = 256;
static_assert(kTile == FJCOMP_VOTE_TILE, "coordinates per workgroup");
static_assert(FJCOMP_VOTE_MAX_CLIENTS == 1 << (kPlanes - 1), "the top plane is the count K = 4096 alone");
static_assert((FJCOMP_VOTE_MAX_CLIENTS + kWaves - 1) / kWaves == 1 << (kWavePlanes - 1), "a wave's planes hold its share");
static_assert(kChunk % (kWaves * kGroup) == 0 && kChunk % kThreads == 0, "whole groups per wave and chunk");
static_assert(kPackThreads * 8 == FJCOMP_SIGN_PACK_BLOCK, "a lane packs one byte");

int refuse(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(signvote_err, sizeof(signvote_err), fmt, ap);
  va_end(ap);
  return code;
}

// Segment of block b in a running-sum table prefix[nseg + 1] (skips empty segments): the
// wave-parallel 64-ary search of fjcomp.hip. Every lane of the wave calls it with the same b.
__device__ inline int64_t find_segment(const int64_t* __restrict__ prefix, int64_t nseg, int64_t b) {
  const int64_t lane = threadIdx.x & 63;
  int64_t lo = 0, hi = nseg;  // prefix[lo] <= b < prefix[hi]
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t idx = lo + lane * step;
    const uint64_t m = __ballot(idx < hi && prefix[idx] <= b);
    lo += (int64_t)(63 - __builtin_clzll(m)) * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  return lo;
}

__device__ __forceinline__ uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a ^ b)); }

// A lane's kWords words of one client.
struct Run {
  uint32_t v[kWords];
};

// The 16 bytes at p, of which `bleft` lie inside the packed leaf (the rest read as 0; <= 0: none).
__device__ __forceinline__ Run load_run(const uint8_t* __restrict__ p, int64_t bleft) {
  Run r;
  if (bleft >= 4 * kWords && ((uintptr_t)p & 15) == 0) {
    const uint4 x = *reinterpret_cast<const uint4*>(p);
    r.v[0] = x.x, r.v[1] = x.y, r.v[2] = x.z, r.v[3] = x.w;
    return r;
  }
#pragma unroll
  for (int q = 0; q < kWords; ++q) r.v[q] = 0u;
#pragma unroll
  for (int j = 0; j < 4 * kWords; ++j)
    if (j < bleft) r.v[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
  return r;
}

// Eight clients' words a[0..7] added into the planes p of one word: carry-save down to one word
// of each weight 1, 2, 4, 8, then one ripple. The carry out of the top plane is zero by the
// bound on the clients a wave counts.
__device__ __forceinline__ void add_group(uint32_t (&p)[kWavePlanes], const uint32_t (&a)[kGroup]) {
  const uint32_t s0 = a[0] ^ a[1] ^ a[2], c0 = maj(a[0], a[1], a[2]);
  const uint32_t s1 = a[3] ^ a[4] ^ a[5], c1 = maj(a[3], a[4], a[5]);
  const uint32_t s2 = a[6] ^ a[7], c2 = a[6] & a[7];
  const uint32_t w1 = s0 ^ s1 ^ s2, c3 = maj(s0, s1, s2);
  const uint32_t t0 = c0 ^ c1 ^ c2, d0 = maj(c0, c1, c2);
  const uint32_t w2 = t0 ^ c3, d1 = t0 & c3;
  const uint32_t w[4] = {w1, w2, d0 ^ d1, d0 & d1};
  uint32_t carry = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t s = p[j] ^ w[j] ^ carry;
    carry = maj(p[j], w[j], carry);
    p[j] = s;
  }
#pragma unroll
  for (int j = 4; j < kWavePlanes; ++j) {
    const uint32_t s = p[j] ^ carry;
    carry &= p[j];
    p[j] = s;
  }
}

// LDS of a workgroup: the staged client pointers during the client loop, then the four waves'
// planes, word-major (a lane's four words are one 16-byte write, a word's reader is one lane).
union alignas(16) VoteLds {
  uint64_t ptr[kChunk];
  uint32_t part[kWaves][kWavePlanes][kTileWords];
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_sign_vote(const uint8_t* const* __restrict__ bit_ptrs, int K, int64_t L,
                                                        const int64_t* __restrict__ leaf_n,
                                                        const int64_t* __restrict__ prefix, float scale,
                                                        float* const* __restrict__ out_ptrs) {
  __shared__ VoteLds lds;
  const int64_t b = blockIdx.x;
  const int64_t l = find_segment(prefix, L, b);
  const int tid = threadIdx.x, lane = tid & (kLanes - 1), wave = tid / kLanes;
  const int64_t n = leaf_n[l];
  const int64_t tile = b - prefix[l];
  const int64_t nbytes = (n + 7) >> 3;                                   // the packed leaf
  const int64_t boff = tile * kTileBytes + (int64_t)lane * 4 * kWords;   // this lane's first byte in it
  const int64_t bleft = nbytes - boff;                                   // its bytes inside (<= 0: none)

  uint32_t p[kWords][kWavePlanes];
#pragma unroll
  for (int q = 0; q < kWords; ++q)
#pragma unroll
    for (int j = 0; j < kWavePlanes; ++j) p[q][j] = 0u;

  // clients g .. g + 7 of this wave's share of the staged chunk (share entry i is chunk entry
  // wave + 4 i; those at or past cnt are zero words)
  auto fetch = [&](int g, int cnt, Run (&x)[kGroup]) {
#pragma unroll
    for (int u = 0; u < kGroup; ++u) {
      if (g + u < cnt) {  // wave-uniform
        x[u] = load_run(reinterpret_cast<const uint8_t*>(lds.ptr[wave + kWaves * (g + u)]) + boff, bleft);
      } else {
#pragma unroll
        for (int q = 0; q < kWords; ++q) x[u].v[q] = 0u;
      }
    }
  };
  auto count = [&](const Run (&x)[kGroup]) {
#pragma unroll
    for (int q = 0; q < kWords; ++q) {
      uint32_t a[kGroup];
#pragma unroll
      for (int u = 0; u < kGroup; ++u) a[u] = x[u].v[q];
      add_group(p[q], a);
    }
  };

  for (int kc = 0; kc < K; kc += kChunk) {
    const int jn = K - kc < kChunk ? K - kc : kChunk;
    if (kc) __syncthreads();  // every wave has read the previous chunk's pointers
    for (int j = tid; j < jn; j += kThreads) lds.ptr[j] = (uint64_t)bit_ptrs[(int64_t)(kc + j) * L + l];
    __syncthreads();
    const int cnt = jn > wave ? (jn - wave + kWaves - 1) / kWaves : 0;  // this wave's clients of the chunk
    Run xa[kGroup], xb[kGroup];
    if (cnt > 0) fetch(0, cnt, xa);
    for (int g = 0; g < cnt; g += 2 * kGroup) {
      if (g + kGroup < cnt) fetch(g + kGroup, cnt, xb);
      count(xa);
      if (g + kGroup >= cnt) break;
      if (g + 2 * kGroup < cnt) fetch(g + 2 * kGroup, cnt, xa);
      count(xb);
    }
  }

  __syncthreads();  // the pointers are done with: the planes take their place
#pragma unroll
  for (int j = 0; j < kWavePlanes; ++j)
    *reinterpret_cast<uint4*>(&lds.part[wave][j][kWords * lane]) = uint4{p[0][j], p[1][j], p[2][j], p[3][j]};
  __syncthreads();

  // this lane's word of the tile from here on: the four partial counters, added bit-sliced
  const int word = wave * kLanes + lane;
  const int64_t e0 = tile * kTile + (int64_t)word * 32;
  const int64_t left = n - e0;  // its coordinates inside the leaf (<= 0: none)
  if (left <= 0) return;        // (no barrier follows)
  uint32_t c[kPlanes];
#pragma unroll
  for (int j = 0; j < kPlanes; ++j) c[j] = j < kWavePlanes ? lds.part[0][j][word] : 0u;
#pragma unroll
  for (int s = 1; s < kWaves; ++s) {
    uint32_t carry = 0u;
#pragma unroll
    for (int j = 0; j < kPlanes; ++j) {
      const uint32_t t = j < kWavePlanes ? lds.part[s][j][word] : 0u;
      const uint32_t sum = c[j] ^ t ^ carry;
      carry = maj(c[j], t, carry);
      c[j] = sum;
    }
  }

  uint32_t neg = 0u, tie = 0u;
  int np = 0;
  if constexpr (MODE == FJCOMP_VOTE_SIGN) {
    // c against h = K / 2 from the top plane down: neg <=> c > h, tie <=> c == h
    const uint32_t h = (uint32_t)K >> 1;
    tie = ~0u;
#pragma unroll
    for (int j = kPlanes - 1; j >= 0; --j) {
      if ((h >> j) & 1u) {
        tie &= c[j];
      } else {
        neg |= tie & c[j];
        tie &= ~c[j];
      }
    }
    if (K & 1) tie = 0u;  // odd K: c == h is 2c < K
  } else {
    np = 32 - __builtin_clz((uint32_t)K);  // planes that can be set
  }
  auto value = [&](int bit) -> float {
    if constexpr (MODE == FJCOMP_VOTE_SIGN) {
      const uint32_t one = 0x3f800000u | (((neg >> bit) & 1u) << 31);
      return __uint_as_float(((tie >> bit) & 1u) ? 0u : one);
    } else {
      uint32_t cnt = 0u;
#pragma unroll
      for (int j = 0; j < kPlanes; ++j)
        if (j < np) cnt |= ((c[j] >> bit) & 1u) << j;
      return __fmul_rn((float)(K - 2 * (int)cnt), scale);
    }
  };
  float* __restrict__ o = out_ptrs[l] + e0;
  if (left >= 32 && ((uintptr_t)o & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      reinterpret_cast<float4*>(o)[q] = float4{value(4 * q), value(4 * q + 1), value(4 * q + 2), value(4 * q + 3)};
    return;
  }
#pragma unroll
  for (int bit = 0; bit < 32; ++bit)
    if (bit < left) o[bit] = value(bit);
}

// The encoder: a lane reads 8 consecutive floats of one row and stores their byte whole, so every
// byte has exactly one writer. x < 0 is false for NaN and both zeros; elements past the row read
// as 0, so the padding bits are written as 0.
__global__ __launch_bounds__(kPackThreads) void k_sign_pack(const float* const* __restrict__ in_ptrs, int64_t R,
                                                            const int64_t* __restrict__ row_n,
                                                            const int64_t* __restrict__ prefix,
                                                            uint8_t* const* __restrict__ sign_ptrs) {
  const int64_t b = blockIdx.x;
  const int64_t r = find_segment(prefix, R, b);
  const int64_t n = row_n[r];
  const int64_t i0 = 8 * ((b - prefix[r]) * kPackThreads + threadIdx.x);
  if (i0 >= n) return;
  const float* __restrict__ x = in_ptrs[r];
  uint32_t byte = 0u;
  if (i0 + 8 <= n && ((uintptr_t)x & 15) == 0) {
    const float4 q0 = *reinterpret_cast<const float4*>(x + i0);
    const float4 q1 = *reinterpret_cast<const float4*>(x + i0 + 4);
    const float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int u = 0; u < 8; ++u) byte |= (v[u] < 0.0f ? 1u : 0u) << u;
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + u < n) byte |= (x[i0 + u] < 0.0f ? 1u : 0u) << u;
  }
  sign_ptrs[r][i0 >> 3] = (uint8_t)byte;
}

int check_launch(const char* kernel) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse(FJAGG_EHIP, "%s: %s", kernel, hipGetErrorString(e));
  return FJAGG_OK;
}

}  // namespace

extern "C" {

int fjcomp_sign_pack(const float* const* in_ptrs, int64_t R, const int64_t* row_n, const int64_t* block_prefix,
                     int64_t nblocks, uint8_t* const* sign_ptrs, void* stream) {
  const char* what = "sign_pack";
  if (R < 1) return refuse(FJAGG_EINVAL, "%s: R must be >= 1 (got %lld)", what, (long long)R);
  if (nblocks < 0 || nblocks > 0x7fffffffll)
    return refuse(FJAGG_EINVAL, "%s: nblocks must be in [0, 2^31) (got %lld)", what, (long long)nblocks);
  if (!in_ptrs || !row_n || !block_prefix || !sign_ptrs) return refuse(FJAGG_EINVAL, "%s: null table", what);
  if (nblocks == 0) return FJAGG_OK;
  hipLaunchKernelGGL(k_sign_pack, dim3((unsigned)nblocks), dim3(kPackThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     in_ptrs, R, row_n, block_prefix, sign_ptrs);
  return check_launch("k_sign_pack");
}

int fjcomp_sign_vote(const uint8_t* const* bit_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                     const int64_t* block_prefix, int64_t nblocks, int mode, float scale, float* const* out_ptrs,
                     void* stream) {
  const char* what = "sign_vote";
  if (K < 1) return refuse(FJAGG_EINVAL, "%s: K must be >= 1 (got %lld)", what, (long long)K);
  if (K > FJCOMP_VOTE_MAX_CLIENTS)
    return refuse(FJAGG_EUNSUPPORTED, "%s: K <= %d clients (got %lld)", what, FJCOMP_VOTE_MAX_CLIENTS, (long long)K);
  if (L < 1) return refuse(FJAGG_EINVAL, "%s: L must be >= 1 (got %lld)", what, (long long)L);
  if (mode != FJCOMP_VOTE_SIGN && mode != FJCOMP_VOTE_MEAN)
    return refuse(FJAGG_EINVAL, "%s: mode must be FJCOMP_VOTE_SIGN or FJCOMP_VOTE_MEAN (got %d)", what, mode);
  if (nblocks < 0 || nblocks > 0x7fffffffll)
    return refuse(FJAGG_EINVAL, "%s: nblocks must be in [0, 2^31) (got %lld)", what, (long long)nblocks);
  if (!bit_ptrs || !leaf_n || !block_prefix || !out_ptrs) return refuse(FJAGG_EINVAL, "%s: null table", what);
  if (nblocks == 0) return FJAGG_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (mode == FJCOMP_VOTE_SIGN)
    hipLaunchKernelGGL(k_sign_vote<FJCOMP_VOTE_SIGN>, dim3((unsigned)nblocks), dim3(kThreads), 0, s, bit_ptrs, (int)K, L,
                       leaf_n, block_prefix, scale, out_ptrs);
  else
    hipLaunchKernelGGL(k_sign_vote<FJCOMP_VOTE_MEAN>, dim3((unsigned)nblocks), dim3(kThreads), 0, s, bit_ptrs, (int)K, L,
                       leaf_n, block_prefix, scale, out_ptrs);
  return check_launch("k_sign_vote");
}

}  // extern "C"
