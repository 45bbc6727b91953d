/* fjcomp.h — C ABI of the compression-aggregator kernels (libfjagg.so).
 *
 * FedJAX's compression aggregators (fedjax/aggregators/compression.py) quantize
 * every client delta with jax.random draws, optionally inside a randomized
 * Walsh-Hadamard rotation (fedjax/aggregators/walsh_hadamard.py), and feed the
 * results to tree_mean. In the reference each step is a jax.jit dispatch per
 * client per leaf; here the steps are a handful of launches per round over
 * device-resident (client, leaf) tables:
 *
 *   fjcomp_row_stats      jnp.amin / amax / std and the DRIVE sums per (client, leaf)
 *                         compression.py:58-61,84-87,331,275
 *   fjcomp_quant_fold     uniform_stochastic_quantize / terngrad_quantize with the
 *                         jax.random.uniform draw, fused with tree_mean's fold
 *                         compression.py:66-97,323-336 + tree_util.py:76-96
 *   fjcomp_rademacher     jax.random.rademacher signs, bit-packed
 *                         walsh_hadamard.py:148,170
 *   fjcomp_wht            walsh_hadamard_transform with the structured_rotation /
 *                         inverse_structured_rotation (and DRIVE) pre/epilogues
 *                         walsh_hadamard.py:25-176, compression.py:269-277
 *   fjcomp_sign_pack      signSGD's client: one sign bit per coordinate, bit-packed
 *   fjcomp_sign_vote      signSGD with majority vote (Bernstein et al., ICLR 2019): the sign the
 *                         majority of the clients sent, or the mean of the signs, from bit-sliced
 *                         integer counts
 *   fjcomp_random_bits / fjcomp_uniform   jax.random.bits / uniform of one key
 *   fjcomp_normal / fjcomp_normal_from_bits   jax.random.normal of one key; its bits -> z map
 *
 * Randomness is jax.random's threefry2x32 (non-partitionable counter layout) and
 * haiku.PRNGSequence; the key schedule runs on the host (fjcomp_random_split,
 * fjcomp_prng_sequence), the draws on the device. All device pointers; all
 * launches are asynchronous on the given hipStream_t. Return 0 or FJAGG_E*;
 * fjagg_last_error() has the message. Table layouts are fixed (static_assert'd
 * in fjcomp.hip) so hosts can build them as plain structured arrays.
 */
#ifndef FJCOMP_H_
#define FJCOMP_H_

#include <stdint.h>

#include "fjagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FJCOMP_ABI_VERSION 1

/* fjcomp_quant_fold methods */
#define FJCOMP_UNIFORM 1  /* uniform_stochastic_quantize, compression.py:66-97 */
#define FJCOMP_TERNGRAD 2 /* terngrad_quantize, compression.py:323-336 */
#define FJCOMP_BINARY 3   /* binary_stochastic_quantize, compression.py:43-63 */

/* fjcomp_wht job kinds */
#define FJCOMP_WHT_PLAIN 0          /* y = H x                                   walsh_hadamard.py:25-98 */
#define FJCOMP_WHT_ROTATE 1         /* y = H(pad(x) * D) / sqrt(d)               walsh_hadamard.py:127-148 */
#define FJCOMP_WHT_UNROTATE 2       /* y = (H x * D) / sqrt(d), first n_out      walsh_hadamard.py:151-176 */
#define FJCOMP_WHT_UNROTATE_DRIVE 3 /* x -> (A sign(x)) / B, then UNROTATE       compression.py:269-277 */

#define FJCOMP_WHT_MAX_LOG2 34 /* 2^34 floats; 13 + 8 + 8 + 8 bits: four passes */

/* per-row statistics (f64 accumulation, fixed combine order) */
typedef struct fjcomp_stats {
  double min, max;   /* NaN-propagating, like lax.min/max */
  double absmax;
  double sum, sumsq, sumabs;
} fjcomp_stats;

/* per-row quantizer parameters derived from fjcomp_stats by fjcomp_row_stats */
typedef struct fjcomp_qparams {
  float vmin, vmax; /* UNIFORM / BINARY: amin, amax. TERNGRAD: 0, amax(|clip(v)|) */
  float range;      /* vmax - vmin (f32) */
  float thr;        /* TERNGRAD: f32(2.5 * std) clip threshold; unused otherwise */
  double rcp_range; /* 1 / (double)range: correctly rounded f32 quotients, see fjcomp.hip */
} fjcomp_qparams;

typedef struct fjcomp_row {
  const float* ptr;
  int64_t n;
} fjcomp_row;

typedef struct fjcomp_sign_job {
  uint32_t key[2];
  int64_t d;        /* number of signs */
  uint32_t* words;  /* ceil(d / 32) words; bit (g % 32) of word g / 32 set <=> sign -1 */
} fjcomp_sign_job;

typedef struct fjcomp_wht_job {
  const float* src;           /* pass 0 input */
  float* mid;                 /* intermediate of a multi-pass job (d floats; may alias src) */
  float* dst;                 /* last-pass output, n_out floats */
  const uint32_t* signs;      /* ROTATE / UNROTATE*: d sign bits (fjcomp_rademacher) */
  const fjcomp_stats* stats;  /* UNROTATE_DRIVE: sumsq / sumabs of src. ROTATE: optional (may be NULL) per-tile
                                 partials of dst for fjcomp_stats_combine (min / max / |max|, and with
                                 FJCOMP_WHT_F_SUMS sumsq / sumabs in f64), one slot of
                                 fjcomp_row_stats_workspace_bytes(1) B per last-pass tile */
  int64_t n_in;               /* valid src elements (ROTATE zero-pads to d) */
  int64_t n_out;              /* elements written to dst (<= d) */
  int32_t log2d;
  int32_t kind;
  float sqrt_d;               /* f32(sqrt(d)), correctly rounded */
  int32_t flags;              /* ROTATE with stats: FJCOMP_WHT_F_SUMS also accumulates sumsq / sumabs */
} fjcomp_wht_job;
#define FJCOMP_WHT_F_SUMS 1

int fjcomp_abi_version(void);

/* ---- host key algebra (no device work) ---- */
/* Threefry-2x32-20 of n counter pairs. */
int fjcomp_threefry2x32(const uint32_t key[2], const uint32_t* x0, const uint32_t* x1, int64_t n,
                        uint32_t* y0, uint32_t* y1);
/* jax.random.split of each of nkeys keys into num: out[nkeys][num][2]. */
int fjcomp_random_split(const uint32_t* keys, int64_t nkeys, int64_t num, uint32_t* out);
/* n draws of haiku.PRNGSequence(key): key (in/out) advances, subkeys[n][2]. */
int fjcomp_prng_sequence(uint32_t key[2], int64_t n, uint32_t* subkeys);

/* ---- device ---- */
/* jax.random.bits(key, (n,), uint32) / jax.random.uniform(key, (n,), float32). */
int fjcomp_random_bits(uint32_t k0, uint32_t k1, int64_t n, uint32_t* out, void* stream);
int fjcomp_uniform(uint32_t k0, uint32_t k1, int64_t n, float* out, void* stream);
/* jax.random.normal(key, (n,), float32) (jax/_src/random.py, _normal_real): the bits of
 * fjcomp_random_bits, b -> f = bitcast((b >> 9) | 0x3f800000) - 1, the uniform on (-1, 1)
 *   u = max(lo, fl(fl(f * 2) + lo)),  lo = nextafter(-1f, 0f)   (fl(1 - lo) = 2 exactly)
 * and z = sqrt(2) * erfinv(u). The bits and u are jax's; the last step is evaluated in f64
 * (the device erfinv) and rounded once to f32, not XLA's f32 erf_inv polynomial. u is never
 * +-1, so every z is finite. 0 <= n < 2^32. The DP clipped folds (fjagg_wsum_clip_noise_*,
 * fjagg.h) draw exactly these values per leaf. */
int fjcomp_normal(const uint32_t key[2], int64_t n, float* out_dev, void* stream);
/* The bits -> z map of fjcomp_normal alone over n given words: fjcomp_normal is
 * fjcomp_random_bits followed by exactly this. */
int fjcomp_normal_from_bits(const uint32_t* bits_dev, int64_t n, float* out_dev, void* stream);

/* Bit-packed jax.random.rademacher(key, (d,)) for J jobs. A workgroup takes block_pairs
 * (a multiple of 256, at most FJCOMP_SIGN_BLOCK_PAIRS) consecutive element pairs of one job:
 * block_prefix[J+1] (device) is the running sum of ceil(ceil(d/2) / block_pairs) over jobs,
 * nblocks its last entry. Large blocks amortise the per-workgroup setup; small ones fill the
 * chip when there are few pairs in total. */
#define FJCOMP_SIGN_BLOCK_PAIRS 8192
int fjcomp_rademacher(const fjcomp_sign_job* jobs, const int64_t* block_prefix, int64_t J,
                      int64_t nblocks, int block_pairs, void* stream);

/* Statistics of R rows (f32). chunk_prefix[R+1] (device): running sum of
 * max(1, ceil(n / FJCOMP_STATS_CHUNK)); nchunks its last entry. Writes stats[R] and, when
 * method is FJCOMP_UNIFORM, FJCOMP_BINARY or FJCOMP_TERNGRAD, qparams[R] (may be NULL).
 * TERNGRAD's sigma comes from the f64 sums of x - x[0] (no cancellation against the mean);
 * the sum and sumsq reported for such a call are recovered from those.
 * Workspace: fjcomp_row_stats_workspace_bytes(nchunks). */
#define FJCOMP_STATS_CHUNK 16384
int64_t fjcomp_row_stats_workspace_bytes(int64_t nchunks);
/* Statistics and (qparams != NULL) UNIFORM / BINARY qparams of R rows from per-tile
 * partials written by fjcomp_wht (ROTATE jobs with a stats pointer): row r owns partials
 * part_prefix[r] .. part_prefix[r+1]-1 (device). min / max / |max| equal fjcomp_row_stats';
 * sumsq / sumabs (FJCOMP_WHT_F_SUMS) are f64 sums in tile order, sum is 0. */
int fjcomp_stats_combine(const fjcomp_row* rows, const int64_t* part_prefix, int64_t R, int method,
                         const void* part, fjcomp_stats* stats, fjcomp_qparams* qparams, void* stream);
int fjcomp_row_stats(const fjcomp_row* rows, const int64_t* chunk_prefix, int64_t R, int64_t nchunks,
                     int method, fjcomp_stats* stats, fjcomp_qparams* qparams, void* ws,
                     int64_t ws_bytes, void* stream);

/* Quantize K clients x L leaves and fold them in client order (tree_mean):
 *   q = Q(x[k][l], key[k][l], qparams[k][l]);  s = (k == 0 && !ACCUMULATE) ? fl(q*w_k) : fl(s + fl(q*w_k))
 *   out[l] = SCALE ? fl(s * scale) : s
 * in_ptrs[K*L] (client-major), keys[K*L][2], qparams[K*L], w[K] f32, out_ptrs[L],
 * leaf_n[L], block_prefix[L+1] (running sum of ceil(ceil(n/2) / 256)). For
 * FJCOMP_UNIFORM, hist (optional, int32 [K*L][num_levels + 1], zeroed by the caller)
 * receives per-row counts of the quantization level index (bin num_levels: non-finite). */
int fjcomp_quant_fold(int method, const float* const* in_ptrs, const uint32_t* keys,
                      const fjcomp_qparams* qparams, const float* w, int64_t K, int64_t L,
                      const int64_t* leaf_n, const int64_t* block_prefix, int64_t nblocks,
                      int num_levels, float scale, int flags, float* const* out_ptrs, int32_t* hist,
                      void* stream);

/* ---- uniform quantizer, transmitted form: 8-bit level codes ----
 * For 2 <= num_levels <= 256 a (client, leaf) row of n elements is n uint8 codes c < num_levels
 * and the float32 pair (vmin, vmax). With top = num_levels - 1 and range = fl(vmax - vmin) a code
 * decodes to exactly the value fjcomp_quant_fold's UNIFORM operator folds:
 *   q(c) = fl(vmin + fl(lev[min(c, top)] * range)),   lev[j] = RN_f32(j / top)
 * (two roundings, no multiply-add; non-finite vmin / range propagate; a code above top counts as
 * top). A workgroup takes block_codes consecutive codes (fold: FJCOMP_CODES_BLOCK, or
 * FJCOMP_CODES_BLOCK_SMALL when the larger share would leave most of the chip idle; same bits)
 * or FJCOMP_CODES_BLOCK element pairs (encode) of one row.
 *
 * fjcomp_codes_fold: tree_mean straight from the codes, one launch, no decoded temporary:
 *   s = fl(q_0 * w_0);  s = fl(s + fl(q_k * w_k)) in client order;  out[l] = SCALE ? fl(s * scale) : s
 * code_ptrs[K*L] (client-major, any alignment), minmax[K*L][2], w[K], leaf_n[L] (0 allowed),
 * block_prefix[L+1] the running sum of ceil(leaf_n / block_codes) and nblocks its last
 * entry, out_ptrs[L]: all device. flags: FJAGG_SCALE only.
 *
 * fjcomp_encode_uniform: rows in_ptrs[R] of row_n[R] >= 1 floats with keys[R][2] and the
 * qparams[R] of fjcomp_row_stats (UNIFORM) become codes at code_ptrs[R] and minmax[R][2], with
 * fjcomp_quant_fold's draws and decisions: folding the codes gives that call's bits.
 * block_prefix[R+1] is the running sum of ceil(ceil(row_n / 2) / FJCOMP_CODES_BLOCK). */
#define FJCOMP_CODES_BLOCK 4096
#define FJCOMP_CODES_BLOCK_SMALL 1024
int fjcomp_codes_fold(const uint8_t* const* code_ptrs, const float* minmax, const float* w, int64_t K, int64_t L,
                      const int64_t* leaf_n, const int64_t* block_prefix, int64_t nblocks, int block_codes,
                      int num_levels, float scale, int flags, float* const* out_ptrs, void* stream);
int fjcomp_encode_uniform(const float* const* in_ptrs, const uint32_t* keys, const fjcomp_qparams* qparams,
                          int64_t R, const int64_t* row_n, const int64_t* block_prefix, int64_t nblocks,
                          int num_levels, uint8_t* const* code_ptrs, float* minmax, void* stream);

/* ---- the same form with bits = 1, 2 or 4 per code (2^bits >= num_levels) ----
 * Element i of a row lives in byte i / (8 / bits) at bit offset bits * (i % (8 / bits)), low bits
 * first; a row of n elements is ceil(n * bits / 8) bytes, and the unused high bits of its last
 * byte influence nothing (the encoder writes them as 0). A field >= num_levels counts as top.
 *
 * fjcomp_codes_fold_packed: fjcomp_codes_fold's sums, bit for bit, from packed rows. A workgroup
 * takes block_codes consecutive elements (FJCOMP_PACKED_BLOCK, or FJCOMP_PACKED_BLOCK_SMALL when
 * the larger share would leave most of the chip idle; same bits); leaf_n counts elements and
 * block_prefix is the running sum of ceil(leaf_n / block_codes).
 *
 * fjcomp_encode_uniform_packed: fjcomp_encode_uniform's decisions, written as the packing of
 * its codes, every output byte stored whole by exactly one lane (no atomics, no cleared
 * buffer). block_prefix as for fjcomp_encode_uniform. */
#define FJCOMP_PACKED_BLOCK 4096
#define FJCOMP_PACKED_BLOCK_SMALL 2048
int fjcomp_codes_fold_packed(const uint8_t* const* code_ptrs, const float* minmax, const float* w, int64_t K,
                             int64_t L, const int64_t* leaf_n, const int64_t* block_prefix, int64_t nblocks,
                             int block_codes, int bits, int num_levels, float scale, int flags,
                             float* const* out_ptrs, void* stream);
int fjcomp_encode_uniform_packed(const float* const* in_ptrs, const uint32_t* keys, const fjcomp_qparams* qparams,
                                 int64_t R, const int64_t* row_n, const int64_t* block_prefix, int64_t nblocks,
                                 int bits, int num_levels, uint8_t* const* code_ptrs, float* minmax, void* stream);

/* Walsh-Hadamard jobs. pass_prefix[npass][J+1] (device): per pass, the running sum of
 * that job's tiles in the pass (0 if the job has fewer passes); pass_tiles[npass] (host):
 * the totals. A job of d = 2^log2d has one pass for log2d <= 13, else
 * 1 + ceil((log2d - 13) / 8) (pass 0: bits 0..12; pass p >= 1: the next 8 bits). */
int fjcomp_wht(const fjcomp_wht_job* jobs, const int64_t* pass_prefix, int64_t J, int npass,
               const int64_t* pass_tiles, void* stream);

/* tiles of pass p for a job of 2^log2d (host helper, mirrors the kernel's tiling) */
int64_t fjcomp_wht_tiles(int log2d, int pass);

/* ---- DRIVE's transmitted form: sign bits + (sum y^2, sum |y|) per leaf ----
 * A client sends, per leaf, the d = 2^log2d sign bits of its rotated leaf (coordinate i in byte
 * i / 8 at bit i % 8, 1 <=> negative; ceil(d / 8) bytes, padding bits of d < 8 ignored) and
 * scales = (A, b) = (f32(sum y^2), f32(sum |y|)). Sign s stands for (A * s) / b, the value
 * FJCOMP_WHT_UNROTATE_DRIVE loads.
 *
 * fjcomp_drive_pack: the client's side. Row r (ptr: its rotated leaf, n = d floats) becomes
 * d sign bits at sign_ptrs[r], every byte stored whole by one lane, and scales[2r .. 2r+1] from
 * stats[r]. block_prefix: running sum of ceil(d / FJCOMP_DRIVE_PACK_BLOCK).
 *
 * fjcomp_drive_pass: pass `pass` (not the last) of the inverse transforms of kb clients' leaves
 * with more than one pass, into / in place on ws[kb][D] (leaf l at ws_off). tile_prefix[L + 1]:
 * running sum of fjcomp_wht_tiles(log2d, pass), 0 for a leaf whose last pass is <= pass; the
 * grid is kb * tiles. Pass 0 reads the sign bits, later passes the workspace.
 *
 * fjcomp_drive_fold: the last pass with tree_mean's fold in its epilogue. One workgroup per
 * (leaf, last-pass tile) walks the kb clients in order: tile from the sign bits (single != 0:
 * leaves of one pass, tile_prefix counts 1 per such leaf and 0 otherwise) or from ws (single == 0:
 * the others), butterflies, * Rademacher sign, / sqrt(d), fl(z * w_k) added in client order into
 * registers. FJAGG_ACCUMULATE starts from out, FJAGG_SCALE multiplies by scale at the end. Only
 * the leaf's first n coordinates are written. Bits: k_wht's UNROTATE_DRIVE + the dense fold's. */
typedef struct fjcomp_drive_leaf {
  float* out;      /* n floats */
  int64_t n;       /* elements of the leaf (<= d) */
  int64_t ws_off;  /* multi-pass leaf: its offset (floats) in a client's workspace row */
  int32_t log2d;
  float sqrt_d;    /* f32(sqrt(d)), correctly rounded */
} fjcomp_drive_leaf;
#define FJCOMP_DRIVE_PACK_BLOCK 2048
int fjcomp_drive_pack(const fjcomp_row* rows, const int64_t* block_prefix, int64_t R, int64_t nblocks,
                      const fjcomp_stats* stats, uint8_t* const* sign_ptrs, float* scales, void* stream);
int fjcomp_drive_pass(const fjcomp_drive_leaf* leaves, const int64_t* tile_prefix, int64_t L, int64_t tiles,
                      int pass, const uint8_t* const* bit_ptrs, const float* scales, int64_t kb, float* ws,
                      int64_t D, void* stream);
int fjcomp_drive_fold(const fjcomp_drive_leaf* leaves, const int64_t* tile_prefix, int64_t L, int64_t tiles,
                      int single, const uint8_t* const* bit_ptrs, const uint32_t* const* sign_ptrs,
                      const float* scales, const float* w, int64_t kb, const float* ws, int64_t D, float scale,
                      int flags, void* stream);

/* ---- top-k sparsified mean (fjsparse.hip) ----
 * Client k's row is its leaves back to back, P float32 elements. With the magnitude key
 * m(v) = bits(v) & 0x7fffffff compared as uint32 (|NaN| > inf > finite > subnormal > 0: a NaN is
 * kept first; this is compression, not robustness), T_k is the c-th largest key of row k, exact,
 * and coordinate i of client k is kept iff m(x_k[i]) >= T_k: all ties at the threshold are kept.
 *   thresholds[k] = T_k's bits as a float;   sent[k] = #{i : m(x_k[i]) >= max(T_k, 1)}
 *   x~ = kept ? x : +0;  s = fl(x~_0 w_0);  s = fl(s + fl(x~_k w_k));  out = fl(s * scale)
 * the multiply and the add separate, in client order: fjagg_wsum_dense's exact fold over x~.
 * The selection is a three-level radix select over integer histograms (fjsparse_dev.h), so
 * thresholds and sent do not depend on the order of its atomics. float32 only, 1 <= K <=
 * FJCOMP_TOPK_MAX_CLIENTS, P < 2^31, 1 <= c <= P; P == 0 launches nothing. All launches are
 * asynchronous on `stream`, nothing visits the host, and the workspace
 * (fjcomp_topk_workspace_bytes(K) bytes, any contents) is zeroed on the stream by the call.
 *
 * _dense: rows x + k * ld (elements). _ptrs: in_ptrs[K*L] client-major and leaf_n[L] as in
 * fjcomp_quant_fold, chunk_prefix[L+1] the running sum of ceil(leaf_n / FJCOMP_TOPK_CHUNK) and
 * nchunks its last entry (all device), P the sum of leaf_n; one histogram per client spans all
 * its leaves. flags: FJAGG_UNALIGNED unless every in_ptrs and out_ptrs entry is 16-byte aligned.
 * _select: thresholds and sent alone. _mean: the selection, then the masked fold with w[K]. */
#define FJCOMP_TOPK_CHUNK 16384
#define FJCOMP_TOPK_MAX_CLIENTS 4096
int64_t fjcomp_topk_workspace_bytes(int64_t K);
int fjcomp_topk_select_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t c,
                             float* thresholds_dev, int32_t* sent_dev, void* ws_dev, int64_t ws_bytes, void* stream);
int fjcomp_topk_select_ptrs(int in_dtype, const float* const* in_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                            const int64_t* chunk_prefix, int64_t nchunks, int64_t P, int64_t c, float* thresholds_dev,
                            int32_t* sent_dev, void* ws_dev, int64_t ws_bytes, int flags, void* stream);
int fjcomp_topk_mean_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t c,
                           const float* w_dev, float scale, float* out_dev, float* thresholds_dev, int32_t* sent_dev,
                           void* ws_dev, int64_t ws_bytes, void* stream);
int fjcomp_topk_mean_ptrs(int in_dtype, const float* const* in_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                          const int64_t* chunk_prefix, int64_t nchunks, int64_t P, int64_t c, const float* w_dev,
                          float scale, float* const* out_ptrs, float* thresholds_dev, int32_t* sent_dev, void* ws_dev,
                          int64_t ws_bytes, int flags, void* stream);

/* ---- top-k's transmitted form: sorted (index, value) lists ----
 * A top-k client sends the coordinates it keeps, those with m(x) >= max(T_k, 1) (zeros are never
 * sent), as n = sent[k] pairs: indices, int32, strictly increasing, an index counting the elements
 * of the client's row as above (the leaves back to back); and values, float32, the elements
 * verbatim.
 *
 * fjcomp_topk_compact_dense / _ptrs: the client's side, rows addressed as in fjcomp_topk_select_*
 * and thresholds_dev from that call. Order-preserving stream compaction in three launches (the
 * kept elements of every FJCOMP_TOPK_CHUNK chunk; one scan of the chunk counts per row; a write
 * pass that ranks the kept elements with wave ballots), ordered by the launch boundaries alone.
 * Row k's pairs go to indices_dev / values_dev at offsets_dev[k] .. offsets_dev[k + 1]
 * (int64 [K + 1], device: the running sum of sent). Every offset is clamped into [0, capacity]
 * before it forms an address and a row writes no slot at or past its end, so a table that
 * disagrees with the thresholds truncates rows but never writes outside the capacity elements
 * of either output. Two calls write the same bytes. The workspace
 * (fjcomp_topk_compact_workspace_bytes(K, nchunks) bytes, nchunks = ceil(P / FJCOMP_TOPK_CHUNK) for
 * _dense) needs no initialisation. P == 0 or capacity == 0 launches nothing.
 *
 * fjcomp_sparse_fold: the server's side, tree_mean from K such lists in one launch with no
 * workspace and no host step. idx_ptrs[K], val_ptrs[K] and counts[K] (int64) are device tables,
 * w_dev[K] the float32 weights, out_dev flat float[P] (every element is written). Per coordinate
 *   s = +0;  for every client that sent it, in client order: s = fl(s + fl(v * w_k));
 *   out = fl(s * scale)
 * the multiply and the add separate. For finite weights this is the masked fold of
 * fjcomp_topk_mean_* over the same clients, bit for bit wherever the result is not a zero. It
 * yields +0 in the one place the masked fold can yield -0: every term of the coordinate is a zero
 * and the first of them is -0. The output is partitioned (a workgroup owns
 * FJCOMP_SPARSE_GROUP_TILE coordinates, each of its four waves FJCOMP_SPARSE_WAVE_TILE of them in
 * LDS), so there are no atomics on the result and two calls give the same bits. An entry is
 * applied only if its index lies in the tile being formed: an index outside [0, P) is ignored,
 * an unsorted list gives an unspecified but in-bounds result, and a count is clamped to [0, P].
 * 1 <= K <= FJCOMP_TOPK_MAX_CLIENTS, P < 2^31, flags must be 0. */
#define FJCOMP_SPARSE_WAVE_TILE 1024
#define FJCOMP_SPARSE_GROUP_TILE 4096
int64_t fjcomp_topk_compact_workspace_bytes(int64_t K, int64_t nchunks);
int fjcomp_topk_compact_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                              const float* thresholds_dev, const int64_t* offsets_dev, int64_t capacity,
                              int32_t* indices_dev, float* values_dev, void* ws_dev, int64_t ws_bytes, void* stream);
int fjcomp_topk_compact_ptrs(int in_dtype, const float* const* in_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                             const int64_t* chunk_prefix, int64_t nchunks, int64_t P, const float* thresholds_dev,
                             const int64_t* offsets_dev, int64_t capacity, int32_t* indices_dev, float* values_dev,
                             void* ws_dev, int64_t ws_bytes, int flags, void* stream);
int fjcomp_sparse_fold(const int32_t* const* idx_ptrs, const float* const* val_ptrs, const int64_t* counts, int64_t K,
                       int64_t P, const float* w_dev, float scale, float* out_dev, int flags, void* stream);

/* ---- signSGD with majority vote: one sign bit per coordinate (fjsignvote.hip) ----
 * A client sends, per leaf of n elements, ceil(n / 8) bytes: coordinate i in byte i / 8 at bit
 * i % 8, low bit first (the 1-bit packing above), 1 <=> the value is < 0 (+0, -0 and NaN are
 * sent as 0). The encoder writes the padding bits of a last byte as 0; the server ignores them.
 *
 * fjcomp_sign_pack: the client's side. Row r (in_ptrs[r], row_n[r] float32 elements, 0 allowed)
 * becomes its sign bits at sign_ptrs[r], every byte stored whole by exactly one lane.
 * block_prefix[R+1] is the running sum of ceil(row_n / FJCOMP_SIGN_PACK_BLOCK), nblocks its last
 * entry; all tables device. R >= 1.
 *
 * fjcomp_sign_vote: the server's side, one launch, integer until the last instruction. With c
 * the number of the K clients whose bit is 1, per coordinate
 *   FJCOMP_VOTE_SIGN   out = -1 if 2c > K,  +1 if 2c < K,  +0 if 2c == K
 *   FJCOMP_VOTE_MEAN   out = fl(f32(K - 2c) * scale)   (the mean of the signs for scale = f32(1 / K))
 * bit_ptrs[K*L] (client-major, any alignment), leaf_n[L] elements (0 allowed), block_prefix[L+1]
 * the running sum of ceil(leaf_n / FJCOMP_VOTE_TILE) and nblocks its last entry, out_ptrs[L]
 * (float32, 4-byte aligned): all device. A workgroup owns FJCOMP_VOTE_TILE coordinates of one
 * leaf and keeps their counts bit-sliced; the clients are split over its four waves and the
 * partial counts added as integers, so there are no atomics and two calls give the same bits.
 * No byte past a packed leaf's last is read and no output past leaf_n is written.
 * 1 <= K <= FJCOMP_VOTE_MAX_CLIENTS (above: FJAGG_EUNSUPPORTED), L >= 1. */
#define FJCOMP_VOTE_SIGN 0
#define FJCOMP_VOTE_MEAN 1
#define FJCOMP_VOTE_TILE 8192
#define FJCOMP_VOTE_MAX_CLIENTS 4096
#define FJCOMP_SIGN_PACK_BLOCK 2048
int fjcomp_sign_pack(const float* const* in_ptrs, int64_t R, const int64_t* row_n, const int64_t* block_prefix,
                     int64_t nblocks, uint8_t* const* sign_ptrs, void* stream);
int fjcomp_sign_vote(const uint8_t* const* bit_ptrs, int64_t K, int64_t L, const int64_t* leaf_n,
                     const int64_t* block_prefix, int64_t nblocks, int mode, float scale, float* const* out_ptrs,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FJCOMP_H_ */
