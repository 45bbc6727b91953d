/*
 * fjagg.h — C ABI of the MI355X-native FedJAX aggregation library (libfjagg.so).
 *
 * This library replaces the arithmetic of FedJAX's server-side client-update
 * aggregation, i.e. the weighted fold that `fedjax.tree_util.tree_mean` performs
 * over K client-delta pytrees:
 *
 *     reference                                   replaced by
 *     ------------------------------------------  ---------------------------------
 *     tree_weight   fedjax/core/tree_util.py:29-32  fjagg_wsum_* (per-client multiply)
 *     _tree_add_eq  fedjax/core/tree_util.py:47-54  fjagg_wsum_* (fused running add)
 *     _tree_inverse_weight_eq  tree_util.py:58-61   fjagg_wsum_* with FJAGG_SCALE
 *     tree_mean loop tree_util.py:76-96             one fjagg_wsum_* launch per bucket
 *     tree_sum       tree_util.py:64-73             fjagg_wsum_* with unit weights
 *     tree_add       tree_util.py:47-50             fjagg_wsum_* K=2, unit weights
 *     tree_l2_squared tree_util.py:105-108          fjagg_l2sq_*
 *     tree_clip_by_global_norm tree_util.py:117-133 fjagg_clip_scales + fjagg_wsum_clip_*
 *     expectation_step algorithms/hyp_cluster.py:268-303  fjagg_wsum_group_* (per-cluster means)
 *     per-cluster apply algorithms/hyp_cluster.py:107-128 fjagg_server_update_group_* (means + steps)
 *     clipped round algorithms/mime_lite.py:131-149,162-167 fjagg_server_update_clip_* (clipped mean + step)
 *     (no reference row) DP-FedAvg's Gaussian mechanism      fjagg_wsum_clip_noise_* (clipped mean + noise)
 *     (no reference row) trimmed mean / median (Yin et al. 2018) fjagg_trim_* (order statistics per coordinate)
 *     (no reference row) Krum / geometric median (Gram matrix)  fjagg_gram_* (K x K inner products, float64)
 *     (no reference row) Krum / Weiszfeld selection on the device fjagg_krum_select, fjagg_weiszfeld_select
 *     (no reference row) mean around the median / Bulyan        fjagg_meamed_* (the keep values nearest the median)
 *     (no reference row) Bulyan on the device                   fjagg_bulyan_select, fjagg_meamed_*_dev
 *     (no reference row) centered clipping (Karimireddy et al. 2021) fjagg_center_* (clipped around the last aggregate)
 *     (no reference row) FLTrust (Cao et al. 2021)              fjagg_dotsq_*, fjagg_fltrust_* (trust-weighted mean against a server delta)
 *
 * The reference has no native code: each of those rows is a `jax.jit` dispatch
 * into XLA. The Python mirror of the reference's API
 * (fedjax_amd/tree_util.py, fedjax_amd/aggregators/) is the only caller inside
 * this repository; INTEGRATION.md shows the ctypes binding a FedJAX maintainer
 * would add.
 *
 * Conventions
 *   - every entry point returns 0 on success or a negative FJAGG_E* code; the
 *     message of the last failure on the calling thread is fjagg_last_error().
 *   - every launch is asynchronous on the given hipStream_t (passed as void*;
 *     NULL = the null stream). No entry point allocates, frees or synchronises,
 *     so launches may be captured into a hipGraph.
 *   - pointers named *_dev are device pointers; everything else is host memory.
 *   - inputs are never written (reference ownership rule, tree_util_test.py:50-51).
 *
 * Arithmetic contract (FJAGG_MODE_EXACT, the default): for every element p
 *     t_k = fl(x_k[p] * w_k)            (IEEE single, round to nearest, no FMA)
 *     s_0 = t_0                          (s_0 = fl(out[p] + t_0) with FJAGG_ACCUMULATE)
 *     s_k = fl(s_{k-1} + t_k)            k = 1 .. K-1, in client order
 *     out[p] = fl(s_{K-1} * scale)       with FJAGG_SCALE, else s_{K-1}
 * which is bit-for-bit the sequence XLA executes for tree_mean.
 * FJAGG_MODE_SPLIT folds contiguous client ranges independently and combines
 * the range sums in range order: not bitwise, within the bound in DESIGN.md.
 */
#ifndef FJAGG_H_
#define FJAGG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FJAGG_ABI_VERSION 4

/* element types */
enum fjagg_dtype {
  FJAGG_F32 = 0,   /* IEEE binary32 */
  FJAGG_BF16 = 1,  /* bfloat16 (stored as uint16) */
  FJAGG_I32 = 2,   /* two's complement int32, wrapping arithmetic like XLA */
};

/* flags (bitwise OR) */
enum fjagg_flags {
  FJAGG_SCALE = 1 << 0,       /* multiply the fold by `scale` (tree_mean's f32(1/W)) */
  FJAGG_ACCUMULATE = 1 << 1,  /* fold starts from the current contents of the output */
  FJAGG_NONTEMPORAL = 1 << 2, /* non-temporal (streaming) loads of the client deltas */
  FJAGG_UNALIGNED = 1 << 3,   /* ptrs path: some pointer is not 16-byte aligned */
  FJAGG_UNBALANCED = 1 << 4,  /* dense path: one tile per workgroup instead of a balanced
                                 resident grid (tuning / A-B only) */
  FJAGG_NARROW = 1 << 5,      /* pytree path, plan AND launch: 64-element stripes per workgroup,
                                 client rows staged through LDS (k_ptrs_narrow) — for small
                                 leaves and many clients; fold only (no fused norms). With
                                 FJAGG_VARIANT(20 / 21 / 22) in both calls: stripes of 64 / 32 / 16
                                 elements folded by the stripe pipeline (k_ptrs_stripe: LDS-
                                 transposed products, one fold wave per stripe); every client and
                                 output pointer must then be 16-byte aligned */
  FJAGG_HOST_TABLES = 1 << 6, /* the weights (and on the pytree path the plan image) are HOST
                                 pointers: the launch copies them into the kernel arguments, so
                                 no upload or staging copy runs on the stream before the fold and
                                 the caller's buffers are free again when the call returns.
                                 Dense: K <= FJAGG_KARG_MAX_WEIGHTS, (in, acc, out) one of
                                 (F32,F32,F32) (BF16,F32,BF16) (BF16,F32,F32), not FJAGG_NARROW
                                 shapes. Pytree: (F32,F32,F32), 16-byte units (no FJAGG_UNALIGNED,
                                 no FJAGG_NARROW), fjagg_karg_image_words(K, L, nblk) <=
                                 FJAGG_KARG_MAX_WORDS. Anything else returns FJAGG_EUNSUPPORTED
                                 (nothing launched): upload the tables and call without the flag. */
  FJAGG_ZEROED_WS = 1 << 7,   /* fused-norm calls (fjagg_wsum_l2_*): the workspace's first 16 bytes
                                 are a completion counter that is zero before the call — zero it
                                 once when the workspace is allocated; every call leaves it zero —
                                 and the norm partials follow it. With K <= 128 and a 16-byte
                                 aligned workspace the fold's last workgroup then adds the
                                 partials itself, with no second (combine) launch; the norms are
                                 bitwise the same either way. Without the flag the 16 bytes are
                                 unused. As always, one workspace serves one call at a time.
                                 Bytes 4..7 are an error word: a call that finds the counter
                                 non-zero sets it to 1 (sticky: that call's norms are not valid;
                                 zero both words to recover).
                                 Graph capture: zero it before the capture (every replayed call
                                 leaves it zero) or with a kernel inside it; a hipMemsetAsync
                                 recorded into a graph acts on the first replay only (ROCm 7,
                                 measured: tools/probe_memset_node.py).
                                 (fedjax_amd's callers pass it unless FJAGG_L2_COMBINE_LAUNCH=1.) */
};
/* kernel-argument capacity of FJAGG_HOST_TABLES launches */
#define FJAGG_KARG_MAX_WEIGHTS 1024 /* dense path: 4 KiB of weights */
#define FJAGG_KARG_MAX_WORDS 3584   /* pytree path: 28 KiB = image words + ceil(K/2) weight words */
/* bits 8..15 of flags select a kernel shape of the dense path: 0 = automatic,
 * 1..17 = fixed (units per lane, clients in flight, waves/SIMD) for tuning, 18 = the
 * LDS-staged narrow fold, 19 = the stripe pipeline (fjstripe.hip) with automatic stripe
 * width, 20 / 21 / 22 = with 64 / 32 / 16 columns; see fjagg.hip */
#define FJAGG_VARIANT(v) (((v)&0xff) << 8)

enum fjagg_mode {
  FJAGG_MODE_EXACT = 0, /* sequential per-element fold: bitwise equal to the reference */
  FJAGG_MODE_SPLIT = 1, /* client axis split over workgroups, ordered combine */
};

/* error codes */
#define FJAGG_OK 0
#define FJAGG_EINVAL (-1)
#define FJAGG_EHIP (-2)
#define FJAGG_EUNSUPPORTED (-3)

/* Message of the last failed call on this thread ("" if none). */
const char* fjagg_last_error(void);
/* FJAGG_ABI_VERSION of the loaded library. */
int fjagg_abi_version(void);

/*
 * Dense client-major slab: client k's delta is x_dev + k*ld elements, P
 * contiguous elements each. acc_dtype is FJAGG_F32 (w_dev is float[K]),
 * FJAGG_I32 (integer fold, w_dev is int32[K]) or FJAGG_BF16 (the reference's bfloat16
 * arithmetic, w_dev is float[K]: each weight and the scale are rounded to bf16, every
 * product and sum is rounded to bf16 — jnp on bf16 leaves with weakly typed weights,
 * tree_util.py:32,50,60). Supported (in, acc, out):
 *   (F32,F32,F32) (F32,F32,BF16) (BF16,F32,BF16) (BF16,F32,F32) (I32,F32,F32) (I32,I32,I32)
 *   (I32,I32,F32) (BF16,BF16,BF16); the pytree path supports the same set except
 *   (F32,F32,BF16).
 * mode FJAGG_MODE_SPLIT needs ws_dev of fjagg_split_workspace_bytes(K, P) bytes
 * (ws may be NULL in exact mode); acc FJAGG_BF16 runs in exact mode only.
 * Replaces: the per-client loop of tree_mean, fedjax/core/tree_util.py:85-96.
 */
int fjagg_wsum_dense(int in_dtype, int acc_dtype, int out_dtype, const void* x_dev,
                     int64_t ld, int64_t K, int64_t P, const void* w_dev, float scale,
                     void* out_dev, int flags, int mode, void* ws_dev, int64_t ws_bytes,
                     void* stream);

/* Workspace bytes FJAGG_MODE_SPLIT needs for a K x P fold (0 if split is not used). */
int64_t fjagg_split_workspace_bytes(int64_t K, int64_t P);

/*
 * Pytree path: K clients x L leaves, each leaf a separate allocation.
 * Launches ONE kernel over every leaf. The plan image is an int64 array in
 * device memory laid out as
 *     in_ptrs [K*L]    client k, leaf l at k*L + l (device addresses)
 *     out_ptrs[L]
 *     leaf_n  [L]      elements per leaf
 *     blocks  [2*nblk] from fjagg_ptrs_plan(): per workgroup (first unit | leaf | tail
 *                      flag | element flag, end unit), unit ranges balanced across the CUs
 * Replaces: jax.tree.map over leaves inside tree_weight/tree_add,
 * fedjax/core/tree_util.py:32,50, for the whole tree_mean loop :85-96.
 */
/* Fills blocks[] (2 int64 per workgroup, up to blocks_cap workgroups) for leaves of
 * leaf_n[l] elements and returns the number of workgroups the plan needs (negative
 * FJAGG_E* on error); call with blocks_cap = 0 to size the array. flags: FJAGG_UNALIGNED if any client or
 * output pointer is not 16-byte aligned (the same flag must go to the launch). */
int64_t fjagg_ptrs_plan(int in_dtype, int flags, const int64_t* leaf_n, int L, int64_t* blocks,
                        int64_t blocks_cap);
/* fjagg_ptrs_plan with a per-leaf choice of unit: leaf_elem[l] != 0 marks a leaf whose
 * client or output pointers are not all 16-byte aligned. Its workgroups walk single
 * elements (the element flag, bit 63 of block word 0; ranges of as many units as the
 * vector ranges, since a workgroup's time is its walks over the K clients) while every other leaf keeps
 * 16-byte units, so one misaligned leaf does not slow the whole launch. Launch the
 * plan WITHOUT FJAGG_UNALIGNED. leaf_elem == NULL is fjagg_ptrs_plan. Replaces the same
 * reference loop as fjagg_ptrs_plan (tree_util.py:85-96); a caller-held pytree may be
 * views into one buffer at any element offset (e.g. deserialized msgpack leaves,
 * fedjax/core/serialization.py:79-87). */
int64_t fjagg_ptrs_plan_leaves(int in_dtype, int flags, const int64_t* leaf_n, const uint8_t* leaf_elem,
                               int L, int64_t* blocks, int64_t blocks_cap);
int fjagg_wsum_ptrs(int in_dtype, int acc_dtype, int out_dtype, const int64_t* image_dev,
                    int L, int64_t K, int64_t nblk, const void* w_dev, float scale,
                    int flags, void* stream);
/* int64 words a FJAGG_HOST_TABLES pytree launch carries in its kernel arguments: the
 * image (K*L + 2*L + 2*nblk words; image_dev and w_dev are then host pointers) and the
 * K f32 weights packed two per word. Compare with FJAGG_KARG_MAX_WORDS. */
int64_t fjagg_karg_image_words(int64_t K, int L, int64_t nblk);

/*
 * fjagg_wsum_ptrs fused with every client's squared L2 norm over ALL L leaves, in the
 * same pass (same plan image and nblk as fjagg_wsum_ptrs; the outputs are bitwise
 * the fjagg_wsum_ptrs ones). l2sq_dev[k] = sum over leaves and elements of x^2 in f32,
 * fixed order: per lane a packed-FMA sum of its units' squares -> the wave's lanes by
 * v_permlane32_swap / v_permlane16_swap and DPP row rotations (groups of clients at once)
 * -> LDS per wave -> workgroup partials ws[b*K + k] added in workgroup order (XLA's own
 * reduction order is not pinned; the tests bound it against an f64 norm) by a second launch,
 * or by the fold's last workgroup under FJAGG_ZEROED_WS. Float inputs, float fold, K <= 4096;
 * ws_dev of fjagg_wsum_l2_ptrs_workspace_bytes(K, nblk) bytes.
 * Replaces the per-client tree_l2_norm(delta) of examples/fed_avg.py:79-81
 * (tree_util.py:105-114) next to the tree_mean of the same deltas (:82).
 */
int64_t fjagg_wsum_l2_ptrs_workspace_bytes(int64_t K, int64_t nblk);
int fjagg_wsum_l2_ptrs(int in_dtype, int acc_dtype, int out_dtype, const int64_t* image_dev,
                       int L, int64_t K, int64_t nblk, const void* w_dev, float scale,
                       float* l2sq_dev, int flags, void* ws_dev, int64_t ws_bytes, void* stream);
/*
 * fjagg_wsum_l2_ptrs writing the norms where a deferred running sum's lazy norm views read
 * them: operand k >= first gets its squared norm in sq_dev[k - first] and its correctly
 * rounded square root in norm_dev[k - first] (either may be NULL, not both); operands below
 * `first` are not written. The per-client delta_l2_norm of the library loop
 * (fedjax/algorithms/fed_avg.py:142-144, tree_util.py:111-114) straight from the fold's norm
 * combine, without a separate fill launch. 0 <= first <= K.
 */
int fjagg_wsum_l2_ptrs_rows(int in_dtype, int acc_dtype, int out_dtype, const int64_t* image_dev,
                            int L, int64_t K, int64_t nblk, const void* w_dev, float scale,
                            float* sq_dev, float* norm_dev, int64_t first, int flags, void* ws_dev,
                            int64_t ws_bytes, void* stream);

/*
 * fjagg_wsum_dense (exact mode) fused with the per-client squared L2 norms of the
 * same deltas, in ONE pass over the K x P slab: out as fjagg_wsum_dense (bitwise
 * the same), l2sq_dev[k] = sum_p x_k[p]^2 in f32 with a fixed reduction order
 * (lane partials -> wave xor-butterfly -> LDS per wave -> workgroups in order).
 * Replaces the per-client tree_l2_norm pass of examples/fed_avg.py:79-81 and
 * fedjax/algorithms/fed_avg.py:142-144 (tree_util.py:105-114) for the whole round.
 * Float inputs (f32, bf16), float fold, K <= 4096, rows <= 1 GiB.
 */
int64_t fjagg_wsum_l2_workspace_bytes(int64_t K, int64_t P);
int fjagg_wsum_l2_dense(int in_dtype, int acc_dtype, int out_dtype, const void* x_dev,
                        int64_t ld, int64_t K, int64_t P, const void* w_dev, float scale,
                        void* out_dev, float* l2sq_dev, int flags, void* ws_dev,
                        int64_t ws_bytes, void* stream);

/*
 * Server optimizer step fused into the fold's epilogue. The round's mean
 * g = fl(fold * scale) (bitwise the fjagg_wsum_dense value) is consumed in
 * registers by the server optimizer of examples/fed_avg.py:97-101 /
 * fedjax/algorithms/fed_avg.py:150-154, restating optax's op sequence
 * (fedjax/core/optimizers.py:57-66 apply = update + apply_updates):
 *   SGD       p += neg_lr * g
 *   MOMENTUM  t = g + decay*t; u = nesterov ? g + decay*t : t; p += neg_lr * u
 *   ADAM      mu = (1-b1) g + b1 mu; nu = (1-b2) g*g + b2 nu;
 *             u = (mu/bc1) / (sqrt(nu/bc2 + eps_root) + eps); p += neg_lr * u
 *   ADAGRAD   v = g*g + v; u = (v > 0 ? rsqrt(v + eps) : 0) * g; p += neg_lr * u
 *   RMSPROP   v = (1-b2) g*g + b2 v; u = g * rsqrt(v + eps);
 *             p += neg_lr * u  [F_MOMENTUM: s = neg_lr * u; t = s + decay*m;
 *             p += nesterov ? s + decay*t : t]
 *   YOGI      mu = (1-b1) g + b1 mu; nu = nu - ((1-b2) sign(nu - g*g)) g*g;
 *             u = (mu/bc1) / (sqrt(nu/bc2 + eps_root) + eps); p += neg_lr * u
 *             (bias-corrected as ADAM: optax.scale_by_yogi keeps a count for it)
 * (rsqrt = 1/sqrt evaluated in f64, rounded once; div / sqrt correctly rounded)
 * with every constant pre-rounded to f32 on the host as JAX's weak typing does
 * (bc1 = f32(1 - b1^t), bc2 = f32(1 - b2^t) for the step count t after the
 * increment). params, m (mu / trace) and v (nu) are float32[P], updated in place;
 * mean_dev (optional) also receives g. Only the params/state are written: the
 * mean never round-trips through HBM.
 */
enum fjagg_opt_kind {
  FJAGG_OPT_SGD = 1,      /* optimizers.py:227-250 (momentum None)                          */
  FJAGG_OPT_MOMENTUM = 2, /* optimizers.py:227-250, optax.trace (m)                          */
  FJAGG_OPT_ADAM = 3,     /* optimizers.py:148-178, optax.scale_by_adam (m, v)               */
  FJAGG_OPT_ADAGRAD = 4,  /* optimizers.py:117-145, optax.scale_by_rss (v = sum of squares)  */
  FJAGG_OPT_RMSPROP = 5,  /* optimizers.py:181-224, optax.scale_by_rms (v) [+ trace (m)]     */
  FJAGG_OPT_YOGI = 6      /* optimizers.py:253-281, optax.scale_by_yogi (m, v; bc1, bc2)     */
};
/* RMSPROP: b2 / one_minus_b2 = decay / 1 - decay. optax.rmsprop's chain is the rescale,
 * then scale_by_learning_rate, then (flags & FJAGG_OPT_F_MOMENTUM) optax.trace(decay = this
 * struct's `decay`, nesterov) of the lr-scaled update (m holds that trace), then
 * apply_updates. flags & FJAGG_OPT_F_CENTERED: the rescale is optax.scale_by_stddev
 * (m holds mu: u = g * rsqrt(nu - mu*mu + eps)); not combinable with the momentum flag
 * (a third state). */
#define FJAGG_OPT_F_MOMENTUM 1
#define FJAGG_OPT_F_CENTERED 2
typedef struct fjagg_server_opt {
  int kind;
  int nesterov;
  float neg_lr;
  float decay;
  float one_minus_b1, b1, one_minus_b2, b2;
  float bc1, bc2;
  float eps, eps_root;
  int flags;
} fjagg_server_opt;
int fjagg_server_update_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                              const float* w_dev, float scale, const fjagg_server_opt* opt,
                              float* params_dev, float* m_dev, float* v_dev, float* mean_dev,
                              int flags, void* stream);
/* The same step on the pytree path: the plan image of fjagg_wsum_ptrs (same blocks,
 * nblk; weights f32) with out_ptrs[L] = the float32 params leaves (updated in place)
 * and state_dev[3*L] (device) = m leaves | v leaves | mean leaves (0 where absent; m
 * for MOMENTUM/ADAM, v for ADAM; mean optional). flags: FJAGG_NONTEMPORAL,
 * FJAGG_UNALIGNED. Replaces tree_mean + server_optimizer.apply over the pytrees of
 * examples/fed_avg.py:82,97-101 in one pass. */
int fjagg_server_update_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk,
                             const float* w_dev, float scale, const fjagg_server_opt* opt,
                             const int64_t* state_dev, int flags, void* stream);

/*
 * Squared L2 norm of each of K client deltas (the per-client diagnostic of
 * examples/fed_avg.py:79-81 -> tree_util.py:105-108), accumulated in f32 per
 * workgroup and combined in a fixed order: deterministic, not bitwise equal to
 * XLA's reduction tree. out_dev is float[K]; ws_dev needs
 * fjagg_l2sq_workspace_bytes(K, P) bytes.
 */
int64_t fjagg_l2sq_workspace_bytes(int64_t K, int64_t P);
int fjagg_l2sq_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                     float* out_dev, void* ws_dev, int64_t ws_bytes, void* stream);

/*
 * Pytree form of the squared norm: R rows at arbitrary device addresses, the
 * image is int64 [ptrs[R] | n[R]]; rows are grouped in consecutive runs of
 * rows_per_group (one client's leaves), out_dev[g] = sum of the group's squares
 * (sqrt of it when take_sqrt != 0: tree_l2_norm, tree_util.py:111-114). Each row
 * is summed in 64 Ki-element blocks and the partials are added in row/block order.
 */
int64_t fjagg_l2sq_rows_workspace_bytes(int64_t R, int64_t max_n);
int fjagg_l2sq_rows(int in_dtype, const int64_t* image_dev, int64_t R, int64_t max_n,
                    int64_t rows_per_group, int take_sqrt, float* out_dev, void* ws_dev,
                    int64_t ws_bytes, void* stream);

/*
 * Clipped weighted mean: per-client norm clipping inside the fold. Replaces the running-sum
 * loop of fedjax/algorithms/mime_lite.py:131-149 — tree_l2_norm(delta), tree_clip_by_global_norm
 * (fedjax/core/tree_util.py:117-133), the clipped norm and flag, then weight and add — for a
 * whole round, with no host synchronisation and no clipped copies: two passes over the deltas
 * (squared norms by fjagg_l2sq_*, then the fold). Float32 deltas, fold and output.
 * With C = f32(max_norm) and q_k client k's squared l2 norm:
 *     n_k = sqrt_rn(q_k)                          correctly rounded (tree_util.py:111-114)
 *     r_k = div_rn(C, n_k)                        correctly rounded
 *     c_k = isnan(r_k) ? r_k : (r_k < 1 ? r_k : 1)   jnp.minimum(1, r): NaN propagates; n = 0 -> 1
 *     t_k = fl(fl(c_k * x_k[p]) * w_k)            two roundings, no FMA (tree_util.py:133, then :32)
 *     s_0 = t_0 (fl(out[p] + t_0) with FJAGG_ACCUMULATE); s_k = fl(s_{k-1} + t_k) in client order
 *     out[p] = fl(s_{K-1} * scale) with FJAGG_SCALE
 * (fl(fl(c x) w) is not fl(x fl(c w)): the factor cannot be merged into the weight bitwise.)
 * Flags: FJAGG_SCALE, FJAGG_ACCUMULATE, FJAGG_NONTEMPORAL and, on the pytree path,
 * FJAGG_UNALIGNED. FJAGG_NARROW, FJAGG_HOST_TABLES, FJAGG_ZEROED_WS, a FJAGG_VARIANT byte,
 * other dtypes, and K > 4096 with norms return FJAGG_EUNSUPPORTED with nothing launched.
 */
/* norm_dev[k] = n_k (norm_dev may be NULL) and c_dev[k] = c_k from l2sq_dev[k] = q_k: one small
 * launch. Replaces tree_util.py:131-132 for K clients. */
int fjagg_clip_scales(const float* l2sq_dev, int64_t K, float max_norm, float* norm_dev, float* c_dev,
                      void* stream);
/* The dense exact fold of fjagg_wsum_dense with the per-client device factor c_dev[k] applied
 * before the weight (c_dev is any device vector, not necessarily fjagg_clip_scales'). With
 * l2sq_clipped_dev (nullable) also l2sq_clipped_dev[k] = sum_p fl(c_k x_k[p])^2, in the
 * reduction order of fjagg_wsum_l2_dense, its workgroup partials added by a separate combine
 * launch; ws_dev of fjagg_wsum_clip_workspace_bytes(K, P) bytes is needed only then.
 * Replaces tree_util.py:133 + :32 + :47-54 inside the loop of mime_lite.py:131-149. */
int64_t fjagg_wsum_clip_workspace_bytes(int64_t K, int64_t P);
int fjagg_wsum_clip_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                          const float* w_dev, const float* c_dev, float scale, void* out_dev,
                          float* l2sq_clipped_dev, int flags, void* ws_dev, int64_t ws_bytes, void* stream);
/* The same fold on the pytree path: the plan image and blocks of fjagg_ptrs_plan_leaves as
 * fjagg_wsum_ptrs takes them (per-leaf element units for misaligned leaves included); w_dev
 * and c_dev are float[K]. ws_dev of fjagg_wsum_clip_ptrs_workspace_bytes(K, nblk) bytes with
 * l2sq_clipped_dev. Replaces the same reference lines as fjagg_wsum_clip_dense. */
int64_t fjagg_wsum_clip_ptrs_workspace_bytes(int64_t K, int64_t nblk);
int fjagg_wsum_clip_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk,
                         const float* w_dev, const float* c_dev, float scale, float* l2sq_clipped_dev,
                         int flags, void* ws_dev, int64_t ws_bytes, void* stream);
/* The round's diagnostics (mime_lite.py:139-146): clipped_dev[k] = (c_k != 1), true for NaN as
 * jnp.not_equal of two NaN norms is; clipped_norm_dev[k] = (c_k == 1) ? norm_dev[k] :
 * sqrt_rn(l2sq_clipped_dev[k]) — an unclipped client's norm verbatim, so clipped_norm == norm
 * bit for bit whenever nothing was clipped. Either output may be NULL, not both. */
int fjagg_clip_finish(const float* norm_dev, const float* c_dev, const float* l2sq_clipped_dev, int64_t K,
                      float* clipped_norm_dev, uint8_t* clipped_dev, void* stream);

/*
 * Clipped weighted mean with the server optimizer step in the fold's epilogue: a round that
 * clips the client deltas and then steps the server model (fedjax/algorithms/mime_lite.py:131-149,
 * then :162-167, `params = p - server_learning_rate * mean`; any clipped FedAvg with an adaptive
 * server optimizer) in one launch. Float32 deltas, fold, params and state. For every element p
 *     y[p] = the clipped mean of fjagg_wsum_clip_* with FJAGG_SCALE, bit for bit
 *            (t_k = fl(fl(c_k * x_k[p]) * w_k), summed in client order, times scale)
 *     (params, m, v)[p] <- the update rules of fjagg_server_update_dense with *opt and g = y[p]
 * The mean stays in registers (mean_dev, optional, also receives it). With FJAGG_OPT_SGD the step
 * is fl(p + fl(f32(-lr) * y)), the bits of Mime Lite's fl(p - fl(f32(lr) * y)).
 * l2sq_clipped_dev (nullable) receives the clipped squares exactly as fjagg_wsum_clip_* forms
 * them on the same deltas (the same workgroup partition, partial rows and combine launch);
 * ws_dev of fjagg_wsum_clip_workspace_bytes(K, P) / fjagg_wsum_clip_ptrs_workspace_bytes(K, nblk)
 * bytes is needed only then. Flags: FJAGG_NONTEMPORAL and, on the pytree entry, FJAGG_UNALIGNED;
 * the scale is always applied. Everything fjagg_wsum_clip_* refuses, FJAGG_ACCUMULATE, a bad
 * descriptor, null x / w / c / params, a null moment the rule reads (dense), K < 1, a bad P, ld
 * or plan, rows over 1 GiB, K > 4096 with l2sq_clipped_dev and a workspace that is too small
 * return their status on the host with nothing launched.
 */
int fjagg_server_update_clip_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                                   const float* w_dev, const float* c_dev, float scale,
                                   const fjagg_server_opt* opt, float* params_dev, float* m_dev, float* v_dev,
                                   float* mean_dev, float* l2sq_clipped_dev, int flags, void* ws_dev,
                                   int64_t ws_bytes, void* stream);
/* The same on the pytree path: the plan image and state_dev[3*L] of fjagg_server_update_ptrs
 * (out_ptrs[L] = the params leaves; m | v | mean leaf addresses, 0 where absent). */
int fjagg_server_update_clip_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk,
                                  const float* w_dev, const float* c_dev, float scale,
                                  const fjagg_server_opt* opt, const int64_t* state_dev,
                                  float* l2sq_clipped_dev, int flags, void* ws_dev, int64_t ws_bytes,
                                  void* stream);

/*
 * Differentially private clipped mean: Gaussian noise in the clipped fold's epilogue, the second
 * half of DP-FedAvg (McMahan et al. 2018: clip each client's update, average, add N(0, sigma^2));
 * the reference has the clipping (tree_clip_by_global_norm, tree_util.py:117-133) and no noise
 * step of its own. Float32 deltas, fold and output. For every element p of leaf l, i its index
 * inside the leaf,
 *     y[p]   = the clipped mean of fjagg_wsum_clip_* with FJAGG_SCALE, bit for bit
 *     out[p] = fl(y[p] + fl(stddev * z_l[i])),   z_l = jax.random.normal(key_l, (n_l,), float32)
 * with z_l exactly fjcomp_normal's values (fjcomp.h): one Threefry block and one erfinv per
 * output element in registers, no noise tensor in memory, no second launch. stddev = 0 is not
 * special-cased (out = fl(y + fl(0 * z))). l2sq_clipped_dev, ws_dev and the workspace sizes are
 * fjagg_wsum_clip_*'s, the clipped squares the same bits. Flags: FJAGG_SCALE (always applied),
 * FJAGG_NONTEMPORAL and, on the pytree entry, FJAGG_UNALIGNED. Everything fjagg_wsum_clip_*
 * refuses, FJAGG_ACCUMULATE, a null or bad descriptor (stddev negative, NaN or inf; L < 1; a leaf
 * of n < 0 or n >= 2^32; dense leaves that overlap, are not ascending or leave the row) return
 * their status on the host with nothing launched. The keys are kernel arguments: a captured
 * launch replays the SAME noise, which voids the privacy guarantee — do not capture these.
 *
 * The leaf table travels in the kernel arguments: up to FJAGG_NOISE_MAX_LEAVES entries. The
 * dense entry refuses more with FJAGG_EUNSUPPORTED; the pytree entry then reads leaves_dev, the
 * same L entries in device memory (FJAGG_EUNSUPPORTED when that is NULL).
 */
#define FJAGG_NOISE_MAX_LEAVES 64
typedef struct fjagg_noise_leaf {
  int64_t begin; /* dense: first element of the leaf in a slab row (ascending, disjoint); ptrs: unused */
  int64_t n;     /* elements of the leaf: the draw's length (ptrs: the plan image's leaf_n is used) */
  uint32_t k0, k1; /* the leaf's key */
} fjagg_noise_leaf;
typedef struct fjagg_noise {
  float stddev;
  int32_t L;                         /* leaves (ptrs: the plan's L, in its leaf order) */
  const fjagg_noise_leaf* leaves;     /* host, L entries (may be NULL when L > FJAGG_NOISE_MAX_LEAVES) */
  const fjagg_noise_leaf* leaves_dev; /* device, L entries; read by the pytree entry when L > FJAGG_NOISE_MAX_LEAVES */
} fjagg_noise;
/* Dense slab (the arguments of fjagg_wsum_clip_dense). Elements of a row outside every leaf
 * (padding) get no noise: they receive the clipped mean as fjagg_wsum_clip_dense writes it. */
int fjagg_wsum_clip_noise_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                                const float* w_dev, const float* c_dev, float scale, void* out_dev,
                                float* l2sq_clipped_dev, const fjagg_noise* noise, int flags, void* ws_dev,
                                int64_t ws_bytes, void* stream);
/* Pytree path (the arguments of fjagg_wsum_clip_ptrs): a workgroup of the plan owns one leaf. */
int fjagg_wsum_clip_noise_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk,
                               const float* w_dev, const float* c_dev, float scale, float* l2sq_clipped_dev,
                               const fjagg_noise* noise, int flags, void* ws_dev, int64_t ws_bytes,
                               void* stream);

/*
 * Grouped weighted mean: the per-cluster means of HypCluster's expectation step in one fold.
 * Replaces the G interleaved running sums of fedjax/algorithms/hyp_cluster.py:268-303 —
 * tree_zeros_like per cluster (:278-281), tree_add(sum[c], tree_weight(delta, n)) per client
 * (:289-291), tree_inverse_weight per cluster (:300) — with one launch that reads every
 * member's delta once. Float32 deltas, fold and output. Each of the K clients belongs to at
 * most one of G groups; the M <= K members are listed in member order (sorted stably by group,
 * so client order within a group):
 *     order[M]   the members' client indices        seg[G+1]  group g's members are
 *     wperm[M]   f32 weights in member order                  order[seg[g] .. seg[g+1])
 *     gscale[G]  f32(1 / W_g), read with FJAGG_SCALE gorder[G] optional: slot y of the grid folds
 *                                                             group gorder[y] (a permutation of
 *                                                             [0, G), longest groups first)
 * For group g with members m_0 < m_1 < ... and every element p:
 *     s = +0;  s = fl(s + fl(x_m[p] * w_m)) for each member in order (no FMA)
 *     out_g[p] = fl(s * gscale[g]) with FJAGG_SCALE, else s
 * The sum starts from +0 (tree_zeros_like), so a group whose products are all -0 gives +0 where
 * fjagg_wsum_* over the same members gives -0; the output is never read. A group without
 * members writes nothing, and a client in no group is never loaded. Whether a group has a mean
 * at all (hyp_cluster.py:298-302: only when its total weight is > 0) is the caller's decision:
 * leave such a group's segment empty.
 * Tables: the device copies are what the kernels read; the entries also take the HOST copies of
 * seg (and, dense, order) and check them before any HIP call — FJAGG_EINVAL when G < 1, seg[0]
 * != 0, seg is not monotone, seg[G] != M, or an order entry is outside [0, K). The caller keeps
 * the two copies equal (fedjax_amd builds both from one array).
 * Flags: FJAGG_SCALE, FJAGG_NONTEMPORAL and, on the pytree path, FJAGG_UNALIGNED. FJAGG_NARROW,
 * FJAGG_HOST_TABLES, FJAGG_ZEROED_WS, FJAGG_ACCUMULATE, FJAGG_UNBALANCED, a FJAGG_VARIANT byte
 * and other dtypes return FJAGG_EUNSUPPORTED with nothing launched. G <= 65535.
 */
/* Dense: client k's row at x_dev + k*ld elements, group g's result at out_dev + g*out_ld. */
int fjagg_wsum_group_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t M,
                           int64_t G, const int32_t* order_dev, const int32_t* seg_dev,
                           const float* wperm_dev, const float* gscale_dev, const int32_t* gorder_dev,
                           const int32_t* order_host, const int32_t* seg_host, void* out_dev,
                           int64_t out_ld, int flags, void* stream);
/* The kernel shape fjagg_wsum_group_dense runs with for these arguments (nothing is launched;
 * M members in `nonempty` non-empty groups): 0 = single-element units, E=1 x U=8 — x_dev, out_dev
 * or a row stride (ld; out_ld when G > 1) is not 16-byte aligned, or P < 4 — else 16-byte units
 * with the FJAGG_VARIANT number of the shape: 2 (E=1 x U=8: fewer than 8 members per group on
 * average, or fewer than 128 Ki units), 5 (E=4 x U=4: below 256 Ki units), 12 (E=8 x U=4).
 * A caller that wants the 16-byte path pads its row strides to 4 elements. The shapes serve the
 * same lines of hyp_cluster.py:268-303; negative FJAGG_E* on a bad shape. */
int fjagg_group_dense_shape(const void* x_dev, int64_t ld, int64_t P, int64_t M, int64_t nonempty, int64_t G,
                            const void* out_dev, int64_t out_ld);
/* Pytree path (the same lines of hyp_cluster.py:268-303 over separate leaves): the image is
 *     in_ptrs[M*L] member i, leaf l at i*L + l | out_ptrs[G*L] | leaf_n[L] | blocks[2*nblk]
 * with the blocks of fjagg_ptrs_plan_leaves (one leaf plan serves every group; mark a leaf
 * unaligned when any member's or any group's pointer to it is). K only bounds M. */
int fjagg_wsum_group_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t M, int64_t G,
                          int64_t nblk, const int32_t* seg_dev, const float* wperm_dev,
                          const float* gscale_dev, const int32_t* gorder_dev, const int32_t* seg_host,
                          int flags, void* stream);

/*
 * Grouped fold with each cluster's server step in its epilogue: one HypCluster round per launch.
 * Replaces, after the expectation step, the per-cluster loop of
 * fedjax/algorithms/hyp_cluster.py:107-128 — server_optimizer.apply(delta_params, opt_state,
 * params) on every cluster whose mean is not None — so the G means never go to HBM. Float32
 * deltas, fold and state. For every group g with members (seg[g+1] > seg[g]):
 *     y[p] = the grouped mean above, bit for bit (from +0, members in order, * gscale[g])
 *     (params_g, m_g, v_g)[p] <- the update rules of fjagg_server_update_dense with opts[g]
 * opts[G] holds one descriptor PER GROUP: the clusters' step counts differ once a cluster has sat
 * out a round, so bc1 / bc2 and a scheduled neg_lr do. Of a group without members nothing is
 * read or written — not its params, moments, mean or descriptor; which groups have a mean
 * (W_g > 0) and whose counts advance is the caller's decision, as for fjagg_wsum_group_*.
 * Both entries take the group tables of fjagg_wsum_group_* (device and HOST copies) and also the
 * device and HOST copies of opts and of the address tables, and check the host copies before any
 * HIP call. FJAGG_EINVAL: what fjagg_wsum_group_* returns it for; flags without FJAGG_SCALE (the
 * step takes the mean); for a group that will be folded, a descriptor that is not valid (kind
 * outside 1..6, unknown flags), a params address of 0, or an m / v address of 0 that the rule
 * reads. FJAGG_EUNSUPPORTED: what fjagg_wsum_group_* returns it for (FJAGG_ACCUMULATE included).
 * Flags: FJAGG_SCALE (mandatory), FJAGG_NONTEMPORAL and, on the pytree path, FJAGG_UNALIGNED.
 */
/* Dense (hyp_cluster.py:107-128 on a slab): fjagg_wsum_group_dense's arguments without the output;
 * state[4*G] int64 = group g's params | m | v | mean address at state[4g ..] (float32[P] each; 0
 * where absent; mean optional: it also receives y). The kernel shape is
 * fjagg_group_dense_shape(x_dev, ld, P, M, nonempty, G, NULL, round_up(P, 4)): the state needs no
 * alignment. */
int fjagg_server_update_group_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t M,
                                    int64_t G, const int32_t* order_dev, const int32_t* seg_dev,
                                    const float* wperm_dev, const float* gscale_dev, const int32_t* gorder_dev,
                                    const int32_t* order_host, const int32_t* seg_host,
                                    const fjagg_server_opt* opts_dev, const int64_t* state_dev,
                                    const fjagg_server_opt* opts_host, const int64_t* state_host, int flags,
                                    void* stream);
/* Pytree path (hyp_cluster.py:107-128 over separate leaves): fjagg_wsum_group_ptrs's arguments
 * with out_ptrs[G*L] of the image = the clusters' params leaves, and state[G*3*L] int64 = per group
 * m leaves | v leaves | mean leaves, as fjagg_server_update_ptrs lays out state[3*L]. params_host
 * [G*L] and leaf_n_host[L] are the host copies of the image's out_ptrs and leaf_n; a leaf with
 * leaf_n 0 has no blocks (a frozen leaf), and its addresses are not checked or read. */
int fjagg_server_update_group_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t M, int64_t G,
                                   int64_t nblk, const int32_t* seg_dev, const float* wperm_dev,
                                   const float* gscale_dev, const int32_t* gorder_dev, const int32_t* seg_host,
                                   const fjagg_server_opt* opts_dev, const int64_t* state_dev,
                                   const fjagg_server_opt* opts_host, const int64_t* state_host,
                                   const int64_t* params_host, const int64_t* leaf_n_host, int flags, void* stream);

/*
 * Coordinate-wise trimmed mean and median over the client axis: the two Byzantine-robust
 * aggregates of Yin, Chen, Ramchandran and Bartlett, "Byzantine-Robust Distributed Learning:
 * Towards Optimal Statistical Rates", ICML 2018 (Definitions 1 and 2). The reference has no such
 * aggregator, so there are no reference lines to cite; the semantics are fixed here.
 * Not a fold: each coordinate needs order statistics across the K clients. One launch, every delta
 * read once, no K x P temporary. Float32 deltas and output, 1 <= K <= 128, trim count 0 <= 2t < K.
 * For every element p, with v_k = x_k[p]:
 *     key(v) = bits(v) ^ (sign(v) ? 0xFFFFFFFF : 0x80000000), compared as uint32: the total order
 *              -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN (NaNs by payload)
 *     the clients are ranked by (key(v_k), k); those of rank t .. K-1-t are kept
 *     s = the first kept v_k verbatim; s = fl(s + v_k) over the kept clients in CLIENT order (no FMA)
 *     out[p] = fl(s * scale) with FJAGG_SCALE (the caller passes f32(1 / (K - 2t))), else s
 * t = 0 is bit for bit fjagg_wsum_dense with unit weights; t = (K-1)/2 is the median (odd K: the
 * middle value; even K: fl(fl(a + b) * 0.5f) with scale 0.5). A +NaN, +inf or huge value is trimmed
 * from the top, a -NaN or -inf from the bottom. There are no weights.
 * Flags: FJAGG_SCALE, FJAGG_NONTEMPORAL and, on the pytree entry, FJAGG_UNALIGNED (the flag the
 * plan was made with). Refused on the host with nothing launched: a dtype other than FJAGG_F32,
 * FJAGG_ACCUMULATE, FJAGG_NARROW, FJAGG_HOST_TABLES, FJAGG_ZEROED_WS, FJAGG_UNBALANCED and a
 * FJAGG_VARIANT byte (FJAGG_EUNSUPPORTED); K > 128 (FJAGG_EUNSUPPORTED); K < 1, t < 0 or 2t >= K,
 * null pointers, P < 1, ld < P, a bad plan (nblk < 1, L < 1) (FJAGG_EINVAL); rows over 1 GiB
 * (FJAGG_EUNSUPPORTED). Rows need float32's alignment only.
 */
/* Dense slab: client k's row at x_dev + k*ld elements, P elements each; out_dev is float[P]. */
int fjagg_trim_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t t, float scale,
                     void* out_dev, int flags, void* stream);
/* Pytree path: the plan image and blocks of fjagg_ptrs_plan_leaves as fjagg_wsum_ptrs takes them
 * (in_ptrs[K*L] | out_ptrs[L] | leaf_n[L] | blocks[2*nblk]; per-leaf element units included), one
 * launch over all leaves. */
int fjagg_trim_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t t, float scale,
                    int flags, void* stream);

/*
 * Bucketing for the two aggregates above: Karimireddy, He and Jaggi, "Byzantine-Robust Learning on
 * Heterogeneous Datasets via Bucketing", ICLR 2022, Algorithm 1 — shuffle the clients, average them in
 * buckets of s, give the B = ceil(K / s) bucket means to the robust rule. The reference has no such
 * aggregator; the semantics are fixed here. The bucket means are formed inside the column
 * routine, where it asks for a value: one launch, no B x P temporary, every delta read twice (once for
 * the sort, once for the sum). Float32, 1 <= K <= 4096 clients, s >= 1, B <= 128, 0 <= 2t < B.
 *     perm = a table of K client indices in device memory, int32 (perm_dev; null: the identity)
 *     bucket j, 0 <= j < B, has the members perm[j*s + i], i = 0 .. n_j - 1, n_j = min(s, K - j*s):
 *              only the last bucket may be short (s > K is s = K: one bucket)
 *     for every element p: a = the first member's x[p] verbatim; a = fl(a + x[p]) over the other
 *              members in table order (no FMA); y_j = a when n_j == 1 (no multiply), else
 *              y_j = fl(a * f32(1 / n_j)), the inverse the float32 of the double quotient; a y_j so
 *              computed that is a NaN becomes +NaN 0x7FC00000 (IEEE leaves a result NaN's sign and
 *              payload open, and the sign decides which end of the order the bucket is trimmed from)
 *     out[p] = fjagg_trim_*'s rule over y_0 .. y_{B-1} in bucket order: the same total order, ties by
 *              bucket index, the kept values added in bucket order, fl(sum * scale) with FJAGG_SCALE
 *              (the caller passes f32(1 / (B - 2t))); t counts buckets, the median is t = (B-1)/2
 * A short last bucket is divided by its own size n_j, not by s: this project's decision (the paper
 * leaves K not divisible by s open); its mean then has the weight of a full bucket in the rule.
 * s = 1 with the identity table is bit for bit fjagg_trim_*; s = 1 with a table is the trimmed mean of
 * the permuted rows; s >= K is the mean in table order. A client holding a NaN poisons only its own
 * bucket, which is then trimmed like any NaN. The host never reads the table, so nothing is uploaded
 * and a graph replay reads it afresh; the kernel clamps every entry into [0, K) before it forms an
 * address, so a stale table can give a wrong result but never an access outside the deltas. A table
 * that is not a permutation counts a client twice or not at all; checking that is the caller's.
 * Flags as fjagg_trim_*. Refused on the host with nothing launched: everything fjagg_trim_* refuses
 * for its dtype and flags (FJAGG_EUNSUPPORTED); s < 1, K < 1, t < 0 or 2t >= B, null pointers other
 * than perm_dev, P < 1, ld < P, a bad plan (FJAGG_EINVAL); B > 128, K > 4096 and rows over 1 GiB
 * (FJAGG_EUNSUPPORTED, fjagg_last_error naming the limit).
 */
/* Dense slab: client k's row at x_dev + k*ld elements, P elements each; out_dev is float[P]. */
int fjagg_trim_bucket_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const int32_t* perm_dev,
                            int64_t s, int64_t t, float scale, void* out_dev, int flags, void* stream);
/* Pytree path: the plan image as fjagg_trim_ptrs takes it, holding all K clients. */
int fjagg_trim_bucket_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk,
                           const int32_t* perm_dev, int64_t s, int64_t t, float scale, int flags, void* stream);

/*
 * The mean around the median over the client axis ("MeaMed": Xie, Koyejo and Gupta, "Generalized
 * Byzantine-tolerant SGD", 2018), which is also the coordinate-wise second stage of Bulyan (El Mhamdi,
 * Guerraoui and Rouault, "The Hidden Vulnerability of Distributed Learning in Byzantium", ICML 2018):
 * per coordinate, the mean of the `keep` client values closest to the coordinate's median. The
 * reference has no such aggregator; the semantics are fixed here. One launch, the
 * participating deltas read once, no temporary. Float32, 1 <= M <= 128 participating clients in client
 * order, 1 <= keep <= M. For every element p, with v_k = x_k[p] and key() and the total order as above:
 *     s_0 .. s_{M-1} = the values ranked by (key(v_k), k); mid = (M-1)/2; med = s_mid (the lower median)
 *     d_j = 0 if key(s_j) == key(med), else |fl(s_j - med)| with a NaN result replaced by +inf
 *     a_lo = max(0, mid - keep + 1), a_hi = min(mid, M - keep),
 *     a = a_lo + #{ i in [a_lo, a_hi) : d_{i+keep} < d_i }   (strict: a tie keeps the lower side)
 *     the clients of rank a .. a + keep - 1 are kept (ties among equal keys by client index)
 *     s = the first kept v_k verbatim; s = fl(s + v_k) over the kept clients in CLIENT order (no FMA)
 *     out[p] = fl(s * scale) with FJAGG_SCALE (the caller passes f32(1 / keep)), else s
 * keep = M is bit for bit fjagg_trim_* at t = 0; keep = 1 is s_mid verbatim (odd M: the median).
 * There are no weights. The dense entry takes an optional table of M slab rows: participating client
 * k is row rows_host[k] of a slab of K_rows rows (strictly ascending; null: rows 0 .. M-1). The table
 * travels in the kernel arguments: nothing is uploaded, and a row outside the table is never read.
 * Flags: FJAGG_SCALE, FJAGG_NONTEMPORAL and, on the pytree entry, FJAGG_UNALIGNED (the flag the
 * plan was made with). Refused on the host with nothing launched: everything fjagg_trim_* refuses
 * for its dtype, flags and client count (M > 128: FJAGG_EUNSUPPORTED; M < 1: FJAGG_EINVAL); keep < 1
 * or keep > M, M > K_rows, K_rows < 1, rows not strictly ascending or outside [0, K_rows), null
 * pointers, P < 1, ld < P, a bad plan (FJAGG_EINVAL); K_rows > 1024 and rows over 1 GiB
 * (FJAGG_EUNSUPPORTED).
 */
/* Dense slab: row r at x_dev + r*ld elements, P elements each; out_dev is float[P]. */
int fjagg_meamed_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K_rows, int64_t P, const int32_t* rows_host,
                       int64_t M, int64_t keep, float scale, void* out_dev, int flags, void* stream);
/* Pytree path: the plan image as fjagg_trim_ptrs takes it, holding only the K participating clients. */
int fjagg_meamed_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t keep, float scale,
                      int flags, void* stream);

/*
 * The K x K Gram matrix of the client deltas, G[i][j] = sum_p x_i[p] * x_j[p], in float64: the one
 * pass over the deltas that the two whole-vector Byzantine-robust aggregates need. Krum and
 * multi-Krum (Blanchard, El Mhamdi, Guerraoui and Stainer, "Machine Learning with Adversaries:
 * Byzantine Tolerant Gradient Descent", NeurIPS 2017) score client i by its squared distances
 * d2(i,j) = G_ii + G_jj - 2 G_ij; every iterate of the smoothed Weiszfeld algorithm for the
 * geometric median (Pillutla, Kakade and Harchaoui, "Robust Aggregation for Federated Learning",
 * IEEE Trans. Signal Processing 2022) is v = sum_j a_j x_j, so |v - x_k|^2 = a'Ga - 2 (Ga)_k + G_kk.
 * The reference has neither aggregator, so there are no reference lines to cite; the semantics
 * are fixed here. The selection itself runs over G, on the host
 * (fedjax_amd/robust.py) or on the device (fjagg_krum_select, fjagg_weiszfeld_select below); the
 * final mean is a grouped fold that never loads an excluded client.
 * Float32 deltas, 1 <= K <= 1024, one GPU. Arithmetic:
 *     the columns of a row are cut into chains of at most FJAGG_GRAM_CHAIN consecutive columns
 *       (dense: from column 0, and a workgroup's chunk, fjagg_gram_chunk_columns, is whole chains;
 *       pytree: from the start of every plan entry, so a chain never crosses a leaf)
 *     within a chain  c = +0; c = fmaf(x_i[p], x_j[p], c) in column order   (v_mfma_f32_32x32x2_f32)
 *     chain results are added in float64: a workgroup adds its chains in column order, then the
 *       workgroups' sums are added in chunk order by a second small kernel over the workspace
 * No floating-point atomics; the order is a function of (K, P) (dense) or of the plan (pytree),
 * so the result is run-to-run bitwise reproducible, and G[i][j] and G[j][i] are the same bits.
 * |G_ij - exact| <= gamma_C * sum_p |x_i[p] x_j[p]|, gamma_C = C u / (1 - C u), u = 2^-24,
 * C = FJAGG_GRAM_CHAIN (the float64 additions add under 1 % of that). A non-finite value in client
 * k's delta makes row k and column k of G non-finite and changes no other entry's bits. Rows past K
 * and columns past P are zeros made on chip, never loaded. Loads are 4 bytes wide: rows and leaves
 * need float32's alignment only. The workspace needs no zeroing and carries nothing between calls.
 * Flags: FJAGG_UNALIGNED on the pytree entry (the flag the plan was made with). Refused on the host
 * with nothing launched: a dtype other than FJAGG_F32, FJAGG_ACCUMULATE, FJAGG_NARROW,
 * FJAGG_HOST_TABLES, FJAGG_ZEROED_WS, FJAGG_UNBALANCED, any other flag or a FJAGG_VARIANT byte, K > 1024,
 * rows over 1 GiB (FJAGG_EUNSUPPORTED); K < 1, P < 1, ld < P, a bad plan, null pointers, a workspace
 * under fjagg_gram_workspace_bytes (FJAGG_EINVAL).
 */
#define FJAGG_GRAM_CHAIN 256
/* Dense slab: client k's row at x_dev + k*ld elements; gram_dev is double[K][K], row-major. */
int fjagg_gram_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, double* gram_dev, void* ws_dev,
                     int64_t ws_bytes, int flags, void* stream);
/* Pytree path: the plan image of fjagg_ptrs_plan_leaves as fjagg_trim_ptrs takes it (in_ptrs[K*L] |
 * out_ptrs[L] | leaf_n[L] | blocks[2*nblk]); out_ptrs is not read. G sums over all leaves. */
int fjagg_gram_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, double* gram_dev,
                    void* ws_dev, int64_t ws_bytes, int flags, void* stream);
/* Workspace bytes: nblk = 0 for the dense entry over P columns, else for a plan of nblk entries. */
int64_t fjagg_gram_workspace_bytes(int64_t K, int64_t P_or_total, int64_t nblk);
/* Columns per workgroup of the dense entry (a multiple of FJAGG_GRAM_CHAIN, a function of K and P alone). */
int64_t fjagg_gram_chunk_columns(int64_t K, int64_t P);

/*
 * Krum's and the smoothed Weiszfeld algorithm's selection on the device, over the Gram matrix above
 * (double[K][K], bitwise symmetric), writing the member tables of ONE group where the grouped fold
 * reads them: a round is fjagg_gram_* -> select -> fjagg_wsum_group_*_dev with no host visit, no
 * synchronisation and nothing uploaded, so it can be captured. The reference has neither aggregator;
 * the semantics are fixed here and in fedjax_amd/csrc/fjselect_dev.h. All arithmetic is
 * float64 in separate IEEE operations (no FMA, correctly rounded divide and square root); there are
 * no floating-point atomics, and the order of every sum is a function of (K, f, m) or of
 * (K, iterations) alone: two runs give the same bits. 1 <= K <= 1024.
 *     usable_k = isfinite(G_kk)
 * Krum / multi-Krum (fjagg_krum_select; bit for bit fedjax_amd.robust.krum_scores / krum_select):
 *     d2(i,j)  = fl(fl(G_ii + G_jj) - fl(2 G_ij)); finite: max(d2, +0), else +inf; +inf when either
 *                client is unusable; j = i is left out
 *     score_i  = the K - f - 2 smallest d2(i, .) added in ascending order from 0.0; +inf if unusable
 *     selected = the m smallest FINITE scores, ties to the lower index; count = how many (0 .. m)
 *     scores[K]; selected[m] best first, -1 padded; count[1];
 *     order[m] the selected clients in ASCENDING client index (0 padded); seg = {0, count};
 *     wperm[m] = 1.0f; gscale[0] = count > 0 ? (float)(1.0 / (double)count) : 0.0f
 * Two launches: one workgroup per row sorts its K uint64 keys in LDS (the bits of a non-negative
 * double order as it does) and one lane adds; one workgroup ranks (score, index).
 * Smoothed Weiszfeld (fjagg_weiszfeld_select), alpha[K] float64 weights (NULL: ones), nu finite
 * and > 0, iterations >= 0. Every sum runs over the usable clients in ascending index,
 * sequentially, from 0.0:
 *     S = sum alpha_k; a_k = alpha_k / S; then `iterations` times
 *     (Ga)_k = sum_j fl(G_kj a_j);  q = sum_k fl(a_k (Ga)_k);  r_k = fl(fl(q - fl(2 (Ga)_k)) + G_kk)
 *     d_k = sqrt(r_k > 0 ? r_k : (r_k == r_k ? 0 : r_k));  beta_k = alpha_k / max(nu, d_k) (a NaN
 *     propagates);  B = sum beta_k;  a_k = beta_k / B
 *     a[K] (0 if unusable); d[K] (inf if unusable; 0 with iterations = 0); a32[k] = (float)a_k;
 *     order[K] the clients with usable && a32 > 0, ascending (0 padded); seg = {0, count};
 *     wperm[j] = that client's a32 (0 padded); gscale[0] = W > 0 ? (float)(1.0 / W) : 0, W the
 *     sequential float64 sum of the members' a32 in member order
 * One launch of one workgroup runs all iterations; alpha is not checked (the caller passes finite
 * positive weights).
 * Refused on the host with nothing launched: K < 1, f < 0, K < 2f + 3, m outside [1, K - f],
 * iterations < 0, nu not finite or <= 0, M_max < 1 or M_max > K, L < 1, null pointers (FJAGG_EINVAL);
 * K > 1024 (FJAGG_EUNSUPPORTED). fjagg_last_error names the limit.
 */
int fjagg_krum_select(const double* gram_dev, int64_t K, int64_t f, int64_t m, double* scores_dev,
                      int64_t* selected_dev, int32_t* count_dev, int32_t* order_dev, int32_t* seg_dev,
                      float* wperm_dev, float* gscale_dev, void* stream);
int fjagg_weiszfeld_select(const double* gram_dev, int64_t K, const double* alpha_dev, double nu, int64_t iterations,
                           double* a_dev, double* d_dev, float* a32_dev, int32_t* count_dev, int32_t* order_dev,
                           int32_t* seg_dev, float* wperm_dev, float* gscale_dev, void* stream);
/* fjagg_wsum_group_dense / _ptrs for ONE group (G = 1, no gorder) whose tables a kernel wrote: no
 * host copies of seg and order, nothing checked against them. The kernel shape comes from the
 * caller's bound M_max on the member count (m for Krum, K for the geometric median) in place of
 * M; the count folded is seg_dev[1] - seg_dev[0] <= M_max. The same kernels as the entries above:
 * the folds are exact and sequential, so every shape gives the same bits. A count of 0 writes
 * nothing. The flags and the other refusals are those entries'. The pytree image is laid out for
 * M_max members: in_ptrs[M_max*L] | out_ptrs[L] | leaf_n[L] | blocks[2*nblk], slots past the count
 * never read. */
int fjagg_wsum_group_dense_dev(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t M_max,
                               const int32_t* order_dev, const int32_t* seg_dev, const float* wperm_dev,
                               const float* gscale_dev, void* out_dev, int flags, void* stream);
int fjagg_wsum_group_ptrs_dev(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t M_max, int64_t nblk,
                              const int32_t* seg_dev, const float* wperm_dev, const float* gscale_dev, int flags,
                              void* stream);
/* Fills the in_ptrs of such an image: slot j < count gets the L leaf pointers of client order_dev[j]
 * from image_all_dev = in_ptrs[K*L] (the image fjagg_gram_ptrs reads). An order entry outside
 * [0, K) copies nothing. */
int fjagg_gather_member_ptrs(const int64_t* image_all_dev, int L, int64_t K, const int32_t* order_dev,
                             const int32_t* seg_dev, int64_t M_max, int64_t* image_group_dev, void* stream);

/*
 * Bulyan on the device (El Mhamdi, Guerraoui and Rouault, ICML 2018): the first stage's selection over
 * the Gram matrix above, and the second stage (the mean around the median, fjagg_meamed_* above) with
 * its member count, keep count, scale and row table read from device memory where the selection wrote
 * them. A round is fjagg_gram_* -> fjagg_bulyan_select -> fjagg_meamed_*_dev with no host visit, no
 * synchronisation and nothing uploaded, so the dense round can be captured. The semantics are fixed
 * here and in fedjax_amd/csrc/fjselect_dev.h; the selection is bit for bit
 * fedjax_amd.robust.bulyan_select. Float64 in separate IEEE operations, no FMA, no atomics: the result
 * is a function of (G, K, f) alone and two runs give the same bits.
 *     theta    = K - 2f;  usable_k = isfinite(G_kk);  d2(i,j) as Krum's above (clamped at +0, +inf when
 *                not finite or when either client is unusable)
 *     R        = the usable clients not yet chosen; n = |R|; c = max(n - f - 2, 1)
 *     score_i  = for i in R, the c smallest d2(i,j) over j in R \ {i}, added in ascending order from
 *                0.0 (0.0 when n = 1). Neighbours at the same distance add the same term whichever is
 *                taken, so the order among equal distances cannot change a sum.
 *     a step   = the smallest FINITE score wins, ties to the lower client index; the winner leaves R
 *     the selection stops after theta steps, or earlier when R is empty or no score is finite
 *     selected[theta]    int64, selection order, -1 padded;       count[1] int32, the steps made
 *     step_scores[theta] float64, each step's winning score, +inf padded
 *     keep[1]  = count - 2f if that is >= 1, else 0;  scale[1] = keep > 0 ? (float)(1.0 / (double)keep) : 0.0f
 *     rows[theta] int32: the chosen clients in ASCENDING client index; entries past count repeat the last
 *                chosen row (0 when count = 0), so every entry is a row of the slab
 * Limits: K >= 4f + 3 and theta <= 128 (the second stage's width). Together: 2f <= (K - 3) / 2, so
 * K <= 128 + (K - 3) / 2, K <= 253; K = 253 would need f <= 62 and theta = 129, so K <= 252 (f = 62).
 * A client index fits a byte, and one workgroup of 256 lanes owns one row per lane.
 * Two launches: one workgroup per row sorts its (key, index) pairs once in LDS and writes them
 * position-major into the workspace (K (K - 1) * 9 bytes, 8-byte aligned, never zeroed, nothing
 * carried between calls); one workgroup then runs all theta steps, lane i walking row i's sorted list
 * past the clients already chosen, then an argmin on (score bits, index).
 * Refused on the host with nothing launched: K < 1, f < 0, K < 4f + 3, null pointers, a workspace under
 * fjagg_bulyan_select_workspace_bytes or not 8-byte aligned (FJAGG_EINVAL); K > 1024 and K - 2f > 128
 * (FJAGG_EUNSUPPORTED). fjagg_last_error names the limit.
 *
 * The second stage from device tables: fjagg_meamed_*'s arithmetic, column routine and walks, with
 * M = count_dev[0], keep = keep_dev[0] and scale = scale_dev[0] (used with FJAGG_SCALE) read by the
 * kernel; all three are uniform over the grid. The kernel width 16 / 32 / 64 / 128 comes from the caller's
 * bound M_max (Bulyan: theta); the routine ranks by (key, client index) and adds the kept values in
 * client order, so its bits do not depend on the width. Dense: participating client k is slab row
 * rows_dev[k]. Pytree: image_group_dev is laid out for M_max members (in_ptrs[M_max*L] | out_ptrs[L] |
 * leaf_n[L] | blocks[2*nblk]); a first small launch fills ALL M_max slots from image_all_dev =
 * in_ptrs[K_rows*L] (the image fjagg_gram_ptrs reads) by rows_dev, so every slot holds a client's
 * pointers; slots past the count are never read. keep < 1: every output element is +0, written by the
 * kernel itself (a graph replay zeroes too), and no client row is loaded.
 * The kernels form no address from an unchecked table value: count is clamped into [0, M_max], keep into
 * [0, count], every row index into [0, K_rows). A stale table can give a wrong result, never an access
 * outside the slab or the table. The refusals are fjagg_meamed_*'s with M_max in place of M (M_max < 1,
 * M_max > K_rows, K_rows < 1, P < 1, ld < P, a bad plan, null pointers: FJAGG_EINVAL; M_max > 128,
 * K_rows > 1024, rows over 1 GiB, the dtype and the flags: FJAGG_EUNSUPPORTED).
 */
int64_t fjagg_bulyan_select_workspace_bytes(int64_t K); /* 0 for K outside [3, 252] */
int fjagg_bulyan_select(const double* gram_dev, int64_t K, int64_t f, void* ws_dev, int64_t ws_bytes,
                        int64_t* selected_dev, int32_t* count_dev, double* step_scores_dev, int32_t* keep_dev,
                        float* scale_dev, int32_t* rows_dev, void* stream);
int fjagg_meamed_dense_dev(int in_dtype, const void* x_dev, int64_t ld, int64_t K_rows, int64_t P, int64_t M_max,
                           const int32_t* rows_dev, const int32_t* count_dev, const int32_t* keep_dev,
                           const float* scale_dev, void* out_dev, int flags, void* stream);
int fjagg_meamed_ptrs_dev(int in_dtype, const int64_t* image_all_dev, int64_t* image_group_dev, int L, int64_t K_rows,
                          int64_t M_max, int64_t nblk, const int32_t* rows_dev, const int32_t* count_dev,
                          const int32_t* keep_dev, const float* scale_dev, int flags, void* stream);

/*
 * Centered clipping: the robust mean clipped around the previous round's aggregate (Karimireddy, He
 * and Jaggi, "Learning from History for Byzantine Robust Optimization", ICML 2021). The reference has
 * no such aggregator; the semantics are fixed here. Float32 deltas, centre and result,
 * 1 <= K <= 4096, T = tau finite and > 0, iterations >= 1. One iteration from centre v:
 *     d_k[p] = fl(x_k[p] - v[p])
 *     q_k    = sum_p fl(d_k[p]^2)     float32, in fjagg_l2sq_rows' order: leaf by leaf, 64 Ki-element
 *                                     blocks, lane / shuffle tree / wave / block / row as k_l2sq_rows
 *     n_k, c_k = fjagg_clip_scales(q, T)      n = sqrt(q), c = min(1, T / n), NaN propagates, n = 0: c = 1
 *     t_k[p] = c_k > 0 ? fl(c_k * d_k[p]) : +0
 *     s = +0; s = fl(s + t_k[p]) for k = 0 .. K-1 in client order (no FMA)
 *     v'[p] = fl(v[p] + fl(s * f32(1/K)))     the divisor is K, whatever was skipped
 * A client holding a NaN has c = NaN, one holding inf or 1e30 has q = inf and c = 0: both contribute
 * +0 by a select on the factor, so their bits never reach the result (their rows may be loaded).
 * There are no weights. With a zero centre q has fjagg_l2sq_rows' bits.
 * Every lane of the fold keeps its centre unit in registers and writes v' for its own columns only:
 * out may be the centre itself (the same address); a partial overlap is refused, and so is, on the
 * dense entries, an out that touches the slab's extent [x, x + ((K-1)*ld + P)*4): the rows are read
 * while out is written (the centre, only read, may be a row of the slab). No entry visits the host
 * or synchronises; all are capturable.
 * Flags: FJAGG_NONTEMPORAL and, on the pytree entries, FJAGG_UNALIGNED (the flag the plan was made
 * with). The dense entries pick 16-byte units when x_dev, ld, the centre and the output allow it and
 * element units otherwise. Refused with nothing launched, all with the one code FJAGG_EUNSUPPORTED:
 * a dtype other than FJAGG_F32; K < 1 or K > 4096; P < 1, ld < P; tau not finite or <= 0;
 * iterations < 1; null pointers; rows over 1 GiB; FJAGG_SCALE, FJAGG_ACCUMULATE, FJAGG_NARROW,
 * FJAGG_HOST_TABLES, FJAGG_ZEROED_WS, FJAGG_UNBALANCED, a FJAGG_VARIANT byte or any other flag; a
 * partial overlap of out and centre; an out overlapping the dense deltas; a bad plan or leaf table;
 * too small a workspace.
 */
/* The norm pass alone: fjagg_l2sq_rows with a centre per row. image_dev = ptrs[R] | n[R] |
 * center_ptrs[R]; out[g] sums fl((x - v)^2) over the rows of group g. The other arguments and the
 * workspace size (fjagg_l2sq_rows_workspace_bytes) are fjagg_l2sq_rows'; R is not limited to 65535. */
int fjagg_l2sq_rows_centered(int in_dtype, const int64_t* image_dev, int64_t R, int64_t max_n, int64_t rows_per_group,
                             int take_sqrt, float* out_dev, void* ws_dev, int64_t ws_bytes, void* stream);
/* One fold over a dense slab with any device factor vector c_dev[K] (fjagg_clip_scales makes the clip
 * factors): client k's row at x_dev + k*ld elements; center_dev and out_dev are float[P]. */
int fjagg_center_fold_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const float* c_dev,
                            const void* center_dev, void* out_dev, int flags, void* stream);
/* One fold over the plan image of fjagg_trim_ptrs followed by the L centre pointers:
 * in_ptrs[K*L] | out_ptrs[L] | leaf_n[L] | blocks[2*nblk] | center_ptrs[L]. A leaf's centre may be
 * its output. The caller's plan must count the centre pointers in its per-leaf alignment choice. */
int fjagg_center_fold_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, const float* c_dev,
                           int flags, void* stream);
/* Workspace of the two whole-round entries: K clients of L leaves, the largest of max_n elements. */
int64_t fjagg_center_clip_workspace_bytes(int64_t K, int64_t L, int64_t max_n);
/* The whole round over a dense slab, `iterations` times norm pass, fjagg_clip_scales and fold: the
 * first from center_dev into out_dev, the later ones in place on out_dev. distances_dev and
 * factors_dev are float[iterations][K]: n_k and c_k of every iteration. leaf_tab_dev = off[L] | n[L]
 * (int64 element offsets and sizes of the row's leaves, ascending and disjoint, max_n the largest)
 * gives the norms their leaf-by-leaf order; NULL with L = 1 takes the row as one leaf. */
int fjagg_center_clip_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P,
                            const int64_t* leaf_tab_dev, int64_t L, int64_t max_n, float tau, int64_t iterations,
                            const void* center_dev, void* out_dev, float* distances_dev, float* factors_dev,
                            void* ws_dev, int64_t ws_bytes, int flags, void* stream);
/* The whole round over fjagg_center_fold_ptrs' image: the first iteration's centre is center_ptrs,
 * every later one's is out_ptrs (in place). max_n is the largest leaf_n. */
int fjagg_center_clip_ptrs(int in_dtype, const int64_t* image_dev, int L, int64_t K, int64_t nblk, int64_t max_n,
                           float tau, int64_t iterations, float* distances_dev, float* factors_dev, void* ws_dev,
                           int64_t ws_bytes, int flags, void* stream);

/*
 * FLTrust: the trust-weighted mean of the client deltas against a delta g the server computed itself
 * on a small trusted dataset (Cao, Fang, Liu and Gong, "FLTrust: Byzantine-robust Federated Learning
 * via Trust Bootstrapping", NDSS 2021). It needs no honest majority. The reference has no such
 * aggregator; the semantics are fixed here and in fedjax_amd/csrc/fjtrust_dev.h.
 * Float32 deltas x_k, server delta and result, 1 <= K <= 4096, no client weights, leaves
 * l = 0 .. L-1 in flatten order.
 * Pass 1, float32, no FMA:
 *     a_k = sum_p fl(x_k[p] * g[p]);  q_k = sum_p fl(x_k[p]^2)
 *   both in fjagg_l2sq_rows' order exactly: leaf by leaf, in 64 Ki-element blocks; lane t of 256 adds
 *   elements t, t + 256, ... ascending from +0; the xor shuffle tree 32 .. 1; the four wave sums in
 *   order; the block partials in leaf / block order from +0. q_k has fjagg_l2sq_rows' bits, and
 *     q_s = sum_p fl(g[p]^2)     is fjagg_l2sq_rows' own output over the server delta's leaves.
 * Selection, float64, no FMA, one rounding per operation:
 *     n_k = sqrt((double)q_k);  n_s = sqrt((double)q_s);  cos_k = (double)a_k / (n_k * n_s)
 *     ts_k = cos_k > 0 ? min(cos_k, 1) : 0            (a NaN gives 0)
 *     c_k  = ts_k > 0 ? (float)((ts_k * n_s) / n_k) : 0
 *     c_k not a finite float32 > 0: c_k = 0 and ts_k = 0
 *     T = sum_k ts_k in client order from +0.0, sequentially;  r = T > 0 ? (float)(1.0 / T) : 0
 *     order[K] = the clients with c_k > 0, ascending (0 padded); seg = {0, count};
 *     wperm[j] = c_order[j] (0 padded); gscale[0] = r
 *   and the diagnostics cos[K], trust[K] = ts (double), factors[K] = c, norms[K] = (float)n_k,
 *   server_norm = (float)n_s, total = T, count. A NaN cosine or norm is stored as the quiet NaN
 *   0x7ff8000000000000 / 0x7fc00000 (the payload of a 0/0 is the processor's).
 * Pass 2, the grouped fold above with G = 1 (fjagg_wsum_group_*_dev) over those tables:
 *     s = +0; s = fl(s + fl(x_m[p] * c_m)) in member order;  y[p] = fl(s * r)
 *   A client that is not in the table is never loaded. A count of 0 writes nothing, so the drivers
 *   zero y first: a round that trusts nobody gives all +0.
 * Consequences: a client holding a NaN has a or q NaN, so ts = 0. One holding inf or 1e30 has
 * q = inf, so cos is 0 or NaN and ts = 0. An all-zero client gives 0/0, so ts = 0. A client so small
 * that q underflows to 0 gets c = inf, which is zeroed. A zero or non-finite server delta trusts
 * nobody. For finite inputs |y| <= |g| up to rounding: y is a convex combination of vectors of norm
 * n_s. The clamp at 1 matters: on clients that are exact multiples of g the float32 sums give cos up
 * to 1 + 1.5e-7.
 * No entry visits the host or synchronises; all are capturable. Flags: FJAGG_NONTEMPORAL (the deltas
 * of both passes) and, on fjagg_fltrust_ptrs, FJAGG_UNALIGNED (the flag the plan was made with).
 * Refused with nothing launched, all with the one code FJAGG_EUNSUPPORTED: a dtype other than
 * FJAGG_F32; K < 1 or K > 4096; P < 1 or ld < P; rows over 1 GiB; a null pointer; too small a
 * workspace (or, for the drivers, one not 16-byte aligned); an out overlapping the dense deltas, the
 * server delta, the workspace or a diagnostics buffer; a leaf table, row grouping or plan whose
 * host-side numbers are bad (L > 65535, max_n > P); any other flag. fjagg_last_error names the limit.
 * What lives in device memory is TRUSTED, because checking it would take a host visit: a leaf table's
 * entries (the caller guarantees off[l] + n[l] <= P and n[l] <= max_n), the pointers and sizes of an
 * image, the plan blocks. A wrong entry reads outside the rows. The diagnostics buffers must not
 * overlap each other, the workspace or the inputs; of these only out is checked.
 */
/* The row pass alone over rows at arbitrary 4-byte aligned addresses: image_dev = ptrs[R] | n[R] |
 * ref_ptrs[R] (fjagg_l2sq_rows_centered's image), dot[g] and sq[g] the sums over the rows_per_group
 * rows of group g in the order above. R is not limited to 65535. */
int64_t fjagg_dotsq_rows_workspace_bytes(int64_t R, int64_t max_n);
int fjagg_dotsq_rows(int in_dtype, const int64_t* image_dev, int64_t R, int64_t max_n, int64_t rows_per_group,
                     float* dot_dev, float* sq_dev, void* ws_dev, int64_t ws_bytes, void* stream);
/* The same over a dense slab against one shared vector ref_dev[P]: client k's row at x_dev + k*ld
 * elements. leaf_tab_dev = off[L] | n[L] (int64 element offsets and sizes of the row's leaves, max_n
 * the largest) gives the sums their leaf-by-leaf order; NULL with L = 1 takes the row as one leaf.
 * Workspace: fjagg_dotsq_rows_workspace_bytes(K * L, max_n). */
int fjagg_dotsq_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const int64_t* leaf_tab_dev,
                      int64_t L, int64_t max_n, const void* ref_dev, float* dot_dev, float* sq_dev, void* ws_dev,
                      int64_t ws_bytes, int flags, void* stream);
/* The selection alone: one launch of one workgroup; T is added by one lane. Every index it writes
 * lies in [0, K). */
int fjagg_fltrust_select(const float* dot_dev, const float* sq_dev, const float* server_sq_dev, int64_t K,
                         double* cos_dev, double* trust_dev, float* factors_dev, float* norms_dev,
                         float* server_norm_dev, double* total_dev, int32_t* count_dev, int32_t* order_dev,
                         int32_t* seg_dev, float* wperm_dev, float* gscale_dev, void* stream);
/* Workspace of the two whole-round entries (the sums, the member tables, the block partials). */
int64_t fjagg_fltrust_workspace_bytes(int64_t K, int64_t L, int64_t max_n);
/* The whole round over a dense slab: server norm, row pass, selection, out zeroed, fold. server_dev and
 * out_dev are float[P]; the leaf table as fjagg_dotsq_dense's. */
int fjagg_fltrust_dense(int in_dtype, const void* x_dev, int64_t ld, int64_t K, int64_t P, const int64_t* leaf_tab_dev,
                        int64_t L, int64_t max_n, const void* server_dev, void* out_dev, double* cos_dev,
                        double* trust_dev, float* factors_dev, float* norms_dev, float* server_norm_dev,
                        double* total_dev, int32_t* count_dev, void* ws_dev, int64_t ws_bytes, int flags, void* stream);
/* The whole round over pytrees: image_all_dev = in_ptrs[K*L] | server_ptrs[L] | leaf_n[L];
 * image_group_dev = in_ptrs[K*L] (member slots, filled here as fjagg_gather_member_ptrs fills them) | out_ptrs[L] |
 * leaf_n[L] | blocks[2*nblk], the plan of fjagg_wsum_group_ptrs_dev for M_max = K. Every output leaf
 * is zeroed before the fold. max_n is the largest leaf_n. */
int fjagg_fltrust_ptrs(int in_dtype, const int64_t* image_all_dev, int64_t* image_group_dev, int L, int64_t K,
                       int64_t nblk, int64_t max_n, double* cos_dev, double* trust_dev, float* factors_dev,
                       float* norms_dev, float* server_norm_dev, double* total_dev, int32_t* count_dev, void* ws_dev,
                       int64_t ws_bytes, int flags, void* stream);

/*
 * Synthetic client deltas for tests and benchmarks (never on the product path):
 *   x[k][p] = amp * u(seed, k0 + k, p),  u = uniform in [-1, 1) with 2^-23 steps,
 * from a counter-based hash shared bit-for-bit with oracle/fold_ref.c.
 */
int fjagg_fill_synth(int dtype, void* x_dev, int64_t ld, int64_t K, int64_t P, int64_t k0,
                     uint64_t seed, float amp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FJAGG_H_ */
