/*
 * tzrec_hip.h -- C ABI of libtzrec_hip.so, the MI355X (gfx950) sharded-embedding hot path
 * for TorchEasyRec (tzrec).
 *
 * This header is the drop-in boundary ("kernel-level seam").  Every entry
 * point replaces one call the reference makes into an un-vendored native wheel (fbgemm-gpu 1.7.0 /
 * torchrec 1.7.0, pinned in /root/reference/requirements/runtime.txt) or one pure-PyTorch module of
 * the reference.  The reference call site that reaches each op is cited next to it
 * (paths relative to /root/reference).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every `d_*` pointer is DEVICE memory; `h_*` is host memory read during the call only.
 *   - `stream` is a hipStream_t passed as void*; every launch is asynchronous on it.
 *   - no allocation inside: scratch comes from the caller (`ws`, sized by the matching
 *     `*_workspace` query, 256-byte aligned).
 *   - return 0 (TZR_OK) or a negative TZR_ERR_* code; never throws, never syncs the device.
 *   - thread-compatible: one caller thread per device (the reference runs one Python thread per
 *     rank, tzrec/utils/dist_util.py:57-75).
 *
 * Jagged input contract = torchrec KeyedJaggedTensor as tzrec builds it
 * (tzrec/datasets/data_parser.py:576-585): `values` int64[N] concatenated key-major then
 * sample-major, `lengths` per (key, sample) key-major, stride = B, `offsets` = [0] + cumsum(lengths)
 * (int64[F*B+1]), optional per-id float `weights`.
 */
#ifndef TZREC_HIP_H_
#define TZREC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TZR_DT_F32 0
#define TZR_DT_F16 1

#define TZR_OK 0
#define TZR_ERR_INVALID (-1)     /* bad argument (null pointer, negative size, unsupported dim) */
#define TZR_ERR_LAUNCH (-2)      /* hipLaunch / hipMemsetAsync reported an error */
#define TZR_ERR_WORKSPACE (-3)   /* workspace too small or misaligned */
#define TZR_ERR_UNSUPPORTED (-4) /* valid request this build has no kernel for */

#define TZR_MAX_DST 8      /* destination (feature-group) buffers per pooled lookup */
#define TZR_MAX_FEAT_DST 4 /* feature groups one feature may be copied into */

#define TZR_POOL_SUM 0
#define TZR_POOL_MEAN 1

#define TZR_OPT_SGD 0
#define TZR_OPT_ADAGRAD 1         /* elementwise state  [rows, D]  (torchrec.optim Adagrad) */
#define TZR_OPT_ROWWISE_ADAGRAD 2 /* one scalar per row [rows]     (RowWiseAdagrad)         */
#define TZR_OPT_ADAM 4            /* elementwise exp_avg | exp_avg_sq [rows, 2 D] (torchrec.optim Adam):
                                     state row = [m(D) | v(D)], m_stride >= 2 D             */
#define TZR_OPT_ACCUMULATE 3      /* no update: the summed gradient of every touched row is
                                     written to TzrTable.m (dense float [rows, dim]); used for
                                     replicated (data_parallel) tables before the all-reduce  */
/* The norm-based and partial row-wise kinds (fbgemm split-TBE optimizer templates [upstream]).  Per touched
 * row, on g = the row's summed (clipped) gradient, w = its weights before the update (fp32), lr = *d_lr,
 * c1 = 1 - beta1^t and c2 = 1 - beta2^t from d_adam, wd = weight_decay, |.| = the L2 norm over the
 * row's D columns (a column-wise shard: its own columns):
 *   PARTIAL_ROWWISE_ADAM: v = b2 v + (1-b2) mean_d(g^2) (one scalar), m = b1 m + (1-b1) g,
 *                         w -= lr ((m/c1) / (sqrt(v/c2) + eps) + wd w)
 *   LAMB:                 m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2,
 *                         u = (m/c1) / (sqrt(v/c2) + eps) + wd w, r = |w| / |u|, w -= lr r u
 *   PARTIAL_ROWWISE_LAMB: v as PARTIAL_ROWWISE_ADAM, m, u, r and w as LAMB
 *   LARS_SGD:             lambda = lr eta |w| / (|g| + wd |w|), m = mu m + lambda (g + wd w), w -= m
 *                         (mu = TzrSparseOptim.beta1, eta = TzrSparseOptim.beta2)
 * r = 0 when |u| = 0 and lambda = 0 when its denominator is 0: the term each multiplies is 0 exactly then,
 * so no row turns NaN -- and under the two LAMB kinds a row whose weights are all zero does not move.
 * Kinds 5-7 need d_adam and are advanced by tzr_sparse_adam_tick like TZR_OPT_ADAM.  State rows:
 *   5, 7: [m(D) | v | 3 floats of padding], m_stride = D + 4 (float4 aligned, one state row per weight row)
 *   6:    [m(D) | v(D)], m_stride >= 2 D          8: [m(D)], m_stride >= D
 * The entry points receive the TzrTable records as a device array and do NOT check m_stride against these rules: the
 * caller must (the Python layer does, embedding.check_state_stride).                                            */
#define TZR_OPT_PARTIAL_ROWWISE_ADAM 5
#define TZR_OPT_LAMB 6
#define TZR_OPT_PARTIAL_ROWWISE_LAMB 7
#define TZR_OPT_LARS_SGD 8
/* The two elementwise kinds without a step counter: "lazy" torch.optim.Adadelta / torch.optim.RMSprop (momentum 0, not
 * centered), the relation the kinds above have to their dense namesakes: a row is updated only in a step that looks it up,
 * a row nobody looked up keeps weights AND state (no decay of the running averages).  fbgemm has no public kernel for
 * either, so these formulas are the definition.  Per touched row, g, w, lr and wd as above:
 *   g = g + wd w                                          (L2 as torch, after clipping; weight_decay_mode is not read)
 *   RMSPROP:   s = alpha s + (1-alpha) g^2,               w -= lr g / (sqrt(s) + eps)
 *   ADADELTA:  s = rho s + (1-rho) g^2,  d = sqrt(a + eps) / sqrt(s + eps) g,  a = rho a + (1-rho) d^2,  w -= lr d
 * rho / alpha = TzrSparseOptim.beta1 (beta2 is not read), eps = TzrSparseOptim.eps and must be > 0 (TZR_ERR_INVALID
 * otherwise: with g = 0 both updates are 0 / eps-terms, exactly 0, so a touched row with a zero gradient does not move).
 * Neither kind has a step: d_adam must be 0 and tzr_sparse_adam_tick is not called.  A call that passes a step state asks
 * for a stepped (bias-corrected) variant this build has no kernel for: TZR_ERR_UNSUPPORTED, which is also what such a call
 * got from version 15 before these kinds existed.  State rows, fp32, zero at the start:
 *   9:  [s(D) | a(D)], m_stride >= 2 D (Adam's layout)      10: [s(D)], m_stride >= D (Adagrad's split layout)
 * Kinds 9 and 10 are new VALUES of an existing field: no struct, entry point or meaning of an older value changes, so the
 * ABI version stays 15 (a library of version 15 built before them answers TZR_ERR_UNSUPPORTED).                      */
#define TZR_OPT_ADADELTA 9
#define TZR_OPT_RMSPROP 10

#define TZR_WD_NONE 0
#define TZR_WD_L2 1
#define TZR_WD_DECOUPLE 2

#define TZR_BOUNDS_FATAL 0   /* count out-of-range ids, leave them (caller raises)   */
#define TZR_BOUNDS_WARNING 1 /* count and clamp to row 0 (fbgemm default [upstream]) */
#define TZR_BOUNDS_IGNORE 2  /* clamp silently                                        */

/* One embedding table shard resident in HBM.  Replaces the fbgemm TBE weight/optimizer-state
 * buffers (tzrec/optim/optimizer.py:106-255).  `w`/`m` are device addresses of row 0; a row is
 * `dim` floats, rows are `*_stride` floats apart (stride 2*dim with m = w + dim gives the
 * interleaved [w|m] 128-byte row used for Adagrad at dim 16). */
typedef struct TzrTable {
  uint64_t w;       /* device address of weights row 0: float* or, w_dtype = TZR_DT_F16, half*  */
  uint64_t m;       /* float* device address of optimizer state row 0 (0 for SGD)             */
  int64_t rows;     /* rows held by this shard                                                */
  int32_t dim;      /* embedding dim D (multiple of 4, <= 256)                                */
  int32_t w_stride; /* ELEMENTS (floats / halves) between consecutive weight rows               */
  int32_t m_stride; /* floats between consecutive state rows (rowwise adagrad: 1)             */
  int32_t first_order; /* smallest TzrFeature.order among the keys reading this table         */
  int32_t n_feats;  /* number of KJT keys reading this table (their orders are consecutive)   */
  int32_t w_dtype;  /* TZR_DT_F32 | TZR_DT_F16 (tzrec feature config `data_type`,
                       tzrec/features/feature.py:346-356,626): half weights are widened to fp32
                       on read; the fused optimizer computes in fp32 and rounds to nearest even
                       on write; optimizer state is always fp32                              */
} TzrTable; /* 48 bytes */

/* One lookup = (KJT key -> table).  Usually one per key; a key read through two tables (DeepFM:
 * `cat_0` feeds `cat_0_emb` for the fm/deep groups and `cat_0_emb_wide` for the wide group,
 * tzrec/modules/embedding.py:744-745,777-786) has one TzrFeature per table.  `dst`/`col` say
 * where its pooled [B, dim] block lands: feature groups sharing a lookup (DeepFM `fm` and `deep`,
 * embedding.py:972-976) each get a copy, and the backward sums the groups' gradients. */
typedef struct TzrFeature {
  int32_t table;   /* index into the TzrTable array                                           */
  int32_t key;     /* KJT key index: bag (key, b) is offsets[key*B + b] .. offsets[key*B+b+1]   */
  int32_t pooling; /* TZR_POOL_SUM / TZR_POOL_MEAN (tzrec/features/feature.py:586-591)         */
  int32_t n_dst;   /* 1..TZR_MAX_FEAT_DST                                                      */
  int32_t dst[TZR_MAX_FEAT_DST]; /* destination buffer index                                   */
  int32_t col[TZR_MAX_FEAT_DST]; /* first float column inside that buffer (multiple of 4)      */
  int32_t order;   /* rank of this lookup when lookups are sorted by (table, index): the
                      table-major order the backward plan groups ids in.  A table is read at
                      most once per key.                                                       */
  int32_t reserved[3];
} TzrFeature; /* 64 bytes */

/* One float4 of one destination row: the forward kernel walks slots so that consecutive lanes
 * write consecutive float4s of a destination row (fuses fbgemm permute_pooled_embs /
 * KeyedTensor.regroup_as_dict, tzrec/modules/embedding.py:972-976). */
typedef struct TzrSlot {
  int32_t feature; /* KJT key index                                                            */
  int32_t chunk;   /* float4 index inside the embedding row                                    */
  int32_t dst;     /* destination buffer index                                                 */
  int32_t col;     /* float column in the destination buffer                                   */
} TzrSlot; /* 16 bytes */

/* Destination / gradient buffer of one feature group: float [B, stride]. */
typedef struct TzrDst {
  uint64_t ptr;   /* float* device address                                                     */
  int64_t stride; /* floats between consecutive samples (multiple of 4)                        */
} TzrDst;

/* Fused sparse optimizer applied inside the backward (tzrec/main.py:774-781,
 * tzrec/optim/optimizer_builder.py:30-97, protos/optimizer.proto:76-139). */
typedef struct TzrSparseOptim {
  int32_t kind;              /* TZR_OPT_*                                                       */
  int32_t weight_decay_mode; /* TZR_WD_* (rowwise adagrad only)                                 */
  uint64_t d_lr;             /* const float* DEVICE scalar: schedulers mutate it per step
                                (tzrec/main.py:877-879); graph-replay safe                      */
  float eps;                 /* fbgemm default 1e-8 [upstream]; not configurable from tzrec --
                                except kinds 9, 10: their proto field (1e-6 / 1e-8), must be > 0  */
  float weight_decay;
  float max_gradient;        /* used when gradient_clipping != 0                                */
  int32_t gradient_clipping;
  float beta1;               /* TZR_OPT_ADAM and kinds 5-7 (protos/optimizer.proto:89-96);
                                TZR_OPT_LARS_SGD: the momentum mu; TZR_OPT_ADADELTA: rho;
                                TZR_OPT_RMSPROP: alpha                                          */
  float beta2;               /* TZR_OPT_LARS_SGD: the trust coefficient eta (fbgemm default 0.001) */
  uint64_t d_adam;           /* TZR_OPT_ADAM, kinds 5-7: float[4] DEVICE state {step, 1 - beta1^step,
                                1 - beta2^step, -}, advanced once per training step by
                                tzr_sparse_adam_tick (graph-replay safe)                        */
} TzrSparseOptim; /* 48 bytes */

/* Sparse Adam step counter: d_adam[0] += 1, d_adam[1] = 1 - beta1^step, d_adam[2] = 1 - beta2^step.
 * Call once per training step BEFORE the step's tzr_pooled_bwd_apply / tzr_dense_rows_update calls
 * (fbgemm's `iter`, incremented once per step [upstream]). */
int tzr_sparse_adam_tick(float* d_adam, float beta1, float beta2, void* stream);

/* ---- library identity ------------------------------------------------------------------- */
const char* tzr_backend(void); /* "hip-gfx950" (the CPU lane emulator used by tests says "emu") */
int tzr_abi_version(void);

/* ---- index stage (integer, bit-exact) ---------------------------------------------------- */

/* K3: lengths -> offsets (exclusive scan, offsets[n] = total).  Replaces fbgemm
 * asynchronous_complete_cumsum reached from KeyedJaggedTensor.offsets()
 * (tzrec/modules/embedding.py:930).  lengths_itemsize is 4 (int32) or 8 (int64). */
size_t tzr_lengths_to_offsets_workspace(int64_t n);
int tzr_lengths_to_offsets(const void* d_lengths, int lengths_itemsize, int64_t n,
                           int64_t* d_offsets, void* ws, size_t ws_bytes, void* stream);

/* K4: bounds check of every id against its table's row count.  Replaces fbgemm
 * bounds_check_indices (mode from ParameterConstraints.bounds_check_mode,
 * tzrec/utils/plan_util.py:580,594).  d_oob_count (int64[1]) is incremented per bad id;
 * WARNING/IGNORE clamp the id to 0 in place. */
int tzr_bounds_check(const TzrTable* d_tables, const TzrFeature* d_feats, int n_feats,
                     int64_t* d_values, const int64_t* d_offsets, int64_t B, int mode,
                     int64_t* d_oob_count, void* stream);

/* K1: KJT permute.  Replaces fbgemm permute_2D_sparse_data reached from the sharded
 * input_dist (tzrec/modules/embedding.py:930 -> torchrec KJT.permute [upstream]).
 * out key t takes input key permute[t] (T output keys, F input keys, repeats allowed).
 * d_in_offsets is int64[F*B+1]; d_out_offsets (int64[T*B+1]) and d_out_lengths are written;
 * d_out_values / d_out_weights must hold the permuted total (<= caller's bound n_out_max). */
size_t tzr_kjt_permute_workspace(int64_t T, int64_t B);
int tzr_kjt_permute(const int32_t* d_permute, int T, int F, int64_t B,
                    const void* d_in_lengths, int lengths_itemsize, const int64_t* d_in_offsets,
                    const int64_t* d_in_values, const float* d_in_weights,
                    void* d_out_lengths, int64_t* d_out_offsets, int64_t* d_out_values,
                    float* d_out_weights, int64_t n_out_max, void* ws, size_t ws_bytes,
                    void* stream);

/* K2: row-wise bucketize.  Replaces fbgemm block_bucketize_sparse_features (row-wise sharded
 * tables; RW geometry = contiguous ceil(rows/W) blocks, tzrec/utils/plan_util.py:
 * 1049-1060 -> torchrec calculate_shard_sizes_and_offsets [upstream]).  For id x of key f:
 * dst = x / block_size[f] (clamped to W-1), local = x - dst*block_size[f].  Output is
 * rank-major: new_lengths[(r*F + f)*B + b]; ids keep their relative order inside each
 * (r, f, b) bag.  d_unbucketize_permute[i] = output position of input id i (nullable).
 * d_rank_offsets (nullable, int32[F]) rotates the owner: dst = (offset[f] + x / block_size[f]) mod W,
 * which spreads tables with fewer rows than ranks (and table-wise placement: block_size = rows,
 * offset = owner) over the node instead of piling them on rank 0.
 * block_size[f] == 0 selects hash routing for key f: dst = splitmix64(x) mod W and the id travels
 * unchanged (zero-collision-hash tables, whose owners map raw ids to rows themselves). */
size_t tzr_block_bucketize_workspace(int64_t F, int64_t B, int W);
int tzr_block_bucketize(const int64_t* d_block_sizes, const int32_t* d_rank_offsets, int F,
                        int64_t B, int W,
                        const int64_t* d_offsets, const int64_t* d_values, const float* d_weights,
                        int64_t n_values, void* d_new_lengths, int lengths_itemsize,
                        int64_t* d_new_offsets, int64_t* d_new_values, float* d_new_weights,
                        int64_t* d_unbucketize_permute, void* ws, size_t ws_bytes, void* stream);

/* Requester side of the sharded exchange for a KJT whose bags all hold `bag_len` ids (Criteo: 1):
 * K1 + K2 restricted to what the id-granularity exchange consumes, in 3 launches instead of 13.
 * For the n_sel selected keys (d_sel[f'] = KJT key index; block size / rank offset per selected key
 * as in tzr_block_bucketize, block size 0 = hash routing):
 *   d_out_ids[N']       local ids grouped by (owner rank, selected key), lookup order inside a group
 *   d_unbucketize[N']   position in d_out_ids of lookup j of selected key f' at index f'*B*bag_len + j
 *   d_counts[W*n_sel]   ids per (rank, key), rank-major (what the counts all-to-all sends)
 * with N' = n_sel * B * bag_len.  W <= 64 and W * n_sel <= 256 in this build.  Same results as
 * tzr_kjt_permute + tzr_block_bucketize (tests compare them). */
size_t tzr_exchange_bucketize_workspace(int n_sel, int64_t n_per_key, int W);
int tzr_exchange_bucketize(const int32_t* d_sel, int n_sel, const int64_t* d_block_sizes,
                           const int32_t* d_rank_offsets, int64_t B, int bag_len, int W,
                           const int64_t* d_values, int64_t* d_out_ids, int64_t* d_unbucketize,
                           int64_t* d_counts, void* ws, size_t ws_bytes, void* stream);

/* Capacity-bounded form of the same (the reference's input dist is torchrec's KJTAllToAll reached
 * from TrainPipelineSparseDist, tzrec/utils/dist_util.py:221-303, whose split sizes cross the host every step):
 * every destination rank owns a FIXED slice of `d_message`, so the ids all-to-all has equal splits known
 * without reading anything back, and the whole sharded step keeps static shapes.
 *   S = tzr_exchange_message_stride(n_sel, capacity) = n_sel + 1 + capacity   (int64 words per destination)
 *   d_message[d*S + f']          ids of selected key f' sent to rank d (clamped to what fits)
 *   d_message[d*S + n_sel]       1 if this rank had to DROP ids for any destination, else 0
 *   d_message[d*S + n_sel+1 ..]  the ids, grouped by key, lookup order inside a key
 *   d_unbucketize[N']            position (in words from the start of d_message) of every lookup's id; a
 *                                dropped lookup points at its destination's first id slot
 * A step whose overflow word is set anywhere must be redone through the exact exchange (the caller checks the
 * flag tzr_exchange_owner_segments returns before it uses anything computed from the message). */
int64_t tzr_exchange_message_stride(int n_sel, int64_t capacity);
int tzr_exchange_bucketize_capped(const int32_t* d_sel, int n_sel, const int64_t* d_block_sizes,
                                  const int32_t* d_rank_offsets, int64_t B, int bag_len, int W,
                                  const int64_t* d_values, int64_t capacity, int64_t* d_message,
                                  int64_t* d_unbucketize, void* ws, size_t ws_bytes, void* stream);
/* The same layout from a DENSE bucketize result (ragged / weighted bags: tzr_block_bucketize): d_counts[W*n_sel] ids per
 * (rank, key), d_ids[n_ids] rank-major, d_unbucketize[n_ids] = dense position of every lookup -> d_message as above and
 * d_unbucketize_out[n_ids] = message position of every lookup (may alias d_unbucketize). */
int tzr_exchange_pad(const int64_t* d_counts, int W, int n_sel, int64_t capacity, const int64_t* d_ids,
                     const int64_t* d_unbucketize, int64_t n_ids, int64_t* d_message,
                     int64_t* d_unbucketize_out, void* stream);
/* Owner side: the received message (W slices of S words, source-rank major) -> key segments over its W*S
 * positions for tzr_rows_gather / tzr_pooled_bwd_plan / _apply (ids pointer = d_message itself):
 *   key s*(n_sel+1)          dead (the words before rank s's ids: unused capacity of rank s-1 + the header)
 *   key s*(n_sel+1) + 1 + f' the ids of selected key f' from rank s
 *   key W*(n_sel+1)          dead (unused capacity of the last rank)
 * d_key_start: int64[W*(n_sel+1) + 2].  *d_overflow = 1 when any source rank dropped ids. */
int tzr_exchange_owner_segments(const int64_t* d_message, int W, int n_sel, int64_t capacity,
                                int64_t* d_key_start, int64_t* d_overflow, void* stream);

/* ---- pooled embedding lookup ------------------------------------------------------------- */

/* K5 (+K8 fused): pooled gather forward.  Replaces torchrec EmbeddingBagCollection.forward ->
 * fbgemm split_embedding_codegen_forward_{un,}weighted (self.ebc(kjt),
 * tzrec/modules/embedding.py:930) and the regroup copy (:972-976):
 *   dst[g][b, col_f : col_f+D_f] = sum_{i in bag(f,b)} weight_i * W_t[id_i, :]   (mean: / len)
 * Empty bag -> zeros.  h_dsts: host array of n_dst destination buffers.  d_slots enumerates every
 * float4 of every destination row exactly once, in destination-then-column order. */
int tzr_pooled_fwd(const TzrTable* d_tables, const TzrFeature* d_feats, int n_feats,
                   const TzrSlot* d_slots, int n_slots, const int64_t* d_values,
                   const int64_t* d_offsets, const float* d_weights, int64_t B,
                   const TzrDst* h_dsts, int n_dst, int uniform_bag_len, void* stream);
/* Same, with flags.  TZR_FWD_MIXED_DTYPE: some table holds fp16 rows (TzrTable.w_dtype); without
 * the flag (and in tzr_pooled_fwd) every table is read as fp32. */
#define TZR_FWD_MIXED_DTYPE 1
int tzr_pooled_fwd_ex(const TzrTable* d_tables, const TzrFeature* d_feats, int n_feats,
                      const TzrSlot* d_slots, int n_slots, const int64_t* d_values,
                      const int64_t* d_offsets, const float* d_weights, int64_t B,
                      const TzrDst* h_dsts, int n_dst, int uniform_bag_len, int flags, void* stream);

/* K6: backward index plan = group the N lookups by (table, row), duplicates adjacent, original
 * order kept inside a row (stable segmented radix sort).  Replaces fbgemm
 * transpose_embedding_input (linearize + cub radix sort + run-length) reached from the autograd
 * of self.ebc(kjt).  Depends only on the ids, so it can run ahead of the forward on another
 * stream.  The plan lives in `ws` and is consumed by tzr_pooled_bwd_apply. */
size_t tzr_pooled_bwd_workspace(int64_t n_values, int64_t n_positions, int n_feats, int n_tables,
                                int64_t B,
                                int max_dim);
int tzr_pooled_bwd_plan(const TzrTable* d_tables, int n_tables, const TzrFeature* d_feats,
                        int n_feats, int n_keys, int64_t max_rows, int max_dim, const int64_t* d_values,
                        const int64_t* d_offsets, int64_t n_values, int64_t n_positions,
                        int64_t B,
                        int uniform_bag_len, void* ws, size_t ws_bytes, void* stream);

/* K6 + K7 in ONE launch, no index plan: the small-batch form of the fused backward (csrc/pooled_bwd_direct.hip).
 * Same semantics and argument meaning as tzr_pooled_bwd_plan followed by tzr_pooled_bwd_apply -- per distinct (table, row)
 * of the batch ONE update with the sum of its lookups' gradients, summation order a function of the ids alone -- for
 * batches whose per-table id lists are small enough to be read by every workgroup of the table (a rank's 8 192-sample
 * share of examples/dlrm_criteo.config: 213 k lookups).  Workgroup (t, j) owns the j-th of k equal row ranges of table t,
 * reads all ids of t, keeps its own in LDS, sorts, reduces, applies; the rows of a tiny table are split over several
 * workgroups by position instead.  Cost grows with (lookups per table)^2 / 256: tzr_pooled_bwd_direct_supported says
 * whether a batch should take this entry -- 0 for shapes it refuses (TZR_ERR_UNSUPPORTED: more than 256 lookups or tables,
 * ragged pooled bags = grad_mode 0 with uniform_bag_len != 1) and for more than 16 384 lookups per table on average
 * (tzr_tune "bwd_direct": 1 = any size, -1 = never); callers take the planned pair then.  Replaces the same fbgemm pieces
 * as the pair (transpose_embedding_input + split_embedding_backward_codegen_*_exact, tzrec/modules/embedding.py:930,
 * tzrec/main.py:774-781).
 * grad_mode | TZR_GRAD_HOT_ROWS: the caller expects a row with more lookups than fit a workgroup's LDS (1 280) -- the shared
 * row of a zero-collision hash's unseen ids (tzrec/features/feature.py:693-736: row zch_size - 1), a default id: such a row,
 * when it is the mode of the table's first 16 ids, is summed by ALL of the table's workgroups (a slice of the positions each,
 * partial sums added in slice order) instead of by its range's workgroup alone (140 -> 45 us at 8 192 lookups, 95 % on one
 * row).  Without the flag, or when the sample misses, the row is still handled correctly, only slower.
 * `ws`: tzr_pooled_bwd_direct_workspace bytes, ZERO-FILLED by the caller before its first use (arrival counters of the
 * workgroups that share a row of a tiny table; every launch leaves them zero, so the buffer can be kept and reused --
 * one buffer per stream of launches). */
#define TZR_GRAD_HOT_ROWS 0x100
int tzr_pooled_bwd_direct_supported(int64_t n_positions, int n_feats, int n_tables, int uniform_bag_len,
                                    int grad_mode);
size_t tzr_pooled_bwd_direct_workspace(int64_t n_positions, int n_tables, int max_dim);
int tzr_pooled_bwd_direct(const TzrTable* d_tables, int n_tables, const TzrFeature* d_feats, int n_feats,
                          int64_t max_rows, int max_dim, const int64_t* d_values, const int64_t* d_offsets,
                          const float* d_weights, int64_t n_values, int64_t n_positions, int64_t B,
                          int uniform_bag_len, int grad_mode, const TzrDst* h_grads, int n_dst,
                          const TzrSparseOptim* h_optim, void* ws, size_t ws_bytes, void* stream);

/* Inspection of a finished plan (tests / debugging): byte offsets into `ws` of out8[0] = the sorted
 * {row, lookup position} pairs (uint32 x 2 per table-major position) of every table with more than
 * 512 rows, out8[1] = the bucket-partitioned pairs (final for tables of <= 512 rows), out8[2] = the
 * table-major start of every lookup by order (uint32[n_feats + 1]); out8[3..7] internal.  After a
 * plan, the pairs of one table hold every lookup of the table exactly once with equal rows adjacent
 * and, inside a row, ascending lookup positions. */
int tzr_pooled_bwd_plan_view(int64_t n_values, int64_t n_positions, int n_feats, int n_tables,
                             int max_dim, int64_t* out8);

/* K7: fused backward + sparse optimizer.  Replaces fbgemm
 * split_embedding_backward_codegen_{sgd,adagrad,rowwise_adagrad}_*_exact (optimizer fused into
 * backward by apply_optimizer_in_backward, tzrec/main.py:774-781): per distinct (table,row)
 * g = sum over its duplicate lookups (in original lookup order) of weight_i * dL/d(pooled bag),
 * summed over the feature groups the feature was copied into; then ONE update of the row:
 *   adagrad          m += g*g;            w -= lr * g / (sqrt(m) + eps)
 *   rowwise adagrad  m += mean_d(g*g);    w -= lr * g / (sqrt(m) + eps)
 *   sgd              w -= lr * g
 * grad_mode 0: h_grads mirrors the forward's h_dsts (same buffer indices / strides).
 * grad_mode 1: h_grads[0] is float [n_values, stride], ONE gradient row per id (indexed by the id's
 * position in `values`): the owner side of the sharded exchange. */
int tzr_pooled_bwd_apply(const TzrTable* d_tables, const TzrFeature* d_feats, int n_feats,
                         int n_tables, int max_dim, const int64_t* d_offsets,
                         const float* d_weights, int64_t n_values, int64_t n_positions, int64_t B,
                         int uniform_bag_len, int grad_mode, const TzrDst* h_grads, int n_dst,
                         const TzrSparseOptim* h_optim, void* ws, size_t ws_bytes, void* stream);

/* K6 / K7 in the "cells" form (csrc/pooled_bwd_cells.hip): the index plan as ONE launch for batches of exactly one id per
 * bag -- the shape of examples/dlrm_criteo.config -- and the apply that reads it.  Same reference pieces replaced as
 * tzr_pooled_bwd_plan / _apply (fbgemm transpose_embedding_input + split_embedding_backward_codegen_*_exact behind
 * tzrec/modules/embedding.py:930, tzrec/main.py:774-781), same semantics: per distinct (table, row) the gradient rows of
 * its lookups added in lookup-position order, one update (the grouping of the partial sums follows each plan's own unit
 * boundaries: the two plans agree to fp32 rounding, each is bit-reproducible).  The plan only orders every chunk of <= 1024 lookups by
 * bucket in place and notes the chunk's bucket starts (no histogram, no scan, no communication between workgroups); a unit of
 * the apply gathers the cells of its bucket range from the chunks and sorts them in LDS.  Which unit reads which cells is a
 * function of the tables and B alone: tzr_bwd_cells_geometry builds that description ON THE HOST, once; the caller keeps a
 * device copy (256-byte aligned; the kernels write its tail: partial-sum records, arrival counters, the overflow word) and
 * hands both to the two calls.
 *   tzr_bwd_cells_geometry: h_tables / h_feats = HOST copies of the arrays the device calls get.  h_out == NULL: sizes only.
 *     out_info8: [0] bytes of the image, [1] chunks, [2] units, [3] table-major positions, [4] positions per chunk,
 *     [5] partial-sum records, [6] byte offset of the overflow word (uint32) inside the image.  TZR_ERR_UNSUPPORTED: not a
 *     case for this plan (a table with more than 256 chunks of lookups, an empty batch): take tzr_pooled_bwd_plan.
 *   Unit sizes are expectations for evenly drawn ids (~1024 of a capacity of 1 280).  A unit that holds more is still updated
 *     correctly -- row by row, without the LDS sort, slowly -- and counted in the overflow word, never reset by the library: a
 *     caller that sees it move sends this id distribution to tzr_pooled_bwd_plan, whose heavy-bucket machinery is made for it.
 *   `ws`: tzr_pooled_bwd_workspace bytes (one size serves either plan).  d_weights: per-id weights or NULL. */
int tzr_bwd_cells_geometry(const TzrTable* h_tables, int n_tables, const TzrFeature* h_feats, int n_feats, int64_t B,
                           int max_dim, void* h_out, size_t out_bytes, int64_t* out_info8);
int tzr_pooled_bwd_cells_plan(const TzrTable* d_tables, int n_tables, const TzrFeature* d_feats, int n_feats, int max_dim,
                              const int64_t* d_values, int64_t n_values, int64_t B, const void* h_geo, void* d_geo, void* ws,
                              size_t ws_bytes, void* stream);
/* The forward and the cells plan of the SAME batch as one launch: tzr_pooled_fwd (one id per bag, fp32 tables, no per-sample
 * weights; d_ftables / d_ffeats / d_slots / h_dsts as there) + tzr_pooled_bwd_cells_plan (the other arguments as there).  The
 * plan needs only the ids, and its work is LDS / ALU work while the forward is bound by its 64-byte row requests: the plan's
 * workgroups follow the forward's in ONE grid and run in the slots those leave (seven workgroups of either kind per CU), which
 * hides all but ~2 us of the plan's 15; results are those of the two calls, bit for bit (each workgroup runs the same code on
 * the same data).  tzr_pooled_fwd_cells_plan_supported == 0 / TZR_ERR_UNSUPPORTED: not a case for it (more than
 * 128 slots, B < 32 768, tzr_tune "fwd_plan" 0) -- make the two calls.  In the reference both halves sit behind self.ebc(kjt)
 * and its autograd (tzrec/modules/embedding.py:930; fbgemm's transpose_embedding_input runs at backward time). */
int tzr_pooled_fwd_cells_plan_supported(int n_slots, int64_t B);
int tzr_pooled_fwd_cells_plan(const TzrTable* d_ftables, const TzrFeature* d_ffeats, int n_ffeats, const TzrSlot* d_slots,
                              int n_slots, const TzrDst* h_dsts, int n_dst, const TzrTable* d_tables, int n_tables,
                              const TzrFeature* d_feats, int n_feats, int max_dim, const int64_t* d_values, int64_t n_values,
                              int64_t B, const void* h_geo, void* d_geo, void* ws, size_t ws_bytes, void* stream);
int tzr_pooled_bwd_cells_apply(const TzrTable* d_tables, const TzrFeature* d_feats, int n_feats, int n_tables, int max_dim,
                               const float* d_weights, int64_t n_values, int64_t B, int grad_mode, const TzrDst* h_grads,
                               int n_dst, const TzrSparseOptim* h_optim, const void* h_geo, void* d_geo, void* ws,
                               size_t ws_bytes, void* stream);

/* Dense update of replicated (data_parallel) tables after their accumulated row gradients were
 * all-reduced: for every row r of every table t with a non-zero gradient
 * g = d_acc[(d_row_start[t] + r) * dim ...], apply h_optim exactly like K7 does for one row.  Rows
 * whose gradient is all zero are left untouched (a sparse update never visits them). */
int tzr_dense_rows_update(const TzrTable* d_tables, int n_tables, const int64_t* d_row_start,
                          int64_t total_rows, const float* d_acc, int dim,
                          const TzrSparseOptim* h_optim, void* stream);
/* Same, and the rows of d_acc it applied are zero afterwards: the accumulation buffer is ready for the next step's
 * TZR_OPT_ACCUMULATE pass (which writes only the rows it touches) without a memset launch in front of it. */
int tzr_dense_rows_update_clear(const TzrTable* d_tables, int n_tables, const int64_t* d_row_start,
                                int64_t total_rows, float* d_acc, int dim, const TzrSparseOptim* h_optim,
                                void* stream);

/* ---- row-wise sharded exchange (one process per GPU, RCCL all-to-all between the stages) ---- */

/* Owner side forward: out[j, 0:dim] = W_{table of key(j)}[ids[j], :] for j in [0, n_ids); ids
 * arrive grouped by key, key k owning positions d_key_start[k] .. d_key_start[k+1] (device,
 * int64[n_keys+1]); d_key_table[k] indexes d_tables (< 0: a dead key, its output rows are left
 * untouched).  Replaces the per-shard TBE lookup of
 * torchrec's row-wise sharded EBC [upstream]; one row per id instead of a pooled partial per bag. */
int tzr_rows_gather(const TzrTable* d_tables, const int32_t* d_key_table,
                    const int64_t* d_key_start, int n_keys, const int64_t* d_ids, int64_t n_ids,
                    float* d_out, int64_t out_stride, int dim, void* stream);

/* Requester side backward: d_out[pos(i), 0:dim] = weight_i (/ len for mean) * sum over the feature
 * groups of key f of grad[g][b, col_g(f) : +dim] for every id i of bag (f, b); pos(i) =
 * d_positions[i] (the unbucketize permute) or i when null. */
int tzr_lookup_grads(const TzrFeature* d_feats, int n_feats, const int64_t* d_offsets,
                     const float* d_weights, int64_t B, int uniform_bag_len,
                     const int64_t* d_positions, const TzrDst* h_grads, int n_dst, float* d_out,
                     int64_t out_stride, int dim, void* stream);

/* ---- dense glue of the training step -------------------------------------------------------- */

/* BCEWithLogitsLoss(reduction="mean") and its gradient in two launches (elementwise + partial
 * sums, fixed-order finish).  Replaces the
 * torch.nn.BCEWithLogitsLoss forward+backward built by tzrec/models/rank_model.py:190-191,233-240
 * (with sample weights: mean(loss_i * w_i), rank_model.py:260-273, w_i already normalised by the
 * caller).  *d_loss = mean_i w_i*(max(x,0) - x*y + log1p(exp(-|x|))); d_grad_logits[i] =
 * w_i*(sigmoid(x_i) - y_i)/B.  Labels: float32 (labels_are_float=1) or int32/int64. */
size_t tzr_bce_logits_workspace(int64_t B);
int tzr_bce_logits(const float* d_logits, const void* d_labels, int labels_itemsize,
                   int labels_are_float, const float* d_sample_weight, int64_t B, float* d_loss,
                   float* d_grad_logits, void* ws, size_t ws_bytes, void* stream);

/* ---- the losses a config names (csrc/loss_ops.hip) --------------------------------------------------------------------
 * tzrec/protos/loss.proto:44-63 as tzrec/models/rank_model.py:181-262 and multi_task_rank.py:97-142 combine them with the
 * sample weights.  Common to the three entry points:
 *   labels       d_labels with labels_itemsize / labels_are_float: float32, int32 or int64 (else TZR_ERR_UNSUPPORTED)
 *   row weights  w_i = d_weight[i] (1 when null) * (d_space_label[i] > 0 ? in_w : out_w) (1 when d_space_label is null;
 *                the task-space indicator label, typed by space_itemsize / space_is_float like the labels)
 *   *d_loss      = task_weight * sum_i(w_i l_i) / sum_i(w_i), 0 when sum_i(w_i) == 0 -- the reference's
 *                mean(l_i * w_i / mean(w)) * weight with div_no_nan; with neither weight input sum(w) is B exactly
 *   d_grad       d l_i / d logits, times w_i, NOT divided by the normaliser, and
 *   *d_scale     = task_weight / sum_i(w_i) (0 when the sum is 0): d(*d_loss)/d logits = d_grad * *d_scale, so that
 *                the autograd backward is one multiply by (grad_out * scale) with no host read
 * sum(w l) and sum(w) are two partial sums per workgroup, added in index order by a one-workgroup finishing launch: no
 * float atomics, the same inputs give the same bits.  No host sync (capturable).  Errors are found before anything is
 * launched and leave every output untouched: TZR_ERR_INVALID (null pointer, B <= 0, C < 2, unknown kind),
 * TZR_ERR_UNSUPPORTED (label width; B >= 2^30 for the two row-structured entries), TZR_ERR_WORKSPACE (null, not 256-byte
 * aligned, shorter than the matching *_workspace query). */
#define TZR_LOSS_BCE 0   /* p0 = label_smoothing s: y' = y (1 - s) + 0.5 s;  l = max(x,0) - x y' + log1p(exp(-|x|)), dl = sigmoid(x) - y' */
#define TZR_LOSS_FOCAL 1 /* p0 = gamma, p1 = alpha: f = alpha y (1-p)^gamma + (1-alpha)(1-y) p^gamma, p = sigmoid(x);  l = f * bce(x, y),
                            dl = f (p - y): f is a constant of the gradient (the reference detaches it, tzrec/loss/focal_loss.py:64-72) */
#define TZR_LOSS_L2 2    /* l = (x - y)^2, dl = 2 (x - y): nn.MSELoss on the prediction `y` */
size_t tzr_loss_pointwise_workspace(int64_t B);
int tzr_loss_pointwise(int kind, float p0, float p1, const float* d_logits, const void* d_labels, int labels_itemsize,
                       int labels_are_float, const float* d_weight, const void* d_space_label, int space_itemsize,
                       int space_is_float, float in_w, float out_w, float task_weight, int64_t B, float* d_loss,
                       float* d_grad, float* d_scale, void* ws, size_t ws_bytes, void* stream);

/* nn.CrossEntropyLoss(label_smoothing = eps) over d_logits [B, C] (row_stride floats between rows, unit column stride),
 * int32 / int64 labels (float labels: TZR_ERR_UNSUPPORTED):  l = (1 - eps)(-log p_y) + (eps / C) sum_c(-log p_c),  d_grad [B, C] contiguous = w (p - ((1 - eps) onehot
 * + eps / C)).  C <= 8: one lane per row, the row in registers; larger C: one wave per row, lanes stride over the classes.
 * A label outside [0, C) is never used as an index: its row has l = 0 and a zero gradient row (its weight still counts in
 * sum(w)) and *d_bad_labels (int64, the caller's to zero, may be null) goes up by one. */
size_t tzr_softmax_ce_workspace(int64_t B, int C);
int tzr_softmax_ce(const float* d_logits, int64_t row_stride, int C, const void* d_labels, int labels_itemsize,
                   int labels_are_float, float eps, const float* d_weight, const void* d_space_label, int space_itemsize,
                   int space_is_float, float in_w, float out_w, float task_weight, int64_t B, float* d_loss,
                   float* d_grad, float* d_scale, int64_t* d_bad_labels, void* ws, size_t ws_bytes, void* stream);

/* JRCLoss (tzrec/loss/jrc_loss.py, arXiv 2208.06164) grouped by session, O(B) memory instead of the reference's [B, B]
 * masks.  d_logits [B, 2] contiguous, l0 = [:, 0], l1 = [:, 1]; a row is positive when its label == 1.  For session s:
 * A_s = logsumexp of l1 over its negatives, B_s = logsumexp of l0 over its positives (-inf for an empty set).
 *   l_i = alpha CE_i + (1 - alpha) ge_i,  ge_i = softplus(A_s - l1_i) for a positive row, softplus(B_s - l0_i) otherwise
 * and the gradient of sum_i w_i l_i in closed form (q_i = sigmoid(A_s - l1_i), r_i = sigmoid(B_s - l0_i), P_s = sum over
 * positives of w q, Q_s = sum over negatives of w r): a positive row gets -w q on l1 and Q_s exp(l0 - B_s) on l0, a
 * negative row -w r on l0 and P_s exp(l1 - A_s) on l1.  The reference masks with -1e9 added in fp32, which excludes to
 * the last bit of an fp32 exp; here the rows are excluded.  A batch without a positive (or without a negative) row makes
 * the reference's mean form NaN (the mean of an empty tensor times 0); this entry returns the finite sum.
 * d_session int64 [B]; d_order int64 [B] = a stable argsort of d_session (the caller's sort).  One wave per 64 sorted
 * rows works through the session heads among them (neighbour compare; the end of the last one by binary search), three
 * sweeps per session with the lanes striding over its rows: a session of any length is correct, every gradient element
 * is written by exactly one lane.  Row losses go to a [B] buffer in ROW order and are summed by the fixed tree above: the
 * loss bits do not depend on how sessions are scheduled. */
size_t tzr_jrc_loss_workspace(int64_t B);
int tzr_jrc_loss(const float* d_logits, const void* d_labels, int labels_itemsize, int labels_are_float,
                 const int64_t* d_session, const int64_t* d_order, float alpha, const float* d_weight,
                 const void* d_space_label, int space_itemsize, int space_is_float, float in_w, float out_w,
                 float task_weight, int64_t B, float* d_loss, float* d_grad, float* d_scale, void* ws, size_t ws_bytes,
                 void* stream);

/* Backward of a Linear+ReLU layer up to the GEMMs: d_grad[b,n] = d_grad_y[b,n] * (d_y[b,n] > 0)
 * and d_colsum[n] = sum_b d_grad[b,n] (the bias gradient), one pass.  Replaces
 * threshold_backward + sum(0) in the autograd of tzrec/modules/mlp.py:37-177 (Perceptron =
 * Linear + ReLU).  N multiple of 4, <= 1024; strides in floats, multiples of 4. */
size_t tzr_relu_bwd_colsum_workspace(int64_t B, int N);
int tzr_relu_bwd_colsum(const float* d_grad_y, int64_t grad_y_stride, const float* d_y,
                        int64_t y_stride, int64_t B, int N, float* d_grad, int64_t grad_stride,
                        float* d_colsum, void* ws, size_t ws_bytes, void* stream);
/* The same without its finishing launch: the column sums stay *out_G rows of N partial sums at the head of `ws` (which remains the
 * caller's until they are consumed) -- a source of kind TZR_ADAM_SRC_ROWS (G = *out_G, P = N, col = 0) for tzr_dense_adam_fused:
 * the bias gradient of a Linear + ReLU layer goes into the optimizer's launch without ever being a tensor. */
int tzr_relu_bwd_colsum_parts(const float* d_grad_y, int64_t grad_y_stride, const float* d_y, int64_t y_stride, int64_t B, int N,
                              float* d_grad, int64_t grad_stride, void* ws, size_t ws_bytes, int* out_G, void* stream);

/* Backward of the one-unit logits layer y = x w^T + b (tzrec/models/rank_model.py output layer
 * with num_class 1): d_grad_x[b,:] = gy[b] * w (nullable), d_grad_wb[0:N] = sum_b gy[b] * x[b,:],
 * d_grad_wb[N] = sum_b gy[b] (d_grad_wb holds N + 4 floats).  One pass over x. */
size_t tzr_head_bwd_workspace(int64_t B, int N);
int tzr_head_bwd(const float* d_grad_y, int64_t grad_y_stride, const float* d_x, int64_t x_stride,
                 const float* d_w, int64_t B, int N, float* d_grad_x, int64_t grad_x_stride,
                 float* d_grad_wb, void* ws, size_t ws_bytes, void* stream);

/* tzr_head_bwd when x is the output of a ReLU (the last hidden layer of the attention MLP in front of DIN's one-unit score
 * layer, tzrec/modules/sequence.py:101-128): d_grad[b,:] = gy[b] * w * (x[b,:] > 0) -- the gradient at the hidden layer's
 * pre-activation --, d_sums = [sum_b gy[b] x[b,:] (N) | sum_b gy[b], 0, 0, 0 | sum_b d_grad[b,:] (N)]: the score layer's weight
 * and bias gradient and the hidden layer's bias gradient from one pass over x.  Replaces tzr_head_bwd + tzr_relu_bwd_colsum. */
size_t tzr_head_bwd_relu_workspace(int64_t B, int N);
int tzr_head_bwd_relu(const float* d_grad_y, int64_t grad_y_stride, const float* d_x, int64_t x_stride,
                      const float* d_w, int64_t B, int N, float* d_grad, int64_t grad_stride,
                      float* d_sums, void* ws, size_t ws_bytes, void* stream);

/* The mixing step of a multi-gate mixture of experts (tzrec/modules/mmoe.py:63-76) for ALL tasks in one launch:
 *   out_t[b,:] = sum_e softmax(logits_t[b,:])_e * expert_e[b,:]
 * forward: reads logits / expert, writes out and probs (the softmax, [B, n_experts] contiguous per task, kept for the backward);
 * backward: reads grad_out / expert / probs, writes d_expert_e[b,:] = sum_t probs_t[b,e] * grad_out_t[b,:] (the sum over the
 * tasks included) and d_logits_t (softmax backward of <grad_out_t[b,:], expert_e[b,:]>).  Nothing is stacked: every expert is its
 * own [B, H] buffer.  H multiple of 4; float pointers 16-byte aligned, row strides multiples of 4 (logits / d_logits: any). */
#define TZR_MOE_MAX_EXPERTS 8
#define TZR_MOE_MAX_TASKS 4
typedef struct TzrMoeMix {
  int64_t B;
  int32_t H, n_experts, n_tasks, reserved;
  uint64_t expert[TZR_MOE_MAX_EXPERTS];          /* const float* [B, H]                       */
  int64_t expert_stride[TZR_MOE_MAX_EXPERTS];
  uint64_t d_expert[TZR_MOE_MAX_EXPERTS];        /* float* [B, H]            (backward)       */
  int64_t d_expert_stride[TZR_MOE_MAX_EXPERTS];
  uint64_t logits[TZR_MOE_MAX_TASKS];            /* const float* [B, n_experts]   (forward)   */
  int64_t logits_stride[TZR_MOE_MAX_TASKS];
  uint64_t probs[TZR_MOE_MAX_TASKS];             /* float* [B, n_experts] contiguous          */
  uint64_t out[TZR_MOE_MAX_TASKS];               /* float* [B, H]                 (forward)   */
  int64_t out_stride[TZR_MOE_MAX_TASKS];
  uint64_t grad_out[TZR_MOE_MAX_TASKS];          /* const float* [B, H]           (backward)  */
  int64_t grad_out_stride[TZR_MOE_MAX_TASKS];
  uint64_t d_logits[TZR_MOE_MAX_TASKS];          /* float* [B, n_experts]         (backward)  */
  int64_t d_logits_stride[TZR_MOE_MAX_TASKS];
} TzrMoeMix;
int tzr_moe_mix_fwd(const TzrMoeMix* h_mix, void* stream);
int tzr_moe_mix_bwd(const TzrMoeMix* h_mix, void* stream);

/* The gate-and-mix step of one CGC level of PLE (tzrec/modules/extraction_net.py:98-139), EVERY gate in one launch; unlike
 * tzr_moe_mix_* each gate g mixes its own subset of the experts, sel[g][0 .. n_sel[g]) in the order of its logit columns (one
 * kernel body serves both, csrc/gate_mix.hip: with sel[g] = 0 .. n_experts-1 for every gate the results equal tzr_moe_mix_*'s
 * bit for bit; the limits and the status codes of the two ABIs are their own):
 *   probs_g[b,:] = softmax(logits_g[b, 0:n_sel[g]]),   out_g[b,:] = sum_j probs_g[b,j] * expert[sel[g][j]][b,:]
 * forward: reads logits / expert, writes out and probs ([B, n_sel[g]] contiguous per gate, kept for the backward);
 * backward: reads grad_out / expert / probs, writes d_expert_e[b,:] = sum over the gates g that hold e, in ascending g, of
 * probs_g[b, j(e)] * grad_out_g[b,:] (stored once; zeros for an expert of no gate) and d_logits_g[b,j] = probs_g[b,j] *
 * (<grad_out_g[b,:], expert[sel[g][j]][b,:]> - sum_k probs_g[b,k] <grad_out_g[b,:], expert[sel[g][k]][b,:]>).  Deterministic.
 * fp32; H multiple of 4, <= 4096.  TZR_ERR_INVALID: a null or misaligned pointer ([B, H] operands 16 bytes, the others 4), a
 * negative B, a non-positive H / n_experts / n_gates / n_sel, a sel entry outside [0, n_experts) or twice in one gate.
 * TZR_ERR_UNSUPPORTED: over a limit (H, n_experts, n_gates, n_sel), a [B, H] row stride that is no multiple of 4 or below H, a
 * logits / d_logits stride below n_sel.  B == 0: TZR_OK, nothing is read or written.  A refused call launches nothing. */
#define TZR_CGC_MAX_EXPERTS 16
#define TZR_CGC_MAX_GATES 5
typedef struct TzrCgcMix {
  int64_t B;
  int32_t H, n_experts, n_gates, reserved;
  uint64_t expert[TZR_CGC_MAX_EXPERTS];          /* const float* [B, H]                       */
  int64_t expert_stride[TZR_CGC_MAX_EXPERTS];
  uint64_t d_expert[TZR_CGC_MAX_EXPERTS];        /* float* [B, H]            (backward)       */
  int64_t d_expert_stride[TZR_CGC_MAX_EXPERTS];
  int32_t n_sel[TZR_CGC_MAX_GATES];              /* members of gate g                         */
  int32_t reserved2[3];
  int32_t sel[TZR_CGC_MAX_GATES][TZR_CGC_MAX_EXPERTS]; /* expert index of logit column j of gate g */
  uint64_t logits[TZR_CGC_MAX_GATES];            /* const float* [B, n_sel[g]]    (forward)   */
  int64_t logits_stride[TZR_CGC_MAX_GATES];
  uint64_t probs[TZR_CGC_MAX_GATES];             /* float* [B, n_sel[g]] contiguous           */
  uint64_t out[TZR_CGC_MAX_GATES];               /* float* [B, H]                 (forward)   */
  int64_t out_stride[TZR_CGC_MAX_GATES];
  uint64_t grad_out[TZR_CGC_MAX_GATES];          /* const float* [B, H]           (backward)  */
  int64_t grad_out_stride[TZR_CGC_MAX_GATES];
  uint64_t d_logits[TZR_CGC_MAX_GATES];          /* float* [B, n_sel[g]]          (backward)  */
  int64_t d_logits_stride[TZR_CGC_MAX_GATES];
} TzrCgcMix;
int tzr_cgc_mix_fwd(const TzrCgcMix* h_mix, void* stream);
int tzr_cgc_mix_bwd(const TzrCgcMix* h_mix, void* stream);

/* The gate-and-scale step of PEPNet (tzrec/modules/personalized_net.py), EVERY slot (a task of one PPNet level, or the one gate
 * of EPNet) in one launch:
 *   out_n[b,:] = act(z_n[b,:] + bz_n) * gamma * sigmoid(g_n[b,:] + bg_n),   act = ReLU (relu != 0) or identity
 * z_n / g_n are the GEMM outputs WITHOUT bias; bz_n may be null (no bias), bg_n not.
 * forward: reads z / bz / g / bg, writes out.
 * backward: reads grad_out / z / bz / g / bg -- nothing else is kept from the forward: the sigmoid and, with the forward's own
 * fp32 add, the ReLU mask are recomputed -- and writes dz_n = grad_out * gamma * s * [z + bz > 0] (identity: no mask),
 * dg_n = grad_out * act(z + bz) * gamma * s * (1 - s), and d_bias = [n_slots][2][H] floats: per slot the column sums of dz_n,
 * then of dg_n, over the batch (per-workgroup partial rows in `ws`, added by a second launch in the interleaved order of
 * csrc/parts_sum.h).  grad_out[n] == 0: slot n has no output gradient, its dz / dg / d_bias are zeros.  dz[n] may be z[n] and
 * dg[n] may be g[n] (in place).  The sigmoid is formed from exp(-|x|) without overflow or cancellation: finite for every finite x, and
 * exactly 0 or 1 past |x| = 87.3 (exp(-|x|) below the smallest normal fp32 counts as 0), where dg is exactly 0.  Deterministic, no atomics.  fp32; H multiple of 4, <= 4096; at most TZR_GATE_SCALE_MAX_SLOTS slots.
 * TZR_ERR_INVALID: a null or misaligned (16 bytes) pointer, B <= 0, a non-positive H / n_slots.  TZR_ERR_UNSUPPORTED: over a
 * limit (H, n_slots), a row stride that is no multiple of 4 or below H.  TZR_ERR_WORKSPACE: `ws` null, not 256-byte aligned or
 * below tzr_gate_scale_bwd_workspace (which includes 256 bytes of alignment slack).  A refused call launches nothing. */
#define TZR_GATE_SCALE_MAX_SLOTS 8
typedef struct TzrGateScale {
  int64_t B;
  int32_t H, n_slots, relu, reserved;
  float gamma;
  int32_t reserved2;
  uint64_t z[TZR_GATE_SCALE_MAX_SLOTS];              /* const float* [B, H]                       */
  int64_t z_stride[TZR_GATE_SCALE_MAX_SLOTS];
  uint64_t bz[TZR_GATE_SCALE_MAX_SLOTS];             /* const float* [H], nullable                */
  uint64_t g[TZR_GATE_SCALE_MAX_SLOTS];              /* const float* [B, H]                       */
  int64_t g_stride[TZR_GATE_SCALE_MAX_SLOTS];
  uint64_t bg[TZR_GATE_SCALE_MAX_SLOTS];             /* const float* [H]                          */
  uint64_t out[TZR_GATE_SCALE_MAX_SLOTS];            /* float* [B, H]                 (forward)   */
  int64_t out_stride[TZR_GATE_SCALE_MAX_SLOTS];
  uint64_t grad_out[TZR_GATE_SCALE_MAX_SLOTS];       /* const float* [B, H], nullable (backward)  */
  int64_t grad_out_stride[TZR_GATE_SCALE_MAX_SLOTS];
  uint64_t dz[TZR_GATE_SCALE_MAX_SLOTS];             /* float* [B, H]                 (backward)  */
  int64_t dz_stride[TZR_GATE_SCALE_MAX_SLOTS];
  uint64_t dg[TZR_GATE_SCALE_MAX_SLOTS];             /* float* [B, H]                 (backward)  */
  int64_t dg_stride[TZR_GATE_SCALE_MAX_SLOTS];
  uint64_t d_bias;                                   /* float* [n_slots][2][H]        (backward)  */
  uint64_t ws;                                       /* workspace                     (backward)  */
  uint64_t ws_bytes;
} TzrGateScale;
int tzr_gate_scale_fwd(const TzrGateScale* h_gs, void* stream);
size_t tzr_gate_scale_bwd_workspace(int64_t B, int H, int n_slots);
int tzr_gate_scale_bwd(const TzrGateScale* h_gs, void* stream);

/* The Bayesian relation towers of DBMTL (tzrec/models/dbmtl.py:90-112, 155-167), the WHOLE chain of a model in one launch
 * forward and two backward.  Tower t of n_towers (config order) has an input x_t [B, x_width[t]], n_deps[t] EARLIER towers
 * deps[t][..] (each at most once) and n_layers[t] in 0..4 layers (w [N, K], b [N], nn.Linear layout, N = width[t][l]):
 *   n_layers[t] == 0:  r_t = x_t; nothing is computed or copied, consumers read x_t (its deps are ignored);
 *   n_layers[t] >= 1:  r_t = relu(W_{L-1} .. relu(W_0 u_t + b_0) .. + b_{L-1}),  u_t = [x_t | r_d for d in deps[t]] -- a virtual
 *                      concatenation, never written: K of layer 0 is x_width[t] plus the widths of the r_d.
 * forward: reads x / w / b, writes every layer's post-ReLU output h[t][l] [B, N] contiguous; the last one is r_t.
 * backward: reads grad_r[t] = dL/dr_t ([B, width of r_t]; 0: none; ignored for a tower without layers), x, w, h; writes
 *   dx[t] [B, x_width[t]] -- a tower with layers: the x_t slice of dz_{t,0} W_{t,0}; a tower without: the sum of the slices its
 *   consumers send, in descending consumer index (zeros without a consumer) --, dw[t][l] [N, K], db[t][l] [N].  The gradient of
 *   r_t is grad_r[t] plus its consumers' slices in descending consumer index.  The pre-activation gradients live in `ws`.
 * Two towers may name the same x; each has its own dx.  fp32; every width a multiple of 4; layer widths <=
 * TZR_RELATION_CHAIN_MAX_WIDTH, x widths <= TZR_RELATION_CHAIN_MAX_X.  Deterministic, no atomics, two runs are bit-equal.
 * TZR_ERR_INVALID: a null or misaligned (16 bytes) pointer, B <= 0, a non-positive n_towers / width, a negative n_layers /
 * n_deps, a dep that is not an earlier tower or stands twice.  TZR_ERR_UNSUPPORTED: over a limit, a width that is no multiple of
 * 4, a row stride that is no multiple of 4 or below the width.  TZR_ERR_WORKSPACE: `ws` null, not 256-byte aligned or below
 * tzr_relation_chain_bwd_workspace (which includes 256 bytes of alignment slack).  A refused call launches nothing. */
#define TZR_RELATION_CHAIN_MAX_TOWERS 8
#define TZR_RELATION_CHAIN_MAX_LAYERS 4
#define TZR_RELATION_CHAIN_MAX_WIDTH 128
#define TZR_RELATION_CHAIN_MAX_X 1024
typedef struct TzrRelationChain {
  int64_t B;
  int32_t n_towers, reserved;
  int32_t x_width[TZR_RELATION_CHAIN_MAX_TOWERS];
  int32_t n_layers[TZR_RELATION_CHAIN_MAX_TOWERS];
  int32_t n_deps[TZR_RELATION_CHAIN_MAX_TOWERS];
  int32_t deps[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_TOWERS];
  int32_t width[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_LAYERS];
  uint64_t x[TZR_RELATION_CHAIN_MAX_TOWERS];                                    /* const float* [B, x_width]          */
  int64_t x_stride[TZR_RELATION_CHAIN_MAX_TOWERS];
  uint64_t w[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_LAYERS];     /* const float* [N, K] contiguous     */
  uint64_t b[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_LAYERS];     /* const float* [N]                   */
  uint64_t h[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_LAYERS];     /* float* [B, N] contiguous           */
  uint64_t grad_r[TZR_RELATION_CHAIN_MAX_TOWERS];                               /* const float*, nullable (backward)  */
  int64_t grad_r_stride[TZR_RELATION_CHAIN_MAX_TOWERS];
  uint64_t dx[TZR_RELATION_CHAIN_MAX_TOWERS];                                   /* float* [B, x_width]    (backward)  */
  int64_t dx_stride[TZR_RELATION_CHAIN_MAX_TOWERS];
  uint64_t dw[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_LAYERS];    /* float* [N, K]          (backward)  */
  uint64_t db[TZR_RELATION_CHAIN_MAX_TOWERS][TZR_RELATION_CHAIN_MAX_LAYERS];    /* float* [N]             (backward)  */
  uint64_t ws;                                                                  /* workspace              (backward)  */
  uint64_t ws_bytes;
} TzrRelationChain;
int tzr_relation_chain_fwd(const TzrRelationChain* h_rc, void* stream);
size_t tzr_relation_chain_bwd_workspace(const TzrRelationChain* h_rc);
int tzr_relation_chain_bwd(const TzrRelationChain* h_rc, void* stream);

/* The similarity head of the match models (tzrec/models/match_model.py:50-64, 303-336, dssm.py:81-83, 147-155): normalize,
 * similarity, temperature, softmax cross entropy and the rank of the positive, without the [B, C] score matrix in memory.
 * u [B, D] and v [M, D] are the towers' outputs, fp32, any row stride that is a multiple of 4 floats.
 *   cosine == 1:  u^_i = u_i / max(|u_i|, 1e-12), v^ likewise (F.normalize); cosine == 0: u^ = u, v^ = v
 *   TZR_MATCH_SAMPLED,  M = B + N, N >= 0:  row i has C = 1 + N scores, s_i0 = <u^_i, v^_i> / T, s_ij = <u^_i, v^_{B+j-1}> / T;
 *                                           the label column is 0
 *   TZR_MATCH_IN_BATCH, M = B:              s_ij = <u^_i, v^_j> / T, C = B; the label column is i
 *   l_i = logsumexp_j s_ij - s_i,label;  loss = sum(w l) / sum(w), 0 when sum(w) == 0 (w [B], nullable: mean(l));
 *   rank_i = the number of columns j != label with s_ij > s_i,label.
 * forward (one launch and a finishing one): writes loss [1], lse [B] = rmax + lsum, rmax [B] (the row's largest score) and lsum
 *   [B] (log of the sum of exp(s - rmax); kept apart for the backward: their sum rounds at the size of the scores, 1 / T), pos
 *   [B] (s_i,label), rank [B] int32, scale [1] (the reciprocal of the loss's denominator), with cosine ru [B] and rv [M] (the
 *   inverse norms, DOUBLE: see csrc/match_softmax.hip), and, when `sim` is not 0, the scores sim [B, C] with row stride
 *   sim_stride >= C.  `ws`: tzr_match_softmax_workspace bytes.
 * backward (two launches; one when SAMPLED has N == 0): reads grad_loss [1] FROM DEVICE MEMORY, u, v, w, rmax, lsum, pos,
 *   scale, ru, rv; writes du [B, D] and dv [M, D], through the normalisation when cosine is set.  w is a constant.
 * Deterministic, no atomics, two runs are bit-equal.  TZR_ERR_UNSUPPORTED: D % 4 != 0, D < 4, D > TZR_MATCH_SOFTMAX_MAX_D, B < 1,
 * M < B, M != B in IN_BATCH mode, an unknown mode, a `cosine` other than 0 or 1, a row stride that is no multiple of 4 or below
 * the width, a sim_stride below C.  TZR_ERR_INVALID: a null or misaligned pointer (u / v / du / dv 16 bytes, ru / rv 8, the
 * others 4; w and sim may be 0, ru and rv without cosine).  TZR_ERR_WORKSPACE: `ws` null, not 256-byte aligned or below the query
 * less its 256 bytes of slack.  A refused call launches nothing. */
#define TZR_MATCH_SOFTMAX_MAX_D 256
#define TZR_MATCH_SAMPLED 0
#define TZR_MATCH_IN_BATCH 1
typedef struct TzrMatchSoftmax {
  int64_t B, M;
  int32_t D, mode, cosine, reserved;
  float inv_temperature;
  int32_t reserved2;
  uint64_t u;          /* const float* [B, D] */
  int64_t u_stride;
  uint64_t v;          /* const float* [M, D] */
  int64_t v_stride;
  uint64_t w;          /* const float* [B], nullable */
  uint64_t loss;       /* float* [1]            (forward writes) */
  uint64_t lse;        /* float* [B]            (forward writes) */
  uint64_t rmax;       /* float* [B]            (forward writes, backward reads) */
  uint64_t lsum;       /* float* [B]            (forward writes, backward reads) */
  uint64_t pos;        /* float* [B]            (forward writes, backward reads) */
  uint64_t rank;       /* int32_t* [B]          (forward writes) */
  uint64_t scale;      /* float* [1]            (forward writes, backward reads) */
  uint64_t ru;         /* double* [B], cosine   (forward writes, backward reads) */
  uint64_t rv;         /* double* [M], cosine   (forward writes, backward reads) */
  uint64_t sim;        /* float* [B, C], nullable (forward writes) */
  int64_t sim_stride;
  uint64_t grad_loss;  /* const float* [1]      (backward) */
  uint64_t du;         /* float* [B, D]         (backward) */
  int64_t du_stride;
  uint64_t dv;         /* float* [M, D]         (backward) */
  int64_t dv_stride;
  uint64_t ws;         /* workspace             (forward) */
  uint64_t ws_bytes;
} TzrMatchSoftmax;
size_t tzr_match_softmax_workspace(const TzrMatchSoftmax* h_ms);
int tzr_match_softmax_fwd(const TzrMatchSoftmax* h_ms, void* stream);
int tzr_match_softmax_bwd(const TzrMatchSoftmax* h_ms, void* stream);

/* The behaviour-to-interest capsule layer of MIND (tzrec/modules/capsule.py:125-231), restated on the jagged rows: pad /
 * truncate to max_seq_len, low capsules U = X W, num_iters rounds of dynamic routing, squash, capsule mask -- one launch
 * forward, two backward, nothing of shape [B, S, H] in memory.
 *   x [N, L] fp32 jagged rows (unit column stride, row stride a multiple of 4 floats, 16-byte aligned rows), offsets [B + 1]
 *   int64 (non-decreasing, offsets[B] <= N), w [L, H] contiguous (`bilinear_matrix`), logits0 [N, K] or 0 for zeros.
 *   Sample b: len_b = offsets[b + 1] - offsets[b], its first s_b = min(len_b, S) rows take part;
 *   k_b = K with const_caps_num, else max(1, #{ j < K : 2^j < len_b }) (= arange(K) < clamp(log2(len_b), 1, K), from the
 *   UNTRUNCATED length); a sample without rows has high = 0 and one valid capsule.
 *   logits = logits0 * stddev; every iteration: c = softmax over the k_b valid capsules of logits * scale (a masked capsule's
 *   weight is exactly 0); except in the last, logits = c + <high_k, u_n / max(|u_n|, 1e-12)> with high = c^T U (the reference
 *   adds the agreement to the softmax WEIGHTS); the last one: pre = c^T U, high_k = pre_k (r^squash_pow / e) with
 *   e = max(|pre_k|, 1e-7), r = e^2 / (1 + e^2).
 * forward writes high [B K, H] (row b K + k, row stride high_stride; rows k >= k_b are zeros), mask [B, K] (bytes 0 / 1), c
 *   [N, K] (the final routing weights; rows behind S are zeros) and pre [B, K, H] (contiguous; for the backward).
 * backward: the routing weights are constants for autograd (capsule.py:146, 154-157), so with Z = c^T X per sample and dpre
 *   the gradient in front of the squash (through max(., 1e-7) as torch.max passes it): dx_n = sum_k c[n, k] (dpre W^T)[k, :]
 *   (rows behind S: zeros), dw = sum_b Z_b^T dpre_b.  A per-sample launch of min(B, TZR_CAPSULE_BWD_MAX_GRID) workgroups (workgroup
 *   g takes the samples g, g + grid, ... in that order) leaves dw as one partial [L x H] row per workgroup in `ws`
 *   (tzr_capsule_workspace bytes); a finishing launch adds the rows in the interleaved order (csrc/parts_sum.h).  logits0 gets
 *   no gradient.  No atomics; every sum's order is a function of the shapes and the offsets alone: two runs are bit-equal.
 * Limits (TZR_ERR_UNSUPPORTED beyond): L, H multiples of 4 in [4, TZR_CAPSULE_MAX_DIM]; 1 <= K <= TZR_CAPSULE_MAX_K; 1 <=
 *   num_iters <= TZR_CAPSULE_MAX_ITERS; 1 <= S <= TZR_CAPSULE_MAX_S and ceil16(S) * H <= TZR_CAPSULE_MAX_SH (the low capsules of one
 *   sample in LDS: S <= 128 at H <= 64, S <= 64 at H <= 128); scale > 0; B, N < 2^31; a row stride that is no multiple of 4 or below the
 *   width.  TZR_ERR_INVALID: a null or misaligned pointer (x / high / grad_high / dx 16 bytes, offsets 8, w 16, the others 4; x and dx
 *   may be 0 when N == 0, logits0 may be 0), B < 0, N < 0.  TZR_ERR_WORKSPACE: `ws` null, not 256-byte aligned or below the
 *   query less its 256 bytes of slack.  B == 0: TZR_OK without a launch.  A refused call launches nothing.
 * A new struct and entry points, no change to existing ones: the ABI version stays 15. */
#define TZR_CAPSULE_MAX_DIM 128
#define TZR_CAPSULE_MAX_K 8
#define TZR_CAPSULE_MAX_ITERS 8
#define TZR_CAPSULE_MAX_S 128
#define TZR_CAPSULE_MAX_SH 8192
#define TZR_CAPSULE_BWD_MAX_GRID 512
typedef struct TzrCapsule {
  int64_t B, N;
  int32_t L, H, K, S, num_iters, const_caps_num;
  float scale, stddev, squash_pow; /* routing_logits_scale, routing_logits_stddev, squash_pow */
  int32_t reserved;
  uint64_t x;           /* const float* [N, L] */
  int64_t x_stride;
  uint64_t offsets;     /* const int64_t* [B + 1] */
  uint64_t w;           /* const float* [L, H] */
  uint64_t logits0;     /* const float* [N, K], nullable */
  uint64_t high;        /* float* [B K, H]        (forward writes) */
  int64_t high_stride;
  uint64_t mask;        /* uint8_t* [B, K]        (forward writes) */
  uint64_t c;           /* float* [N, K]          (forward writes, backward reads) */
  uint64_t pre;         /* float* [B, K, H]       (forward writes, backward reads) */
  uint64_t grad_high;   /* const float* [B K, H]  (backward) */
  int64_t grad_high_stride;
  uint64_t dx;          /* float* [N, L]          (backward) */
  int64_t dx_stride;
  uint64_t dw;          /* float* [L, H]          (backward) */
  uint64_t ws;          /* workspace              (backward) */
  uint64_t ws_bytes;
} TzrCapsule;
size_t tzr_capsule_workspace(const TzrCapsule* h_cap);
int tzr_capsule_fwd(const TzrCapsule* h_cap, void* stream);
int tzr_capsule_bwd(const TzrCapsule* h_cap, void* stream);

/* MIND's label-aware attention (tzrec/models/mind.py:303-333): the positive item of a sample attends over its interests.
 * i [B K, D] (row b K + k = interest k of sample b), v [B, D] (the first B rows of the item embeddings), fp32, row strides that are
 * multiples of 4 floats, 16-byte aligned rows; mask [B, K] bytes (the capsule mask).
 *   forward:   a_k = <i_bk, v_b>; w = softmax over the valid capsules of simi_pow a_k (a masked capsule's weight is exactly 0);
 *              out[b] = sum_k w_k i_bk; d_w [B, K] is kept for the backward.
 *   backward:  t_k = <g_b, i_bk>; da_k = simi_pow w_k (t_k - sum_j w_j t_j); d_di[b K + k] = w_k g_b + da_k v_b (zero rows for masked
 *              capsules); d_dv[b] = sum_k da_k i_bk.
 * One launch each way, one wave per sample, fixed summation order, no atomics: bit-reproducible.  TZR_ERR_UNSUPPORTED: D % 4
 * != 0, D < 4, D > TZR_LABEL_ATTN_MAX_D, K < 1, K > TZR_LABEL_ATTN_MAX_K, simi_pow <= 0, B >= 2^31, a row stride that is no
 * multiple of 4 or below D.  TZR_ERR_INVALID: a null or misaligned pointer (rows 16 bytes, d_w 4), B < 0.  B == 0 is TZR_OK
 * without a launch.  Entry points only, no struct changes: the ABI version stays 15. */
#define TZR_LABEL_ATTN_MAX_D 256
#define TZR_LABEL_ATTN_MAX_K 8
int tzr_label_attn_fwd(const float* d_i, int64_t i_stride, const float* d_v, int64_t v_stride, const uint8_t* d_mask, int64_t B, int K, int D,
                       float simi_pow, float* d_out, int64_t out_stride, float* d_w, void* stream);
int tzr_label_attn_bwd(const float* d_grad_out, int64_t grad_out_stride, const float* d_i, int64_t i_stride, const float* d_v, int64_t v_stride,
                       const float* d_w, const uint8_t* d_mask, int64_t B, int K, int D, float simi_pow, float* d_di, int64_t di_stride,
                       float* d_dv, int64_t dv_stride, void* stream);

/* DAT's Adaptive-Mimic loss (tzrec/models/dat.py:212-259), the user side and the item side in one launch.  ua [B, D] / ia [M, D]:
 * the towers' augment rows; ue [B, D] / ie [M, D]: the towers' embeddings BEFORE any normalisation, constants here (no gradient);
 * M >= B, only the first B rows of ia / ie take part.  fp32, unit column stride, row strides that are multiples of 4 floats and no
 * narrower than D, 16-byte aligned rows (column slices of wider buffers are fine); w [B] fp32 sample weights or 0.
 *   Side u: a = ua[b], t = ie[b], c = c_u; side i: a = ia[b], t = ue[b], c = c_i.
 *   n = max(|a|, 1e-12), y = a / n; tau = t / max(|t|, 1e-12) when `cosine`, else t; l_b = sum_d (y_d - tau_d)^2;
 *   loss_s = c sum_b l_b (a sum, not a mean), with w: c sum_b(l_b w_b) / sum_b(w_b), exactly 0 when the weights add to 0.
 * forward writes loss [2] (loss_u, loss_i), rows [6, B] contiguous (l_u, l_i, 1/n of side u, of side i -- NEGATED where |a| < 1e-12,
 *   the backward's clamp branch --, 1/max(|t|, 1e-12) of side u, of side i: 1 without `cosine`) and scale [1] (1 / sum(w), 0 when that sum
 *   is 0, 1 without w).  One wave per sample, four samples per workgroup, one partial row (sum l_u w, sum l_i w, sum w) per
 *   workgroup in `ws` (tzr_amm_loss_workspace bytes); a finishing launch adds the rows in the interleaved order (csrc/parts_sum.h).
 * backward reads the upstream gradients g_u, g_i from device memory (grad_u / grad_i, one float each; 0 = no gradient for that
 *   side) and `rows`, `scale` as the forward left them: k_b = g c (with w: g c w_b scale); dy = 2 k_b (y - tau);
 *   da = (dy - y <y, dy>) / n where |a| >= 1e-12, dy / 1e-12 below (torch's clamp_min branch); writes dua [B, D] and dia [M, D], rows
 *   b >= B of dia as exact zeros.  One launch.  Nothing flows to ue / ie.
 * No atomics, every sum's order a function of B alone: two runs are bit-equal.  TZR_ERR_UNSUPPORTED: D % 4 != 0, D < 4, D >
 * TZR_AMM_MAX_D, M < B, B or M >= 2^31, `cosine` not 0 / 1, a row stride that is no multiple of 4 or below D.  TZR_ERR_INVALID: a
 * null or misaligned pointer (rows 16 bytes, the others 4; w, grad_u, grad_i may be 0), B < 0.  TZR_ERR_WORKSPACE (forward): `ws`
 * null, not 256-byte aligned or below the query less its 256 bytes of slack.  B == 0 is TZR_OK without a launch.  A refused call
 * launches nothing.  A new struct and entry points, no change to existing ones: the ABI version stays 15. */
#define TZR_AMM_MAX_D 256
typedef struct TzrAmmLoss {
  int64_t B, M;
  int32_t D, cosine;
  float c_u, c_i;      /* amm_u_weight, amm_i_weight */
  uint64_t ua;         /* const float* [B, D] */
  int64_t ua_stride;
  uint64_t ia;         /* const float* [M, D] */
  int64_t ia_stride;
  uint64_t ue;         /* const float* [B, D] */
  int64_t ue_stride;
  uint64_t ie;         /* const float* [M, D] */
  int64_t ie_stride;
  uint64_t w;          /* const float* [B], nullable */
  uint64_t loss;       /* float* [2]            (forward writes) */
  uint64_t rows;       /* float* [6, B]         (forward writes, backward reads) */
  uint64_t scale;      /* float* [1]            (forward writes, backward reads) */
  uint64_t grad_u;     /* const float* [1], nullable (backward) */
  uint64_t grad_i;     /* const float* [1], nullable (backward) */
  uint64_t dua;        /* float* [B, D]         (backward) */
  int64_t dua_stride;
  uint64_t dia;        /* float* [M, D]         (backward) */
  int64_t dia_stride;
  uint64_t ws;         /* workspace             (forward) */
  uint64_t ws_bytes;
} TzrAmmLoss;
size_t tzr_amm_loss_workspace(const TzrAmmLoss* h_amm);
int tzr_amm_loss_fwd(const TzrAmmLoss* h_amm, void* stream);
int tzr_amm_loss_bwd(const TzrAmmLoss* h_amm, void* stream);

/* Rocket Launching's distillation terms (tzrec/models/rocket_launching.py:125-204): the similarity term of every pair of equally
 * wide hidden layers and the hint loss on the logits, in one launch.  P <= TZR_DISTILL_MAX_PAIRS pairs; pair p is light[p] and
 * booster[p], both [B, W[p]] fp32 with unit column stride, their own row strides (multiples of 4 floats, no narrower than W[p]) and
 * 16-byte aligned rows (column slices of wider buffers are fine); W[p] % 4 == 0, 4 <= W[p] <= TZR_DISTILL_MAX_W, the widths of one
 * call may differ.  logits_light / logits_booster [B, C] contiguous fp32, 1 <= C <= 64; w [B] fp32 sample weights or 0.  Every
 * booster operand is a constant: no gradient.
 *   lw_b = w_b / mean(w), 0 when mean(w) is 0 (div_no_nan); 1 without w.
 *   cosine:   sim_p = -0.1 mean_b(lw_b <l / max(|l|, 1e-12), t / max(|t|, 1e-12)>), l = light[p][b], t = booster[p][b];
 *   distance: sim_p = sqrt(sum_b lw_b |t - l|^2) (the root of a sum, not a mean);
 *   hint = sum_b lw_b sum_c (logits_light[b, c] - logits_booster[b, c])^2 / (B C).
 * forward writes loss [P + 1] (sim_0 .. sim_{P-1}, hint) and scale [1 + TZR_DISTILL_MAX_PAIRS] (scale[0] = B / sum(w), 0 when
 *   that sum is 0, 1 without w; scale[1 + p] = 1 / sim_p under distance, 0 where sim_p is 0 and under cosine).  One wave per
 *   sample walks the pairs, four samples per workgroup, one partial row of P + 2 sums per workgroup in `ws`
 *   (tzr_distill_loss_workspace bytes); a finishing launch adds the rows in the interleaved order (csrc/parts_sum.h).  Nothing is
 *   saved per sample: the backward recomputes the norms from the rows it reads anyway.
 * backward reads the upstream gradients from device memory (grad_sim[p], grad_hint: one float each; 0 = nobody asked for that
 *   term) and `scale` as the forward left it, and writes dlight[p] [B, W[p]] (0 = skip the pair; with grad_sim[p] == 0 the rows are
 *   written as zeros) and dlogits_light [B, C] contiguous (0 = skip; with grad_hint == 0 zeros).  cosine: dy = k t / max(|t|, 1e-12),
 *   k = g_p (-0.1 / B) lw_b; dl = (dy - y <y, dy>) / |l| where |l| >= 1e-12, dy / 1e-12 below (torch's clamp_min branch).
 *   distance: dl = g_p lw_b (l - t) / sim_p, and ZERO rows where sim_p is exactly 0 (the literal form gives NaN there: 0 * inf).
 *   hint: g_h lw_b 2 (ll - lb) / (B C).  One launch.
 * No atomics, every sum's order a function of the shapes alone: two runs are bit-equal.  TZR_ERR_UNSUPPORTED: P outside 0 ..
 * TZR_DISTILL_MAX_PAIRS, C outside 1 .. 64, B >= 2^31, `cosine` not 0 / 1, a W[p] that is no multiple of 4, below 4 or above
 * TZR_DISTILL_MAX_W, a row stride that is no multiple of 4 or below W[p].  TZR_ERR_INVALID: a null or misaligned pointer (rows 16
 * bytes, the others 4; w, grad_*, dlight[p], dlogits_light may be 0), B < 0.  TZR_ERR_WORKSPACE (forward): `ws` null, not 256-byte
 * aligned or below the query less its 256 bytes of slack.  Limits are checked first, then pointers.  B == 0 is TZR_OK without a
 * launch.  A refused call launches nothing.  A new struct and entry points, no change to existing ones: the ABI version stays 15. */
#define TZR_DISTILL_MAX_PAIRS 8
#define TZR_DISTILL_MAX_W 1024
typedef struct TzrDistillLoss {
  int64_t B;
  int32_t P, C, cosine, pad_;
  int32_t W[TZR_DISTILL_MAX_PAIRS];
  uint64_t light[TZR_DISTILL_MAX_PAIRS];          /* const float* [B, W[p]] */
  int64_t light_stride[TZR_DISTILL_MAX_PAIRS];
  uint64_t booster[TZR_DISTILL_MAX_PAIRS];        /* const float* [B, W[p]] */
  int64_t booster_stride[TZR_DISTILL_MAX_PAIRS];
  uint64_t logits_light;                          /* const float* [B, C] */
  uint64_t logits_booster;                        /* const float* [B, C] */
  uint64_t w;                                     /* const float* [B], nullable */
  uint64_t loss;                                  /* float* [P + 1]                          (forward writes) */
  uint64_t scale;                                 /* float* [1 + TZR_DISTILL_MAX_PAIRS]      (forward writes, backward reads) */
  uint64_t grad_sim[TZR_DISTILL_MAX_PAIRS];       /* const float* [1] each, nullable         (backward) */
  uint64_t grad_hint;                             /* const float* [1], nullable              (backward) */
  uint64_t dlight[TZR_DISTILL_MAX_PAIRS];         /* float* [B, W[p]], nullable              (backward) */
  int64_t dlight_stride[TZR_DISTILL_MAX_PAIRS];
  uint64_t dlogits_light;                         /* float* [B, C], nullable                 (backward) */
  uint64_t ws;                                    /* workspace                               (forward) */
  uint64_t ws_bytes;
} TzrDistillLoss;
size_t tzr_distill_loss_workspace(const TzrDistillLoss* h_dst);
int tzr_distill_loss_fwd(const TzrDistillLoss* h_dst, void* stream);
int tzr_distill_loss_bwd(const TzrDistillLoss* h_dst, void* stream);

/* Linear layers with a handful of output units, n_out <= 8: the logits layer of the rank models
 * (tzrec/models/rank_model.py:190-191) and the gates of MMoE (tzrec/modules/mmoe.py: Linear(in, num_expert)).
 * forward: d_y[b, j] = sum_k d_x[b, k] * d_w[j, k] + d_bias[j] (d_bias nullable); one pass over x.
 * backward: d_grad_x[b, :] = sum_j gy[b, j] * w[j, :] (nullable), d_grad_wb = [gy^T x (n_out x K row-major) | sum_b gy[b, :]
 * (n_out, padded to a multiple of 4)]; one pass over x + a fixed-order sum of the workgroups' rows.  K multiple of 4, <= 1024;
 * x / w / grad_x strides multiples of 4 floats.  Replace torch's addmm + three backward products (one output tile wide). */
int tzr_skinny_linear_fwd(const float* d_x, int64_t x_stride, const float* d_w, int64_t w_stride, const float* d_bias,
                          int64_t B, int K, int n_out, float* d_y, int64_t y_stride, void* stream);
size_t tzr_skinny_linear_bwd_workspace(int64_t B, int K, int n_out);
int tzr_skinny_linear_bwd(const float* d_grad_y, int64_t grad_y_stride, const float* d_x, int64_t x_stride,
                          const float* d_w, int64_t w_stride, int64_t B, int K, int n_out, float* d_grad_x,
                          int64_t grad_x_stride, float* d_grad_wb, void* ws, size_t ws_bytes, void* stream);
/* ... without its finishing launch: [weight gradient n_out x K | bias gradient n_out, padded to 4] stay *out_G rows of *out_P
 * partial sums at the head of `ws`: two sources of kind TZR_ADAM_SRC_ROWS (col 0 and col n_out K) for tzr_dense_adam_fused. */
int tzr_skinny_linear_bwd_parts(const float* d_grad_y, int64_t grad_y_stride, const float* d_x, int64_t x_stride,
                                const float* d_w, int64_t w_stride, int64_t B, int K, int n_out, float* d_grad_x,
                                int64_t grad_x_stride, void* ws, size_t ws_bytes, int* out_G, int* out_P, void* stream);

/* Input gradient of a Linear layer chained with the ReLU mask and bias gradient of the layer below it (autograd of
 * Linear -> ReLU -> Linear, tzrec/modules/mlp.py:58-83), one launch on the matrix cores (exact fp32):
 *   d_grad_out[n,h] = (sum_k d_grad_in[n,k] * d_w[k,h]) * (d_y[n,h] > 0),  d_colsum[h] = sum_n d_grad_out[n,h].
 * d_w = the upper layer's weight [K, H] row-major (nn.Linear's own layout: out_features x in_features), d_y = the lower
 * layer's ReLU output.  d(loss)/d(y) is never written.  Shapes: tzr_linear_bwd_relu_supported(K, H) (K in {16, 32, 64},
 * H in {64, 128, 256}); strides in floats, multiples of 4; 16-byte aligned pointers.  Deterministic. */
int tzr_linear_bwd_relu_supported(int K, int H);
size_t tzr_linear_bwd_relu_workspace(int64_t N, int H);
int tzr_linear_bwd_relu(const float* d_grad_in, int64_t grad_in_stride, const float* d_w, int64_t w_stride,
                        const float* d_y, int64_t y_stride, int64_t N, int K, int H, float* d_grad_out,
                        int64_t grad_out_stride, float* d_colsum, void* ws, size_t ws_bytes, void* stream);

/* Linear layers over a TALL input (every position of a sequence batch: the attention MLP of DIN on the jagged positions,
 * tzrec/modules/sequence.py:101-128 over tzrec/modules/mlp.py:58-83) with the small weight matrix resident in registers, exact
 * fp32 on the matrix cores (csrc/gemm_rows.hip).
 *   tzr_linear_rows:  d_out[n, h] = act(sum_k d_in[n, k] * W(k, h) + d_bias[h] + d_rowvec[d_row_index[n], h])
 *     w_out_major != 0: W(k, h) = d_w[h * w_stride + k]  (nn.Linear's weight [H, K]: the layer's forward, torch's addmm + ReLU);
 *     w_out_major == 0: W(k, h) = d_w[k * w_stride + h]  (the input gradient g @ weight of a layer whose weight is [K, H]).
 *     d_bias / d_rowvec may be NULL; d_rowvec [R, H] is a per-row addend gathered through d_row_index (int32 [N]) -- the part of a
 *     layer over positions that depends on the SAMPLE only (DIN's query terms).  relu != 0: max(., 0).
 *   tzr_linear_rows_wgrad:  d_dw[h, k] (+)= sum_n d_g[n, h] * d_x[n, k]  (autograd's weight gradient g^T x), partial sums of
 *     <= 512 workgroups added in workgroup order by a second launch (deterministic; workspace from _wgrad_workspace).
 * Shapes: *_supported (K, H multiples of 16 out of a fixed list up to 256; tzr_linear_rows_supported returns 3 where d_rowvec is
 * taken too, 1 where only the plain form is built); strides in floats, multiples of 4; 16-byte aligned
 * pointers.  TZR_ERR_UNSUPPORTED otherwise: the caller keeps its GEMM library call. */
int tzr_linear_rows_supported(int K, int H);
int tzr_linear_rows(const float* d_in, int64_t in_stride, const float* d_w, int64_t w_stride, int w_out_major,
                    const float* d_bias, const float* d_rowvec, int64_t rowvec_stride, const int32_t* d_row_index, int relu,
                    int64_t N, int K, int H, float* d_out, int64_t out_stride, void* stream);
int tzr_linear_rows_wgrad_supported(int H, int K);
size_t tzr_linear_rows_wgrad_workspace(int64_t N, int H, int K);
int tzr_linear_rows_wgrad(const float* d_g, int64_t g_stride, const float* d_x, int64_t x_stride, int64_t N, int H, int K,
                          float* d_dw, int64_t dw_stride, int accumulate, void* ws, size_t ws_bytes, void* stream);

#define TZR_ADAM_MAX_TENSORS 32
typedef struct TzrAdamTensor { /* one dense parameter tensor, device addresses, float32 */
  uint64_t param, grad, exp_avg, exp_avg_sq;
  uint64_t state; /* float[3], zero-initialised by the caller: [0] step count of THIS tensor
                     (torch counts steps per parameter), [1], [2] bias corrections */
  int64_t numel;
} TzrAdamTensor; /* 48 bytes */

/* Adam step over every dense parameter tensor (torch.optim.Adam semantics, amsgrad off, L2
 * weight decay): the dense optimizer TZRecOptimizer.step() runs after the fused sparse backward
 * (tzrec/optim/optimizer.py:56-68; adam_optimizer of tzrec/optim/optimizer_builder.py).
 * Only tensors that have a gradient this step are passed; their step counts are incremented
 * here.  The learning rate is read from d_lr when non-null (so a captured hipGraph follows a
 * scheduler), else `lr`.  h_tensors is a HOST array; 32 tensors per launch pair. */
int tzr_dense_adam(const TzrAdamTensor* h_tensors, int n_tensors, const float* d_lr, float lr,
                   float beta1, float beta2, float eps, float weight_decay, void* stream);

/* The same Adam step in ONE launch, with gradients taken as they lie (csrc/adam_fused.hip): a finished tensor
 * (TZR_ADAM_SRC_TENSOR: TzrAdamTensor.grad), rows of per-workgroup partial sums left by tzr_mlp2_bwd_parts (TZR_ADAM_SRC_ROWS:
 * element i of the tensor = sum over the G rows of parts[g * P + col + i], added in tzr_mlp2_bwd's own finish order), or the
 * batch slices of tzr_dot_interaction_top_wgrad_parts (TZR_ADAM_SRC_WGRAD, at most one per call: *h_wgrad).  The column-sum
 * finish launches and the slice reduction of the DLRM step (tzrec/models/dlrm.py:101-135 behind tzrec/optim/optimizer.py:56-68)
 * disappear into the optimizer's launch.  The sums are bit-identical to the separate launches where the order of additions is
 * theirs: tzr_mlp2_bwd's finish (16 contiguous ranges of the G rows, then the 16 range sums) and the slice reduction of
 * tzr_dot_interaction_top_wgrad.  Partial rows whose separate finish is the interleaved one of csrc/parts_sum.h (tzr_relu_bwd_colsum_parts,
 * tzr_skinny_linear_bwd_parts) are added in THIS order too, not in that kernel's interleaved slices: equal to it up to fp32
 * rounding, and equal between every consumer of this summation (tzr_dense_adam_fused, tzr_dense_optim_fused, store-only calls).
 * Refused: TZR_ERR_UNSUPPORTED for a source that would need more than 1024 workgroups (the arrival counters of a state row);
 * TZR_ERR_INVALID for param == 0 && grad == 0 (nowhere to write).
 * TzrAdamTensor.state here: float[TZR_ADAM_FUSED_STATE]: [0] step count, [1 ..] arrival counters (ZERO between launches: the
 * tensor's workgroups arrive in groups of 32, the last one moves the step on and clears them) -- not interchangeable with
 * tzr_dense_adam's float[3] on the same tensor.
 * A tensor with param == 0 only gets its finished gradient stored into `grad` (for a caller that needs the tensor after all).
 * TZR_ADAM_SRC_TENSOR with `parts` != 0: the finished gradient is read from `parts` instead of `grad` -- with param == 0 a copy,
 * which makes ONE store-only call the packing of a model's gradients (finished or not) into a flat buffer for a collective.
 * h_sources NULL: every gradient is a finished tensor. */
#define TZR_ADAM_FUSED_STATE 40 /* 1 step + 1 + 32 counters (<= 1024 workgroups per tensor), padded */
#define TZR_ADAM_SRC_TENSOR 0
#define TZR_ADAM_SRC_ROWS 1
#define TZR_ADAM_SRC_WGRAD 2
typedef struct TzrAdamSource {
  int32_t kind, G, P, col;
  uint64_t parts; /* const float* device address of the partial-sum rows (TZR_ADAM_SRC_ROWS) */
  uint64_t reserved;
} TzrAdamSource; /* 32 bytes */
typedef struct TzrWgradParts { uint64_t opaque[24]; } TzrWgradParts; /* filled by tzr_dot_interaction_top_wgrad_parts */
int tzr_dense_adam_fused(const TzrAdamTensor* h_tensors, const TzrAdamSource* h_sources, int n_tensors,
                         const TzrWgradParts* h_wgrad, const float* d_lr, float lr, float beta1, float beta2, float eps,
                         float weight_decay, void* stream);
/* ... and, when one of the tensors is the W1 [64, 783] of the fused interaction layer (contiguous: ldw = 783), its packed copies
 * (tzr_ia_top_pack_w1) written by the thread that updates each element: plain stores in the same launch.  h_w1 null, or
 * h_w1->param not among the tensors: exactly tzr_dense_adam_fused.  Either copy may be 0. */
typedef struct TzrPackedW1 {
  uint64_t param;                  /* the parameter tensor the copies belong to (matched against TzrAdamTensor.param) */
  uint64_t fwd_packed, bwd_packed; /* float[tzr_ia_top_packed_floats()] each */
} TzrPackedW1; /* 24 bytes */
int tzr_dense_adam_fused_w1(const TzrAdamTensor* h_tensors, const TzrAdamSource* h_sources, int n_tensors,
                            const TzrWgradParts* h_wgrad, const float* d_lr, float lr, float beta1, float beta2, float eps,
                            float weight_decay, const TzrPackedW1* h_w1, void* stream);
/* The dense optimizer step of every kind `train_config.dense_optimizer` and its `part_optimizers` can name
 * (tzrec/optim/optimizer_builder.py:100-260 -> torch.optim.SGD / Adagrad / Adam / AdamW / Adadelta / RMSprop), over every
 * dense tensor of the step in ONE launch per TZR_ADAM_MAX_TENSORS tensors, whatever mix of kinds (csrc/dense_optim_fused.hip).
 * A tensor names its group; a group holds the kind, the learning rate (read from d_lr when non-zero, so a captured hipGraph
 * follows a scheduler; else `lr`) and the hyper-parameters.  Per element, torch.optim's single-tensor path in fp32, g the
 * gradient, p the parameter, wd = weight_decay:
 *   SGD       g += wd p;  state0 (momentum_buffer, only when hp0 = momentum != 0): buf = g on the tensor's first step (step
 *             count 0), else buf = momentum buf + (1 - hp1 = dampening) g;  TZR_DENSE_OPT_NESTEROV: g += momentum buf, else
 *             g = buf;  p -= lr g
 *   ADAGRAD   g += wd p;  state0 (sum, filled with initial_accumulator_value by the caller) += g^2;  p -= lr g / (sqrt(sum) + eps)
 *   ADAM      as tzr_dense_adam_fused: hp0 = beta1, hp1 = beta2, state0 = exp_avg, state1 = exp_avg_sq, L2 weight decay
 *   ADAMW     p *= 1 - lr wd, then ADAM without the L2 term
 *   ADADELTA  g += wd p;  state0 (square_avg) = rho sq + (1 - rho) g^2 (hp0 = rho);  d = sqrt(acc + eps) / sqrt(sq + eps) g;
 *             state1 (acc_delta) = rho acc + (1 - rho) d^2;  p -= lr d
 *   RMSPROP   g += wd p;  state0 (square_avg) = alpha sq + (1 - alpha) g^2 (hp0 = alpha);  p -= lr g / (sqrt(sq) + eps)
 * (no amsgrad, no lr_decay, no momentum / centered RMSprop: protos/optimizer.proto:159-208 has no such fields, or the caller
 * refuses them.)  `state`: float[TZR_ADAM_FUSED_STATE] as for tzr_dense_adam_fused: [0] the tensor's step count, moved on
 * by the last of its workgroups, [1 ..] arrival counters, zero between launches.  Gradient sources, store-only tensors
 * (param == 0; `group` is not read) and refusals as for tzr_dense_adam_fused: the summation is the same code.  Also refused,
 * before anything is launched: n_groups > TZR_DENSE_OPT_MAX_GROUPS (TZR_ERR_UNSUPPORTED); an unknown kind, a group index out
 * of range, a null state tensor that the kind needs, a null `state` (TZR_ERR_INVALID). */
#define TZR_DENSE_OPT_SGD 0
#define TZR_DENSE_OPT_ADAGRAD 1
#define TZR_DENSE_OPT_ADAM 2
#define TZR_DENSE_OPT_ADAMW 3
#define TZR_DENSE_OPT_ADADELTA 4
#define TZR_DENSE_OPT_RMSPROP 5
#define TZR_DENSE_OPT_MAX_GROUPS 8
#define TZR_DENSE_OPT_NESTEROV 1 /* TzrDenseOptGroup.flags */
typedef struct TzrDenseOptTensor { /* device addresses, float32 */
  uint64_t param, grad, state0, state1, state;
  int64_t numel;
  int32_t group, reserved;
} TzrDenseOptTensor; /* 56 bytes */
typedef struct TzrDenseOptGroup {
  int32_t kind, flags;
  uint64_t d_lr; /* const float* device address, or 0: `lr` */
  float lr, weight_decay, eps, hp0, hp1, reserved;
} TzrDenseOptGroup; /* 40 bytes */
int tzr_dense_optim_fused(const TzrDenseOptTensor* h_tensors, const TzrAdamSource* h_sources, int n_tensors,
                          const TzrDenseOptGroup* h_groups, int n_groups, const TzrWgradParts* h_wgrad, void* stream);
/* tzr_mlp2_bwd / tzr_dot_interaction_top_wgrad without their finishing launch (same arguments, same workspace, which stays the
 * caller's until tzr_dense_adam_fused has consumed it): *out_G rows of *out_P floats, columns [dWb: H2 x H1 | dbb: H2 |
 * dWa: H1 x K0 | dba: H1]; *h_out for TZR_ADAM_SRC_WGRAD (B > 0). */
int tzr_mlp2_bwd_parts(const float* d_dhb, int64_t dhb_stride, const float* d_hb, int64_t hb_stride, const float* d_ha,
                       int64_t ha_stride, const float* d_x, int64_t x_stride, int64_t B, int K0, int H1, int H2,
                       const float* d_Wb, void* ws, size_t ws_bytes, int* out_G, int* out_P, void* stream);
int tzr_dot_interaction_top_wgrad_parts(const float* d_dense, int64_t dense_stride, const float* d_sparse, int64_t sparse_stride,
                                        int F, int D, int64_t B, const float* d_g1, int64_t g1_stride, int H, const float* d_scale,
                                        void* d_ws, int64_t ws_bytes, TzrWgradParts* h_out, void* stream);

/* ---- zero-collision hash ---------------------------------------- */

#define TZR_ZCH_EMPTY INT64_MAX /* unoccupied cell / row (tzrec/utils/zch_util.py:29 ZCH_EMPTY_SLOT) */
#define TZR_ZCH_TOMB (INT64_MAX - 1) /* cell whose id was evicted (tzr_zch_update); as a raw id: served from the shared row, never admitted */

/* One managed-collision table: an open-addressing map raw id -> row plus per-row eviction metadata. */
typedef struct TzrZchModule {
  int64_t* keys;      /* [capacity] raw id per cell, TZR_ZCH_EMPTY when free                    */
  int32_t* rows;      /* [capacity] remapped row of the cell's id                               */
  int64_t* counts;    /* [zch_size] accesses per row           (written when profile != 0)      */
  int64_t* last_iter; /* [zch_size] iteration of the last access                                */
  int64_t capacity;   /* power of two, >= 2 * occupied rows                                     */
  int64_t zch_size;   /* rows of the embedding table; ids not in the map go to row zch_size-1   */
  int64_t reserved[2];
} TzrZchModule; /* 64 bytes */

/* K13: remap the ids of every KJT key through its module (d_key_module[key] = module index, -1 =
 * pass through).  Replaces torchrec MCHManagedCollisionModule.remap + .profile [upstream], built by
 * BaseFeature.mc_module (tzrec/features/feature.py:693-736) and applied in front of the lookup by
 * ManagedCollisionEmbeddingBagCollection (tzrec/modules/embedding.py:856-864).  profile != 0 also
 * bumps counts/last_iter of the rows hit and fills d_candidates (int64[n_values], positional):
 * the raw id where it has no row yet (an admission candidate), TZR_ZCH_EMPTY elsewhere.
 * d_out_values may alias d_values. */
int tzr_zch_remap(const TzrZchModule* d_modules, const int32_t* d_key_module, int n_keys,
                  const int64_t* d_values, const int64_t* d_offsets, int64_t B, int uniform_bag_len,
                  int64_t n_values, int64_t iter, int profile, int64_t* d_out_values,
                  int64_t* d_candidates, void* stream);

/* The same for a step that is replayed from a hipGraph: uniform bags only; the iteration number is read from DEVICE memory
 * (*d_iter: the caller bumps it inside the graph), and with profile != 0 the candidates of the step go to slot
 * `*d_iter % ring_slots` of d_cand_ring, int64 [ring_slots][n_cand_keys][B * uniform_bag_len]: one block per key that has
 * a module (d_key_cand[key] = its index among those keys, -1 for the others), the raw id where it has no row yet,
 * TZR_ZCH_EMPTY elsewhere.  Which step filled which slot is a function of the counter alone. */
int tzr_zch_remap_ring(const TzrZchModule* d_modules, const int32_t* d_key_module, int n_keys,
                       const int64_t* d_values, int64_t B, int uniform_bag_len, int64_t n_values,
                       const int64_t* d_iter, int profile, int64_t* d_out_values, const int32_t* d_key_cand,
                       int n_cand_keys, int64_t* d_cand_ring, int64_t ring_slots, void* stream);

/* Rebuild a module's map from n distinct (raw id, row) pairs (after admission / eviction, or when
 * restoring a checkpoint).  h_module is a HOST struct holding device pointers. */
int tzr_zch_build(const TzrZchModule* h_module, const int64_t* d_ids, const int32_t* d_rows,
                  int64_t n, void* stream);

/* The same after an admission / eviction round, touching only what changed: the n ids d_old_ids[i] (TZR_ZCH_EMPTY: the
 * row was free) leave the map, the n distinct ids d_new_ids[i] enter it with rows d_rows[i].  Evicted cells become
 * tombstones that later insertions reuse; the caller rebuilds (tzr_zch_build) when too many have piled up. */
int tzr_zch_update(const TzrZchModule* h_module, const int64_t* d_old_ids, const int64_t* d_new_ids,
                   const int32_t* d_rows, int64_t n, void* stream);

/* Admission / eviction round (torchrec MCHManagedCollisionModule eviction policies LFU / LRU / DistanceLFU
 * [upstream 1.7.0] as tzrec configures them, tzrec/features/feature.py:693-736, docs/source/feature/zch.md):
 * residents and candidates are ranked together (score descending, residents first, raw id ascending) and the first
 * zch_size - 1 stay.  The entries to drop are found by radix SELECTION on the reversed order instead of sorting:
 * tzr_zch_select_hist counts, over the residents (d_row_ids[r] != TZR_ZCH_EMPTY, r < zch_size - 1) and the n_new
 * candidates that match what is known of the threshold, one digit of the drop key
 *   field 0: bits [shift, shift + bits) of the score image, given its higher bits t1
 *   field 1: the kind (bin 0 candidates, bin 1 residents) of the entries whose score image is t1
 *   field 2: bits [shift, shift + bits) of the id image of the entries with score image t1 and kind t2, given its
 *            higher bits t3
 * into d_bins[2048] (uint64, zeroed by the call); the caller reads them, extends the threshold and calls again
 * (torcheasyrec_amd/zch.py: at most 13 passes, each ONE streaming read of the three per-row arrays).
 * policy: 0 LFU (count), 1 LRU (1 / age), 2 DistanceLFU (count / age), age = max(cur_iter - last, 1) ^ decay_exponent.
 * tzr_zch_select_mark then writes d_row_kept[zch_size - 1] / d_new_kept[n_new] = 1 for every entry ABOVE the threshold
 * (t1, t2, t3) (drop_none != 0: everything live stays).  h_module is a HOST struct holding device pointers. */
int tzr_zch_select_hist(const TzrZchModule* h_module, const int64_t* d_row_ids, const int64_t* d_new_ids,
                        const int64_t* d_new_cnt, int64_t n_new, int64_t cur_iter, int policy,
                        double decay_exponent, int field, int shift, int bits, uint64_t t1, int t2,
                        uint64_t t3, uint64_t* d_bins, void* stream);
int tzr_zch_select_mark(const TzrZchModule* h_module, const int64_t* d_row_ids, const int64_t* d_new_ids,
                        const int64_t* d_new_cnt, int64_t n_new, int64_t cur_iter, int policy,
                        double decay_exponent, int drop_none, uint64_t t1, int t2, uint64_t t3,
                        uint8_t* d_row_kept, uint8_t* d_new_kept, void* stream);

/* ---- small dense layer stacks (tzrec.modules.mlp.MLP, models/dlrm.py:101-135) ----------------
 * The MLPs stay on PyTorch / hipBLASLt in general; the three calls below take over the layer stacks whose GEMMs are
 * too skinny to be worth a launch each (N = 64 / 32 / 16 / 1): all fp32, row-major, `*_stride` in floats.
 * tzr_mlp2_fwd: ha = relu(x Wa^T + ba) [B, H1], hb = relu(ha Wb^T + bb) [B, H2]; Wa [H1, K0], Wb [H2, H1] as
 * nn.Linear stores them; K0 <= 32, H1 <= 64, H2 <= 32 (TZR_ERR_UNSUPPORTED beyond).
 * tzr_mlp2_bwd: from dhb = d(loss)/d(hb): the four parameter gradients (no input gradient: x is data).
 * tzr_mlp_tail: y2 = relu(y1 W2^T + b2), logit = y2 . w3 + b3, loss = mean BCE-with-logits(logit, label) -- and its
 * whole backward: g1 = d(loss)/d(pre-activation of y1) (y1 is a ReLU output: masked where y1 == 0), db1 = column sums
 * of g1 (the bias gradient of the layer that produced y1), dW2, db2, dw3, d_scalars = {d(loss)/d(b3), loss}.
 * ws: tzr_mlp_workspace() bytes.  Deterministic (fixed-order reductions).
 * Every operand may sit at any 4-byte-aligned address with any row stride: the general LDS-tiled kernels take whatever the
 * MFMA kernels (knob mlp_mfma) do not.  Those run when the shape is DLRM-Criteo's and their 16-byte accesses are aligned:
 *   tzr_mlp2_fwd          K0 <= 16, H1 = 64, H2 = 16; ha_stride % 4 == 0; d_ha and d_Wb 16-byte aligned
 *   tzr_mlp2_bwd / _parts K0 <= 16, H1 = 64, H2 = 16; ha_stride, hb_stride, dhb_stride % 4 == 0; d_ha, d_hb, d_dhb 16-byte aligned
 *   tzr_mlp_tail          H1 = 64, H2 = 32; y1_stride, g1_stride % 4 == 0; d_y1, d_g1 and d_W2 16-byte aligned
 * (x, x_stride, hb in the forward, the biases, w3, the labels and the outputs of the finish are read and written 4 bytes
 * at a time by both families.)  The two families add in different orders: equal within rounding, not bit for bit. */
size_t tzr_mlp_workspace(void);
int tzr_mlp2_fwd(const float* d_x, int64_t x_stride, int64_t B, int K0, const float* d_Wa, const float* d_ba, int H1,
                 const float* d_Wb, const float* d_bb, int H2, float* d_ha, int64_t ha_stride, float* d_hb,
                 int64_t hb_stride, void* stream);
int tzr_mlp2_bwd(const float* d_dhb, int64_t dhb_stride, const float* d_hb, int64_t hb_stride, const float* d_ha,
                 int64_t ha_stride, const float* d_x, int64_t x_stride, int64_t B, int K0, int H1, int H2,
                 const float* d_Wb, float* d_dWa, float* d_dba, float* d_dWb, float* d_dbb, void* ws, size_t ws_bytes,
                 void* stream);
int tzr_mlp_tail(const float* d_y1, int64_t y1_stride, const void* d_labels, int labels_itemsize, int labels_are_float,
                 int64_t B, int H1, const float* d_W2, const float* d_b2, int H2, const float* d_w3, const float* d_b3,
                 float* d_logits, float* d_g1, int64_t g1_stride, float* d_dW2, float* d_db2, float* d_dw3,
                 float* d_scalars, float* d_db1, void* ws, size_t ws_bytes, void* stream);

/* ---- sequence path --------------------------------------------- */

/* K12: jagged [N, dim] (+ offsets int64[B+1]) -> dense [B, max_len, dim]; positions past a
 * sample's length get padding_value, sequences longer than max_len are truncated.  Replaces fbgemm
 * jagged_to_padded_dense reached from JaggedTensor.to_padded_dense
 * (tzrec/modules/embedding.py:1429,1480).  The unpooled lookup itself is tzr_rows_gather with one
 * key segment per KJT key, its backward tzr_pooled_bwd_plan/apply with grad_mode 1. */
int tzr_jagged_to_padded_dense(const float* d_values, int64_t values_stride,
                               const int64_t* d_offsets, int64_t B, int64_t max_len, int dim,
                               float padding_value, float* d_out, void* stream);
/* backward of the above: d_values[offsets[b] + l, :] = d_dense[b, l, :] for l < min(len, max_len),
 * zero for truncated positions. */
int tzr_padded_dense_to_jagged(const float* d_dense, const int64_t* d_offsets, int64_t B,
                               int64_t max_len, int dim, float* d_values, int64_t values_stride,
                               void* stream);

/* Multi-valued sequence steps: replaces torch.segment_reduce(jt.values(), pooling,
 * lengths=key_lengths) + nan_to_num in SequenceEmbeddingGroupImpl
 * (tzrec/modules/embedding.py:1353-1366).  Segment s = rows [offsets[s], offsets[s+1]) of
 * d_values [N, dim]; mode 0 = sum, 1 = mean (an empty segment gives a zero row).
 * out [S, dim].  The backward writes every row of d_grad_values covered by a segment. */
int tzr_segment_reduce_fwd(const float* d_values, int64_t values_stride, const int64_t* d_offsets,
                           int64_t S, int dim, int mode, float* d_out, int64_t out_stride,
                           void* stream);
int tzr_segment_reduce_bwd(const float* d_grad_out, int64_t grad_out_stride,
                           const int64_t* d_offsets, int64_t S, int dim, int mode,
                           float* d_grad_values, int64_t grad_values_stride, void* stream);

/* DIN target attention over JAGGED positions: replaces DINEncoder.forward on padded [B, L, .] tensors
 * (tzrec/modules/sequence.py:101-128; the padding is SequenceEmbeddingGroupImpl's to_padded_dense,
 * tzrec/modules/embedding.py:1429-1480).  A position is a row of the unpooled lookup's output [N, D]; sample b owns rows
 * [offsets[b], offsets[b+1]); rows at index >= max_len inside a sample do not exist for the encoder (the padded length /
 * `max_seq_length`).  csrc/din_attention.hip states the masking semantics.  D, H multiples of 4, strides in floats
 * (multiples of 4), max_len <= 2048.
 *   tzr_jagged_segment_ids  d_seg[n] = sample of row n (B for rows at or behind offsets[B])
 *   tzr_din_assemble_fwd    X[n] = [ k_n | q_b * k_n | q_b ]  ([N, 3 D]): the input of the attention MLP whose first layer
 *                           W [q, k, q - k, q * k] the caller folds into [Wb - Wc | Wd | Wa + Wc]
 *   tzr_din_assemble_bwd    d_dkv[n] (+)= dX_n[0:D] + q_b * dX_n[D:2D];  d_dq[b] = sum_n (k_n * dX_n[D:2D] + dX_n[2D:3D])
 *   tzr_din_attn_fwd        s_n = h_n . w + bias[0]; p = softmax of s over a sample's rows; out[b] = sum_n p_n k_n
 *   tzr_din_attn_bwd        d_ds[n] = p_n (g_b . k_n - sum_m p_m g_b . k_m);  d_dkv[n] = p_n g_b
 * (the backward of s = h . w + bias is tzr_head_bwd on d_ds) */
int tzr_jagged_segment_ids(const int64_t* d_offsets, int64_t B, int64_t N, int32_t* d_seg, void* stream);
int tzr_din_assemble_fwd(const float* d_kv, int64_t kv_stride, const float* d_q, int64_t q_stride,
                         const int32_t* d_seg, int64_t B, int64_t N, int D, float* d_X, int64_t x_stride,
                         void* stream);
int tzr_din_assemble_bwd(const float* d_dX, int64_t x_stride, const float* d_kv, int64_t kv_stride,
                         const float* d_q, int64_t q_stride, const int32_t* d_seg, const int64_t* d_offsets,
                         int64_t B, int64_t N, int D, float* d_dkv, int64_t dkv_stride, int accumulate_dkv,
                         float* d_dq, int64_t dq_stride, void* stream);
/* The same pair with the query's own block left out of the rows: X[n] = [k_n | q_b * k_n] (2 D wide).  The first attention
 * layer W [q, k, q - k, q * k] = (Wb - Wc) k + Wd (q * k) + (Wa + Wc) q: its last term is one product per SAMPLE, added to the
 * per-position product as tzr_linear_rows' gathered row vector -- a third less contraction length than the 3 D form above.
 * Backward: dk_n (+)= dX_n[0:D] + q_b * dX_n[D:2D];  dq_b = sum_n k_n * dX_n[D:2D] + d_dq_add[b] (d_dq_add [B, D] or NULL: the
 * query's gradient through that per-sample term). */
int tzr_din_assemble2_fwd(const float* d_kv, int64_t kv_stride, const float* d_q, int64_t q_stride, const int32_t* d_seg, int64_t B,
                          int64_t N, int D, float* d_X, int64_t x_stride, void* stream);
int tzr_din_assemble2_bwd(const float* d_dX, int64_t x_stride, const float* d_kv, int64_t kv_stride, const float* d_q,
                          int64_t q_stride, const int32_t* d_seg, const int64_t* d_offsets, int64_t B, int64_t N, int D,
                          float* d_dkv, int64_t dkv_stride, int accumulate_dkv, const float* d_dq_add, int64_t dq_add_stride,
                          float* d_dq, int64_t dq_stride, void* stream);
int tzr_din_attn_fwd(const float* d_h, int64_t h_stride, int H, const float* d_w, const float* d_bias,
                     const float* d_kv, int64_t kv_stride, int D, const int64_t* d_offsets, int64_t B,
                     int64_t max_len, float* d_out, int64_t out_stride, float* d_p, void* stream);
int tzr_din_attn_bwd(const float* d_grad_out, int64_t grad_out_stride, const float* d_p, const float* d_kv,
                     int64_t kv_stride, int D, const int64_t* d_offsets, int64_t B, int64_t max_len, float* d_ds,
                     float* d_dkv, int64_t dkv_stride, void* stream);

/* The two cheap encoders of a DEEP group's `sequence_encoders`, over the same jagged rows: replace SimpleAttention.forward and
 * PoolingEncoder.forward on padded [B, L, D] tensors (tzrec/modules/sequence.py:131-218).  Conventions of tzr_din_attn_*: rows
 * [N, D], offsets int64[B+1], a position at index >= max_len inside a sample does not exist for the encoder; D a multiple of 4
 * and at most 256 (one lane per float4 piece of a row), strides in floats (multiples of 4), 16-byte aligned pointers;
 * TZR_ERR_UNSUPPORTED for a D, stride or max_len outside these limits, TZR_ERR_INVALID for a null or misaligned pointer;
 * B == 0 is TZR_OK without a launch, N == 0 needs no row pointer.  One wave per sample, fixed summation order, no atomics:
 * bit-reproducible.  csrc/jagged_encoders.hip.
 *   tzr_jagged_dot_attn_fwd  s_n = k_n . q_b; p = softmax of s over sample b's positions; out[b] = sum_n p_n k_n; d_p [N] is
 *                            written for the backward (0 for positions at or behind max_len).  max_len <= 2048 (a sample's
 *                            scores live in LDS).  The rows are read once where a wave holds them (16 * (64 / P) positions,
 *                            P = D / 4 rounded up to a power of two), twice for a longer sample.
 *   tzr_jagged_dot_attn_bwd  t_n = g_b . k_n; ds_n = p_n (t_n - sum_m p_m t_m); d_dkv[n] = p_n g_b + ds_n q_b (zero rows at or
 *                            behind max_len); d_dq[b] = sum_n ds_n k_n.
 *                            A sample with no position: out[b] = 0 and d_dq[b] = 0 (the reference's uniform softmax over zero
 *                            padding rows gives the same).
 *   tzr_jagged_pool_fwd      out[b] = sum of the first min(len, max_len) rows; mode TZR_POOL_MEAN divides by
 *                            max(min(len, max_len), 1).  Any max_len >= 0.
 *   tzr_jagged_pool_bwd      d_dkv[n] = g_b (mean: / the same count) for those rows, zero rows for positions at or behind
 *                            max_len (as tzr_padded_dense_to_jagged).  tzr_segment_reduce_* has no max_len and stays as it is.
 * Entry points only, no struct or constant changes: the ABI version stays 15. */
int tzr_jagged_dot_attn_fwd(const float* d_kv, int64_t kv_stride, const float* d_q, int64_t q_stride, int D,
                            const int64_t* d_offsets, int64_t B, int64_t N, int64_t max_len, float* d_out,
                            int64_t out_stride, float* d_p, void* stream);
int tzr_jagged_dot_attn_bwd(const float* d_grad_out, int64_t grad_out_stride, const float* d_p, const float* d_kv,
                            int64_t kv_stride, const float* d_q, int64_t q_stride, int D, const int64_t* d_offsets,
                            int64_t B, int64_t N, int64_t max_len, float* d_dkv, int64_t dkv_stride, float* d_dq,
                            int64_t dq_stride, void* stream);
int tzr_jagged_pool_fwd(const float* d_kv, int64_t kv_stride, int D, const int64_t* d_offsets, int64_t B, int64_t N,
                        int64_t max_len, int mode, float* d_out, int64_t out_stride, void* stream);
int tzr_jagged_pool_bwd(const float* d_grad_out, int64_t grad_out_stride, int D, const int64_t* d_offsets, int64_t B,
                        int64_t N, int64_t max_len, int mode, float* d_dkv, int64_t dkv_stride, void* stream);

/* The cross network of Deep & Cross v1, all L layers in one launch per direction: replaces Cross.forward and its autograd
 * (tzrec/modules/interaction.py:94-132).  csrc/cross_net.hip.
 *   tzr_cross_fwd  x_0 = x; s_l = x_l . w_l; x_{l+1} = s_l x_0 + b_l + x_l; d_y = x_L; d_s [B, L] contiguous (nullable: inference)
 *                  takes the scalars s for the backward.  One launch.
 *   tzr_cross_bwd  from g = d(loss)/d(y), x and s: d_dx [B, D], d_dw [L, D] and d_db [L, D] (contiguous; row l is the finished
 *                  gradient of w_l / b_l).  No x_l is read or stored: x_l = (1 + s_0 + .. + s_{l-1}) x + b_0 + .. + b_{l-1}.
 *                  Two launches: the pass over the batch, which leaves one row of partial sums per workgroup in `ws`
 *                  (tzr_cross_bwd_workspace(B, D, L) bytes, 256-byte aligned), and their sum in a fixed order.
 * h_w / h_b: HOST arrays of L device pointers (the reference's L separate [1, D] weights and [D] biases), read by the call and
 * passed to the kernels by value.  fp32; any D in [1, 1024], L in [1, 8], row strides (in floats) >= D; rows and parameters
 * need 4-byte alignment only.  TZR_ERR_INVALID: a null pointer (a misaligned workspace), B < 0, D <= 0, L <= 0;
 * TZR_ERR_UNSUPPORTED: D > 1024, L > 8, a stride below D, a workspace shorter than the query; B == 0 is TZR_OK without a
 * launch.  One wave per sample, no atomics, every sum over the batch in an order fixed by (B, D, L): bit-reproducible.
 * Entry points only, no struct or constant changes: the ABI version stays 15. */
int tzr_cross_fwd(const float* d_x, int64_t x_stride, const float* const* h_w, const float* const* h_b, int L, int64_t B, int D,
                  float* d_y, int64_t y_stride, float* d_s, void* stream);
size_t tzr_cross_bwd_workspace(int64_t B, int D, int L);
int tzr_cross_bwd(const float* d_grad_y, int64_t gy_stride, const float* d_x, int64_t x_stride, const float* d_s,
                  const float* const* h_w, const float* const* h_b, int L, int64_t B, int D, float* d_dx, int64_t dx_stride,
                  float* d_dw, float* d_db, void* ws, size_t ws_size, void* stream);

/* The low-rank cross network of Deep & Cross v2, all L layers in one launch forward and two launches backward: replaces
 * CrossV2.forward and its autograd (tzrec/modules/interaction.py:135-180).  csrc/cross_v2.hip.
 *   tzr_cross_v2_fwd  x_0 = x; t_l = x_l U_l^T [B, R]; y_l = t_l V_l^T + c_l; x_{l+1} = x_0 * y_l + x_l; d_y = x_L.  One launch; no
 *                     x_l passes through memory between layers.  Saved for the backward (both nullable: inference):
 *                     d_xs [L-1, B, D] contiguous = x_1 .. x_{L-1} (not read or written when L == 1), d_t [L, B, R] contiguous =
 *                     t_0 .. t_{L-1}.  y_l is never stored.
 *   tzr_cross_v2_bwd  from g = d(loss)/d(y), x, d_xs and d_t: d_dx [B, D], d_du [L, R, D], d_dv [L, D, R] and d_dc [L, D]
 *                     (contiguous; slice l is the finished gradient of U_l / V_l / c_l).  Two launches: the row pass, which
 *                     recomputes y_l from t_l, writes d_dx and leaves dy_l [L, B, D] and dt_l [L, B, R] in `ws`
 *                     (tzr_cross_v2_bwd_workspace(B, D, R, L) bytes, 256-byte aligned); and the weight-gradient pass, whose
 *                     workgroups each own a 16-wide strip of one dV_l (with dc_l) or dU_l over the whole batch.
 * h_u / h_v / h_c: HOST arrays of L device pointers (the reference's L separate [R, D] and [D, R] weights and [D] biases), read
 * by the call and passed to the kernels by value.  fp32; any D in [1, 1024], R in [1, 64], L in [1, 8], row strides (in floats)
 * >= D; rows and parameters need 4-byte alignment only.  TZR_ERR_INVALID: a null pointer (a misaligned workspace), B < 0,
 * D <= 0, R <= 0, L <= 0; TZR_ERR_UNSUPPORTED: D > 1024, R > 64, L > 8, a stride below D, a workspace shorter than the query;
 * B == 0 is TZR_OK without a launch.  Blocks of 16 rows per 256-thread workgroup, every product on the exact-fp32 MFMA.  No
 * atomics and no partial rows; reduction order: t_l and dt_l a wave its quarter of K = D on eight interleaved chains added as a fixed tree, then the waves 0..3; dV_l,
 * dU_l and dc_l a wave the 4-row steps w, w + 8, .. of the batch in order, then the waves 0..7 (dc_l: then the row residues
 * 0..3) -- fixed by (B, D, R, L): bit-reproducible.  Entry points only, no struct or constant changes: the ABI version stays 15. */
int tzr_cross_v2_fwd(const float* d_x, int64_t x_stride, const float* const* h_u, const float* const* h_v, const float* const* h_c,
                     int L, int64_t B, int D, int R, float* d_y, int64_t y_stride, float* d_xs, float* d_t, void* stream);
size_t tzr_cross_v2_bwd_workspace(int64_t B, int D, int R, int L);
int tzr_cross_v2_bwd(const float* d_grad_y, int64_t gy_stride, const float* d_x, int64_t x_stride, const float* d_xs, const float* d_t,
                     const float* const* h_u, const float* const* h_v, const float* const* h_c, int L, int64_t B, int D, int R,
                     float* d_dx, int64_t dx_stride, float* d_du, float* d_dv, float* d_dc, void* ws, size_t ws_size, void* stream);

/* LayerNorm, an optional ReLU and an optional elementwise mask over rows, up to eight outputs per launch: the non-GEMM work of
 * MaskNet (tzrec/modules/masknet.py:77-85, 142-161).  csrc/ln_mask.hip.
 *   tzr_ln_mask_fwd  f_j = act(LN(x_j; gamma_j, beta_j, eps)), act = ReLU (relu != 0) or identity; out_j = f_j * m_j, or f_j
 *                    when h_m is null.  shared_x != 0: every j reads x_0, gamma_0, beta_0 (the arrays h_x, h_x_stride, h_gamma,
 *                    h_beta hold ONE entry), the statistics are computed once and LN(x) is never stored; otherwise they hold
 *                    n_out entries.  d_stats [B, n_stat, 2] contiguous takes (mean, rstd), n_stat = 1 (shared) or n_out.
 *                    LN is nn.LayerNorm's (biased variance, eps inside the root), the variance a second pass over
 *                    (x - mean)^2.  One launch.
 *   tzr_ln_mask_bwd  from gout_j, the same x / gamma / beta / m and d_stats: gm_j = gout_j * f_j (with masks), the pre-mask
 *                    gradient sum_j gout_j * m_j (shared) or gout_j * m_j through the ReLU mask (recomputed by the
 *                    forward's instruction sequence) and LN's backward into gx_j (n_stat of them), d_dgamma and d_dbeta
 *                    [n_stat, D] contiguous, finished.  Two launches: the pass over the batch, which leaves one row of
 *                    partial sums per workgroup in `ws` (tzr_ln_mask_bwd_workspace bytes, 256-byte aligned), and their sum in
 *                    a fixed order.
 * Every h_* is a HOST array (of device pointers, or of row strides in floats), read by the call and passed to the kernels by
 * value; x_j, m_j, out_j, gout_j, gx_j, gm_j may be column slices of wider tensors.  fp32; D in [1, 1024], n_out in [1, 8],
 * strides >= D, 4-byte alignment.  TZR_ERR_INVALID: a null pointer (h_m / h_m_stride / h_gm / h_gm_stride may be null
 * together: no masks), a misaligned workspace, B < 0, D <= 0, n_out <= 0; TZR_ERR_UNSUPPORTED: D > 1024, n_out > 8, a stride
 * below D, a workspace shorter than the query; B == 0 is TZR_OK without a launch.  One wave per sample, no atomics, every
 * sum over the batch in an order fixed by (B, D, n_out, shared_x): bit-reproducible.  Entry points only: the ABI version stays 15. */
int tzr_ln_mask_fwd(const float* const* h_x, const int64_t* h_x_stride, const float* const* h_gamma, const float* const* h_beta,
                    const float* const* h_m, const int64_t* h_m_stride, float* const* h_out, const int64_t* h_out_stride, int n_out,
                    int shared_x, int relu, float eps, int64_t B, int D, float* d_stats, void* stream);
size_t tzr_ln_mask_bwd_workspace(int64_t B, int D, int n_out, int shared_x);
int tzr_ln_mask_bwd(const float* const* h_gout, const int64_t* h_gout_stride, const float* const* h_x, const int64_t* h_x_stride,
                    const float* const* h_gamma, const float* const* h_beta, const float* const* h_m, const int64_t* h_m_stride,
                    const float* d_stats, int n_out, int shared_x, int relu, int64_t B, int D, float* const* h_gx,
                    const int64_t* h_gx_stride, float* const* h_gm, const int64_t* h_gm_stride, float* d_dgamma, float* d_dbeta,
                    void* ws, size_t ws_size, void* stream);

/* The compressed interaction network of xDeepFM: replaces CIN.forward and its autograd (tzrec/modules/interaction.py:183-233),
 * which per layer build z = einsum("bhd,bfd->bhfd") as a [B, H F, D] tensor and keep it for the backward.  csrc/cin.hip; z is
 * never built, forward or backward.  x is the group tensor [B, F D] (X0[f, (b, d)] = x[b, f D + d]), H_0 = F, H_{i+1} = O_i:
 *   tzr_cin_fwd   X^{i+1}[b, o, d] = c_i[o] + sum_{h,f} W_i[o, h F + f] X^i[b, h, d] X0[b, f, d];  d_y[b, O_0 + .. + O_{i-1} + o] =
 *                 sum_d X^{i+1}[b, o, d].  ONE launch for every layer.  h_xs: HOST array of L - 1 device pointers, h_xs[i] takes
 *                 X^{i+1} [B, O_i, D] contiguous, the saved state of the backward (nullable, or null entries: inference; X^L is
 *                 only pooled and never stored).
 *   tzr_cin_bwd   from d_grad_y [B, sum O], x and the saved h_xs: d_gx [B, F D], and in d_dwc, contiguous, per layer dW_i
 *                 [O_i, H_i F] followed by dc_i [O_i].  The saved state is CONSUMED: on return h_xs[i] holds dX^{i+1} (a second
 *                 backward needs a second forward); this is what keeps the backward free of any [B, O, D] temporary.  2 L + 1
 *                 launches: per layer the weight gradient (a workgroup owns its output tile and walks its part of the columns;
 *                 the layer's S_i parts, a function of the shapes alone, lie in `ws`) and the input gradients, then one launch that
 *                 adds every layer's parts 0..S_i-1.
 *                 `ws`: tzr_cin_bwd_workspace bytes, 256-byte aligned.
 * h_w / h_c: HOST arrays of L device pointers (Conv1d weight [O_i, H_i F, 1] and bias [O_i], contiguous); h_layers: HOST
 * array of the L sizes O_i.  fp32; D in [1, 64], F in [1, 64], O_i in [1, 256], L in [1, 4], B < 2^30; row strides (floats) of x
 * and gx >= F D, of y and grad_y >= sum O.  Every pointer needs 4-byte alignment only (single-float loads and stores), so a
 * column slice of a wider tensor is taken as it lies.  TZR_ERR_INVALID: a null pointer, B < 0, a size <= 0;
 * TZR_ERR_UNSUPPORTED: outside the limits above; TZR_ERR_WORKSPACE: `ws` null, misaligned or shorter than the query less its
 * 256 bytes of slack.  Every check precedes the first launch; B == 0 is TZR_OK without a launch.  No atomics; every sum's order
 * is a function of the shapes alone: bit-reproducible.  Entry points only: the ABI version stays 15. */
int tzr_cin_fwd(const float* d_x, int64_t x_stride, const float* const* h_w, const float* const* h_c, const int* h_layers, int L,
                int64_t B, int F, int D, float* const* h_xs, float* d_y, int64_t y_stride, void* stream);
size_t tzr_cin_bwd_workspace(int64_t B, int F, int D, const int* h_layers, int L);
int tzr_cin_bwd(const float* d_grad_y, int64_t gy_stride, const float* d_x, int64_t x_stride, const float* const* h_w,
                const int* h_layers, int L, int64_t B, int F, int D, float* const* h_xs, float* d_gx, int64_t gx_stride,
                float* d_dwc, void* ws, size_t ws_size, void* stream);

/* The two per-sample operations of a WuKong layer outside its GEMMs (tzrec/modules/interaction.py:236-378).  csrc/wukong.hip.
 * Per sample X [F, D] (row-major in x), k = compressed_feature_num, Fo = Ff + Fl (fmb_feature_num + lcb_feature_num):
 *   tzr_wukong_fm_fwd   P = X^T W [D, k], Z = X P [F, k], d_out[b, :] = LN(vec(Z); gamma, beta, eps) over the F k values; W is
 *                       fmb.weight [F, k], gamma / beta [F k].  d_stats [B, 2] contiguous takes (mean, rstd); P and Z never
 *                       reach memory.  One launch.
 *   tzr_wukong_fm_bwd   from gout, x, W, gamma and d_stats (P, Z recomputed): gX [B, F, D] into d_gx, and d_dparams =
 *                       [dW F k | dgamma F k | dbeta F k] contiguous, finished.
 *   tzr_wukong_mix_fwd  pre[o, :] = (o < Ff ? Fm[o, :] : 0) + sum_f Wc[f, o] X[f, :], Wc[f, o] = Wr[f, o] + (o >= Ff ? Wl[f, o - Ff] : 0),
 *                       d_out[b, o, :] = LN(pre[o, :]; gamma, beta, eps) over D.  Fm [Ff, D] per sample in d_fm (feature_out_liner's
 *                       row as it lies), Wl = lcb.weight [F, Fl], Wr = residual_projection.weight [F, Fo]; d_wr null: the
 *                       identity residual (Wr[f, o] = (f == o), needs F == Fo).  d_stats [B, Fo, 2] contiguous.  One launch.
 *   tzr_wukong_mix_bwd  from gout, x, fm, Wl, Wr, gamma and d_stats (pre recomputed): gX into d_gx, gFm [B, Ff, D] into d_gfm,
 *                       and d_dparams = [dWr F Fo | dWl F Fl | dgamma D | dbeta D] contiguous, finished (dWr is written with a
 *                       null d_wr too, and then means nothing).
 * Each backward is two launches: the pass over the batch, which leaves one row of partial sums (the layout of d_dparams) per
 * workgroup in `ws` (the *_bwd_workspace query's bytes, 256-byte aligned), and their sum in the interleaved order above.  LN is
 * nn.LayerNorm's (biased variance, eps inside the root, the variance a second pass).  fp32; F, Fo, k in [1, 64], Ff, Fl >= 1, D in
 * [1, 128], B < 2^30; strides are floats per sample, >= the sample's width (F D, F k, Ff D, Fo D); single-float loads and stores:
 * 4-byte alignment, a column slice of a wider tensor is taken as it lies.  TZR_ERR_INVALID: a null pointer (d_wr excepted), B < 0,
 * a size <= 0; TZR_ERR_UNSUPPORTED: outside the limits, a short stride, d_wr null with F != Fo; TZR_ERR_WORKSPACE: `ws` null,
 * misaligned or shorter than the query less its 256 bytes of slack.  Every check precedes the first launch; B == 0 is TZR_OK
 * without a launch.  No atomics; every sum's order is a function of the shapes alone: bit-reproducible.  Entry points only: the
 * ABI version stays 15. */
int tzr_wukong_fm_fwd(const float* d_x, int64_t x_stride, const float* d_w, const float* d_gamma, const float* d_beta, float eps,
                      int64_t B, int F, int D, int k, float* d_out, int64_t out_stride, float* d_stats, void* stream);
size_t tzr_wukong_fm_bwd_workspace(int64_t B, int F, int D, int k);
int tzr_wukong_fm_bwd(const float* d_gout, int64_t gout_stride, const float* d_x, int64_t x_stride, const float* d_w,
                      const float* d_gamma, const float* d_stats, int64_t B, int F, int D, int k, float* d_gx, int64_t gx_stride,
                      float* d_dparams, void* ws, size_t ws_size, void* stream);
int tzr_wukong_mix_fwd(const float* d_x, int64_t x_stride, const float* d_fm, int64_t fm_stride, const float* d_wl, const float* d_wr,
                       const float* d_gamma, const float* d_beta, float eps, int64_t B, int F, int D, int Ff, int Fl, float* d_out,
                       int64_t out_stride, float* d_stats, void* stream);
size_t tzr_wukong_mix_bwd_workspace(int64_t B, int F, int D, int Ff, int Fl);
int tzr_wukong_mix_bwd(const float* d_gout, int64_t gout_stride, const float* d_x, int64_t x_stride, const float* d_fm, int64_t fm_stride,
                       const float* d_wl, const float* d_wr, const float* d_gamma, const float* d_stats, int64_t B, int F, int D, int Ff,
                       int Fl, float* d_gx, int64_t gx_stride, float* d_gfm, int64_t gfm_stride, float* d_dparams, void* ws,
                       size_t ws_size, void* stream);

/* ---- native step driver (csrc/step_driver.hip) ------------------------------------------------------------------
 * Replaces the host side of a steady-state train step of tzrec's pipeline (tzrec/utils/dist_util.py:221-303: Python +
 * torch.distributed calls per collective) for a sharded step that was cut into captured hipGraphs: ONE call queues the
 * graphs and the RCCL collectives between them.
 *
 * Communicator: RCCL reached through the librccl the process already holds (`librccl_path`: e.g. <torch>/lib/librccl.so;
 * NULL = default search); rank 0 makes the 128-byte unique id, the launcher carries it to every rank (torch.distributed's
 * store or one broadcast), every rank calls tzr_comm_create.  tzr_comm_all_to_all / _all_reduce are in stream order on
 * `stream` (bytes_per_peer: what each rank sends to and receives from every rank; all-reduce: fp32 sum or average).
 * Program: ops recorded once (tzr_step_add_*: each returns the op's index >= 0, or a negative TZR_ERR_*), replayed by
 * tzr_step_run: a graph op is hipGraphLaunch on `stream`; a collective runs on the program's own communication stream
 * behind everything queued on `stream` so far (sync != 0: `stream` waits for it on the spot; else a later wait op does);
 * nothing allocates, nothing synchronises the host.  Buffers and graph handles must outlive the program. */
int tzr_comm_available(const char* librccl_path); /* 1 / 0 */
int tzr_comm_version(const char* librccl_path);   /* ncclGetVersion, -1 when RCCL is not reachable */
int tzr_comm_unique_id(const char* librccl_path, void* out, size_t out_bytes); /* out_bytes >= 128 */
int tzr_comm_create(const char* librccl_path, const void* unique_id, size_t id_bytes, int world, int rank,
                    void** out_comm);
int tzr_comm_destroy(void* comm);
int tzr_comm_all_to_all(void* comm, const void* d_send, void* d_recv, int64_t bytes_per_peer, void* stream);
int tzr_comm_all_reduce(void* comm, float* d_buf, int64_t count, int average, void* stream);
int tzr_step_create(void** out_program);
int tzr_step_destroy(void* program);
int tzr_step_add_graph(void* program, void* graph_exec /* hipGraphExec_t */);
int tzr_step_add_all_to_all(void* program, void* comm, const void* d_send, void* d_recv, int64_t bytes_per_peer, int sync);
int tzr_step_add_all_reduce(void* program, void* comm, float* d_buf, int64_t count, int average, int sync);
int tzr_step_add_wait(void* program, int collective_op);
int tzr_step_num_ops(void* program);
int tzr_step_run(void* program, void* stream);

/* ---- export ------------------------------------------------------------------------------ */

/* Row-wise INT8 export of a table: replaces _quantize_quint8_rowwise_f16
 * (tzrec/utils/quant_util.py:25-131; reached from tzrec/utils/export_util.py:2353 and the
 * delta-embedding dump).  d_out[rows, dim + 4] bytes per row:
 * [dim uint8 values][float16 scale][float16 offset] (QUint8RowwiseF16), byte-exact with the
 * reference encoder.  d_w: float or (w_dtype = TZR_DT_F16) half rows, w_stride ELEMENTS apart.
 * d_first_bad: int64[3] device scratch; after the stream has drained it holds the smallest row
 * index with (0) a non-finite value, (1) an offset, (2) a scale outside the finite float16 range,
 * INT64_MAX where there is none -- the conditions the reference raises ValueError for; such rows'
 * output bytes are unspecified. */
int tzr_quantize_rows_q8f16(const void* d_w, int w_dtype, int64_t w_stride, int64_t rows, int dim,
                            uint8_t* d_out, int64_t* d_first_bad, void* stream);
/* dequantize_quint8_rowwise_f16 (tzrec/utils/quant_util.py:158-196): out[r, c] = q * scale + offset
 * (product rounded first), float32 [rows, dim]. */
int tzr_dequantize_rows_q8f16(const uint8_t* d_rows, int64_t rows, int dim, float* d_out,
                              int64_t out_stride, void* stream);

/* ---- delta-embedding tracker ---------------------------------------- */

/* Which rows were looked up since the last dump.  Replaces the id store of tzrec's ModelDeltaTracker
 * (tzrec/utils/delta_embedding_dump.py:352-641): torchrec DeltaStoreTrec.append per lookup (:478-513)
 * and compact / torch.cat(...).unique() per dump (:565-609).  Here the touched set of a table is a
 * bitmap in HBM, one bit per LOCAL row, uint32 words, (rows + 31) / 32 of them, bit r & 31 of word
 * r >> 5; the caller owns and zero-initialises it. */
typedef struct TzrDeltaSeg {
  uint32_t* bitmap; /* bitmap of the table this lookup segment reads; NULL = segment not tracked */
  int64_t rows;     /* local rows of that table: ids outside [0, rows) are counted, not marked   */
  int32_t key;      /* key segment of the id array the lookup reads (see tzr_delta_mark)         */
  int32_t reserved;
} TzrDeltaSeg; /* 24 bytes */

/* record_lookup (delta_embedding_dump.py:478-513): mark the ids of n_segs lookup segments.  Segment
 * s covers ids [o(k), o(k+1)) with k = d_segs[s].key and o(k) = d_key_offsets[k * key_stride], or
 * k * key_stride * uniform_len when d_key_offsets is NULL (a KJT: key_stride = B and the offsets
 * array, or uniform bags; the owner side of the sharded exchange: key_stride = 1 and the received
 * key starts).  *d_oob (nullable, caller-zeroed accumulator) += ids outside their table -- the
 * condition the reference raises ValueError for at dump time (:1026-1035). */
int tzr_delta_mark(const TzrDeltaSeg* d_segs, int n_segs, const int64_t* d_ids,
                   const int64_t* d_key_offsets, int64_t key_stride, int64_t uniform_len,
                   int64_t n_ids, int64_t* d_oob, void* stream);
/* get_unique (:565-609): *d_total += number of marked rows (caller-zeroed accumulator). */
size_t tzr_delta_collect_workspace(int64_t rows);
int tzr_delta_count(const uint32_t* d_bitmap, int64_t rows, int64_t* d_total, void* ws,
                    size_t ws_bytes, void* stream);
/* ... and the marked rows themselves, ascending, as id_base + local row (the reference's
 * ids.unique(sorted=True) + shard row_offset, :976,1036) into d_out_ids[0 : min(count, capacity)];
 * clear != 0 zeroes the bitmap in the same pass (delete_on_read). */
int tzr_delta_collect(uint32_t* d_bitmap, int64_t rows, int64_t id_base, int clear,
                      int64_t* d_out_ids, int64_t capacity, void* ws, size_t ws_bytes, void* stream);

/* Process-wide knobs; returns TZR_ERR_INVALID for unknown names.  Every knob, with its default; "tests only" = a hook that
 * forces a path, or caps a grid, so that a small input reaches code the library otherwise picks at production sizes.
 *   fwd_tile_b          0: samples per workgroup of the pooled forward (0 = by problem size)
 *   fwd_variant         0: pooled forward kernel by shape; 1 = the general kernel only, 2 = the LDS-ids kernel whenever
 *                       eligible (tests only)
 *   fwd_plan            1: tzr_pooled_fwd_cells_plan from B = 32 768 up; 0 = never, 2 = at any batch size (tests only)
 *   bwd_ch              0: lookups per chunk of the backward plan: 256 / 512 / 768 / 1024 (0 = by problem size)
 *   bwd_force_prep      0; 1: geometry prologue as its own launch (the > 1024 features path; tests only)
 *   bwd_one_wg_heavy    0; 1: a heavy bucket of the backward plan is sorted by ONE workgroup instead of one per
 *                       1024-lookup tile.  Same plan, slower under heavy skew.  Set it when plans are built on a
 *                       stream other than the one the rest of the step runs on (NOTES.md, "Side-stream plan").
 *   bwd_no_fuse_sort    0; 1: every unit of the backward plan is sorted by the sort launch, so that
 *                       tzr_pooled_bwd_plan_view shows the complete sorted pairs (tests only)
 *   bwd_direct          0: tzr_pooled_bwd_direct_supported says yes up to 16 384 lookups per table on average;
 *                       1 = at any size, -1 = never (tests only)
 *   bwd_direct_ch       0: lookups per workgroup of tzr_pooled_bwd_direct by problem size; 64 .. 1024 = that many (tests only)
 *   bwd_direct_hot      1: tzr_pooled_bwd_direct shares a hot row among a table's workgroups when the caller sets
 *                       TZR_GRAD_HOT_ROWS; 0 = never, 2 = always (tests only)
 *   bwd_direct_debug    0; 5: only the row-split workgroups of tzr_pooled_bwd_direct run (wrong results; tests only)
 *   ia_bwd_wgs          0: workgroups of the D = 16 dot-interaction backward by batch size (at most 3 072); > 0 = at most
 *                       that many
 *   ia_fwd_wgs          0: workgroups of the D = 16 dot-interaction forward by batch size; > 0 = at most that many
 *   ia_gen_wgs          0: workgroups of the generalised MFMA backward (D != 16 or 33-64 rows) = the resident set; > 0 = at
 *                       most that many
 *   it_wgs              0: persistent workgroups of the fused interaction + first-layer kernels = 256, one per CU
 *   it_fwd_stagger      0: fused interaction forward, half of the waves build the next tile's row before the product and half
 *                       behind it when z is written, all behind when not; 1 = half and half, 2 / 3 = all before / all behind
 *   wg_debug            0; phase-skipping bits of tzr_dot_interaction_top_wgrad for timing experiments (wrong results).  Kept:
 *                       without the run-time guard around its product the kernel's tile loop compiles to a slower schedule
 *   mlp_mfma            0: the MFMA kernels of mlp_mfma.hip where the shape is DLRM-Criteo's; -1: tzr_mlp2_* / tzr_mlp_tail
 *                       use their general LDS-tiled kernels for every shape (tests only); > 0: as 0, and the MFMA kernels
 *                       launch at most that many workgroups of four waves, one 16-sample tile per wave and turn (tests only:
 *                       several turns per wave on small batches; the general kernels ignore it)
 *   linear_bwd_wg       0; > 0 caps the workgroups of tzr_linear_bwd_relu (many tiles per workgroup on small inputs; tests only)
 *   gemm_rows_wg        0; > 0 caps the workgroups of tzr_linear_rows and tzr_linear_rows_wgrad (tests only) */
int tzr_tune(const char* name, int value);

/* ---- feature interaction ----------------------------------------------------------------- */

/* K9: DLRM dot interaction.  Replaces tzrec InteractionArch.forward
 * (tzrec/modules/interaction.py:80-91: bmm(X, X^T) then strict-upper-triangle gather, row-major
 * (i<j) order) fused with the concatenations of DLRM.predict (tzrec/models/dlrm.py:123-130).
 * X[b] = [dense[b] (optional, row 0); sparse[b, 0:F*D] as F rows of D].  n = F + (dense!=0).
 * out[b, 0 : n(n-1)/2] = X X^T upper triangle (exact fp32);
 * if cat_dense: out[b, P : P+D] = dense[b]; if cat_sparse: the F*D sparse floats follow.
 * D = 16 with n <= 32 (DLRM-Criteo) runs kernels specialised for that shape; any other D % 4 == 0
 * with n <= 64 the same MFMA 16x16x4 f32 scheme generalised (2 or 4 row blocks, a loop over
 * 16-column blocks of D); n > 64 a general LDS-staged VALU kernel, as long as one sample fits its
 * 60 KB of LDS: n (D + 1) floats forward, n (D + 1) + n (n + 1) backward; beyond that
 * TZR_ERR_UNSUPPORTED. */
int tzr_dot_interaction_fwd(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                            int64_t sparse_stride, int F, int D, int64_t B, float* d_out,
                            int64_t out_stride, int cat_dense, int cat_sparse, void* stream);
/* backward: dX = (G + G^T) X with G the upper-triangular gradient; concatenated pass-through
 * gradients are added.  d_grad_dense may be null when d_dense is null. */
int tzr_dot_interaction_bwd(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                            int64_t sparse_stride, int F, int D, int64_t B,
                            const float* d_grad_out, int64_t grad_out_stride, int cat_dense,
                            int cat_sparse, float* d_grad_dense, int64_t grad_dense_stride,
                            float* d_grad_sparse, int64_t grad_sparse_stride, void* stream);

/* K9b: the dot interaction FUSED with the first Linear of the MLP behind it (DLRM.predict,
 * tzrec/models/dlrm.py:123-135: `final_mlp(cat(interaction, dense, sparse))`, first layer [P + D n -> H]).
 * Layout of the interaction row as tzr_dot_interaction_fwd writes it with cat_dense = (dense != 0), cat_sparse = 1:
 * [P pairs | dense row | sparse rows], width P + D n.  W1 is the nn.Linear weight [H, ldw >= width], row-major.
 * Supported: D = 16, H = 64, ceil(P / 16) + n <= 64 column blocks, i.e. n <= 32 (tzr_dot_interaction_top_supported;
 * otherwise TZR_ERR_UNSUPPORTED and the caller runs the unfused ops).  Up to n = 29 the backward keeps two dz tiles in
 * LDS (one barrier per tile); n = 30 .. 32 run the same kernel with one tile (two barriers), same results.  fp32 MFMA, fixed summation order (deterministic).
 * B <= 2^30 samples per call (the kernels count tiles and samples in 32 bits; more: TZR_ERR_UNSUPPORTED).
 *   _top_fwd: y1[b] = act(z[b] W1^T + bias) (relu != 0: ReLU), [B, H]; the interaction row z[b] itself is written
 *             only when d_z is non-null (training keeps it for the weight gradient; inference does not need it).
 *   _top_bwd: from g1 = d(loss)/d(z W1^T + bias) [B, H]: grad_dense / grad_sparse = the interaction backward of
 *             dz = scale * g1 W1, with dz never leaving the chip.  d_scale: device scalar or null (= 1). */
int tzr_dot_interaction_top_supported(int F, int D, int has_dense, int H);
int tzr_dot_interaction_top_fwd(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                int64_t sparse_stride, int F, int D, int64_t B, const float* d_W1, int64_t ldw,
                                const float* d_bias, int H, int relu, float* d_z, int64_t z_stride, float* d_y1,
                                int64_t y1_stride, void* stream);
int tzr_dot_interaction_top_bwd(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1, int64_t g1_stride,
                                int H, const float* d_W1, int64_t ldw, const float* d_scale, float* d_grad_dense,
                                int64_t grad_dense_stride, float* d_grad_sparse, int64_t grad_sparse_stride,
                                void* stream);
/* W1 in the order of the two kernels' MFMA fragments (csrc/interaction_pack.h), for the DLRM-Criteo shape (n = 27 vectors with
 * the dense one, D = 16, H = 64).  Out of the plain matrix every persistent workgroup re-orders the 200 KB through LDS before its
 * first tile; out of a packed copy its lanes load their registers directly.  Same numbers in the same registers: results are
 * bit-identical to the plain entry points.
 *   tzr_ia_top_packed_floats: floats of either copy (16-byte aligned buffers).
 *   tzr_ia_top_pack_w1: both copies (either pointer may be null) of W1 [64, ldw]; n != 27: TZR_ERR_UNSUPPORTED.
 *   _top_fwd_packed / _top_bwd_packed: the plain entry points with the matching copy; null, d_z != null (forward) or another
 *   shape: the copy is not read and W1 is staged as ever.  `scale` stays a multiply in the backward kernel.
 * The copies are the caller's to keep equal to W1: tzr_dense_adam_fused_w1 writes them in the optimizer's launch. */
int tzr_ia_top_packed_floats(void);
int tzr_ia_top_pack_w1(const float* d_W1, int64_t ldw, int n, float* d_fwd_packed, float* d_bwd_packed, void* stream);
int tzr_dot_interaction_top_fwd_packed(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                       int64_t sparse_stride, int F, int D, int64_t B, const float* d_W1, int64_t ldw,
                                       const float* d_bias, int H, int relu, float* d_z, int64_t z_stride, float* d_y1,
                                       int64_t y1_stride, const float* d_W1_fwd_packed, void* stream);
int tzr_dot_interaction_top_bwd_packed(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                       int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1, int64_t g1_stride,
                                       int H, const float* d_W1, int64_t ldw, const float* d_scale, float* d_grad_dense,
                                       int64_t grad_dense_stride, float* d_grad_sparse, int64_t grad_sparse_stride,
                                       const float* d_W1_bwd_packed, void* stream);

/* K9c: the weight gradient of that first Linear, dW1 = scale * g1^T z [H, P + D n] (autograd of nn.Linear in
 * tzrec/modules/mlp.py:58-83 behind tzrec/models/dlrm.py:123-135), with the interaction rows z REBUILT from the
 * embeddings on the chip: training does not keep z (tzr_dot_interaction_top_fwd with d_z = null).  Same shapes as
 * tzr_dot_interaction_top_supported; exact-fp32 MFMA; the batch is summed in a fixed order (run-to-run identical).
 * d_ws: tzr_dot_interaction_top_wgrad_workspace(F, D, has_dense, H) bytes, 16-byte aligned (partial sums of the batch
 * slices).  d_scale: device scalar or null (= 1).  d_dW1 row pitch ldw >= P + D n; columns behind the width are left alone.
 * B = 0 writes zeros (the width still follows from F and whether d_dense is null). */
int64_t tzr_dot_interaction_top_wgrad_workspace(int F, int D, int has_dense, int H);
int tzr_dot_interaction_top_wgrad(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                  int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1, int64_t g1_stride,
                                  int H, const float* d_scale, float* d_dW1, int64_t ldw, void* d_ws, int64_t ws_bytes,
                                  void* stream);

/* Two pairs of those launches as ONE launch each (csrc/interaction_phases.hip), DLRM-Criteo shape only (26 sparse vectors + the
 * dense one, D = 16, H = 64): the neighbour runs as a phase of the persistent interaction kernel, on the samples the workgroup
 * owns anyway.  Same bodies, same order of every addition: outputs bit-identical to the two calls they stand for.  (Added without
 * a change to an existing signature or struct: the version stays, a library without them fails to bind.)
 *   _top_fwd_mlp2: tzr_mlp2_fwd (its arguments first, without the stream) then tzr_dot_interaction_top_fwd_packed (its arguments,
 *             without B) with the bottom MLP's output as the dense vector: d_dense == d_hb and dense_stride == hb_stride.  Writes
 *             ha, hb and y1.  TZR_ERR_UNSUPPORTED for anything else than K0 <= 16, H1 = 64, H2 = 16 (16-byte aligned Wb and ha
 *             rows), F = 26, d_z = null and a packed copy of W1.
 *   _top_bwd_wgrad_parts: tzr_dot_interaction_top_bwd_packed (its arguments, without the stream) then the workspace and the
 *             blob of tzr_dot_interaction_top_wgrad_parts: grad_dense / grad_sparse, and the weight gradient's batch slices in
 *             d_ws described by *h_out for tzr_dense_adam_fused.  d_scale applies to both.  B > 0; d_dense non-null, F = 26. */
int tzr_dot_interaction_top_fwd_mlp2(const float* d_x, int64_t x_stride, int64_t B, int K0, const float* d_Wa, const float* d_ba, int H1,
                                     const float* d_Wb, const float* d_bb, int H2, float* d_ha, int64_t ha_stride, float* d_hb,
                                     int64_t hb_stride, const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                     int64_t sparse_stride, int F, int D, const float* d_W1, int64_t ldw, const float* d_bias, int H,
                                     int relu, float* d_z, int64_t z_stride, float* d_y1, int64_t y1_stride,
                                     const float* d_W1_fwd_packed, void* stream);
int tzr_dot_interaction_top_bwd_wgrad_parts(const float* d_dense, int64_t dense_stride, const float* d_sparse, int64_t sparse_stride,
                                            int F, int D, int64_t B, const float* d_g1, int64_t g1_stride, int H, const float* d_W1,
                                            int64_t ldw, const float* d_scale, float* d_grad_dense, int64_t grad_dense_stride,
                                            float* d_grad_sparse, int64_t grad_sparse_stride, const float* d_W1_bwd_packed, void* d_ws,
                                            int64_t ws_bytes, TzrWgradParts* h_out, void* stream);

/* K10: FM second order.  Replaces tzrec FactorizationMachine.forward
 * (tzrec/modules/fm.py:27-42): out[b,:] = 0.5*((sum_f x_f)^2 - sum_f x_f^2), x:[B,F,D]. */
int tzr_fm_fwd(const float* d_x, int64_t x_stride, int F, int D, int64_t B, float* d_out,
               int64_t out_stride, void* stream);
int tzr_fm_bwd(const float* d_x, int64_t x_stride, int F, int D, int64_t B,
               const float* d_grad_out, int64_t grad_out_stride, float* d_grad_x,
               int64_t grad_x_stride, void* stream);

/* ---- evaluation metrics (csrc/eval_metrics.hip) ------------------------------------------------
 * State of the binary metrics the reference builds from `model_config.metrics` (tzrec/models/rank_model.py:264-334,
 * 375-443): torchmetrics' binned AUROC (tzrec/metrics/decay_auc.py:27-60 is the same form), tzrec/metrics/
 * normalized_entropy.py and tzrec/metrics/grouped_auc.py.  Every update is one asynchronous launch on the caller's
 * stream that reads device memory only: it can sit inside a captured evaluation step.  Labels are int64 as Batch
 * carries them; any non-zero label is the positive class.  Entry points added to version 15: no struct or older
 * entry point changes.
 *
 * K14a: tzr_metric_update -- one launch per (tower, eval step) for `auc` and `normalized_entropy` together.
 *   d_thresholds  float[T], ascending (torch.linspace(0, 1, T): the caller's own floats, so that both sides of a
 *                 comparison see the same values), 1 <= T <= TZR_METRIC_MAX_THRESHOLDS
 *   d_hist        uint64[(T + 1) * 2], zeroed by the caller: d_hist[bin * 2 + class] += 1 per sample, where
 *                 bin(p) = the number of thresholds <= p, found by SEARCHING the threshold values (p >= thr[t] <=> bin > t
 *                 for every float; a NaN falls into bin 0).  Counted per workgroup in LDS, flushed with 64-bit atomic adds:
 *                 integers, so the result does not depend on the order.  null: no histogram (T and d_thresholds not read).
 *   d_ne          double[3] = {sum of cross-entropy, samples, sum of labels}, zeroed by the caller.  The cross-entropy
 *                 of a sample is torch's F.binary_cross_entropy: -(y max(log p, -100) + (1 - y) max(log(1 - p), -100));
 *                 summed wave -> workgroup in double, one double atomic add per workgroup and word.  null: skipped.
 * B < 0, or both states null, or a null input with B > 0: TZR_ERR_INVALID; T > TZR_METRIC_MAX_THRESHOLDS (what one
 * workgroup's LDS histogram holds): TZR_ERR_UNSUPPORTED; B == 0: TZR_OK, nothing launched. */
#define TZR_METRIC_MAX_THRESHOLDS 4096
int tzr_metric_update(const float* d_probs, const int64_t* d_labels, int64_t B, const float* d_thresholds, int T,
                      uint64_t* d_hist, double* d_ne, void* stream);

/* K14b: grouped AUC, rows kept on the device.  tzr_grouped_auc_append writes row i of the batch to position
 * cursor + i of the caller's buffers (struct of arrays, `capacity` rows each: prob float, label int32 0/1, key int64)
 * and advances the cursor by the rows written -- the cursor lives in DEVICE memory, so a captured launch appends behind
 * the previous replay's rows.  d_state: int64[4], zeroed by the caller = {cursor, overflow, arrivals, -}: rows that do
 * not fit are not written and counted in `overflow`; `arrivals` is the launch's own workgroup counter (0 between
 * launches).  B == 0: TZR_OK, nothing launched. */
int tzr_grouped_auc_append(const float* d_probs, const int64_t* d_labels, const int64_t* d_keys, int64_t B,
                           float* d_row_probs, int32_t* d_row_labels, int64_t* d_row_keys, int64_t capacity,
                           int64_t* d_state, void* stream);

/* tzr_grouped_auc_reduce: n rows SORTED by (key, prob) ascending (two stable sorts on the caller's side; no NaN) ->
 * *d_auc_sum = the sum over the groups that hold both classes (grouped_auc.py:113-116) of the group's exact, tie-aware
 * AUC, *d_groups = their number.  Per group the Mann-Whitney count with ties at one half is carried as the integer
 * 2U = sum over positive rows of (2 negatives below + negatives tied) in int64 and divided once, in double, by
 * 2 P N -- the value the exact ROC trapezoid has.  One row per lane; group and tie-run boundaries by binary search
 * in the sorted rows, label counts by prefix sums: a group of any size costs its rows nothing extra.  Sums in a fixed
 * order: the same rows give the same bits.  d_ws: tzr_grouped_auc_reduce_workspace(n) bytes, 256-byte aligned.
 * n == 0 writes zeros. */
size_t tzr_grouped_auc_reduce_workspace(int64_t n);
int tzr_grouped_auc_reduce(const int64_t* d_keys, const float* d_probs, const int32_t* d_labels, int64_t n,
                           double* d_auc_sum, int64_t* d_groups, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TZREC_HIP_H_ */
