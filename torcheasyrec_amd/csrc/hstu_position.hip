// HSTU's positional and timestamp encoder (tzrec/ops/position.py: add_positional_embeddings, add_timestamp_positional_embeddings
// under tzrec/modules/gr/positional_encoder.py) on the jagged rows where they lie, fp32 and bf16; the rule is restated in
// include/tzrec_hip.h.  The reference pads the timestamps to [B, N], gathers two [B, N, E] tensors and scatters L gradient rows
// into two small tables; here a row's table rows are two integers computed once, and the table gradients are fixed-order sums.
//
// Forward, one launch: a workgroup owns HP_SLAB consecutive rows.  Its first wave finds each row's sample by bisection of the
// (clamped) offsets and computes idx and bucket; then all four waves stream x and the two table rows in 16-byte pieces.  The
// bucket goes to memory as int32 for the backward (4 bytes a row beside 4 E).
//
// Backward, dx = alpha g and two table gradients:
//   (1) row pass, a workgroup a slab.  Wave 0 ranks the slab's rows by (bucket, row) -- 64 x 64 compares in LDS, a stable
//       order -- and a ballot over the sorted keys numbers the distinct buckets.  The workgroup's column groups (a group: the
//       E / 4 or E / 8 threads that hold one row in 16-byte pieces) take the distinct buckets in turn: a group walks its bucket's
//       rows in row order, stores dx and keeps the sum; one fp32 partial row a distinct bucket and the slab's sorted keys go to
//       the workspace.  Every row of g is read once here.  The same pass leaves one partial per HOT position row and slab: the
//       rows of the position table that whole runs of every sample land on (timestamp mode: c, every target, and P - 1, the
//       clamped head; positional mode: P - 1) are known on the host, so their sums are split over the slabs here instead of
//       walking all their rows in one workgroup.
//   (2) position gather, a workgroup a table row j that is not hot.  The index rule inverted for sample b gives the rows with
//       idx == j: one row, or in positional mode the run behind high.  The column groups split the samples; their sums meet in
//       LDS and are added in group order.  A row nobody maps to is written as zero.
//   (3) the hot rows: the slabs' partials in the interleaved order of parts_sum.h.
//   (4) timestamp table, a workgroup a bucket: 256 slabs at a time, a thread bisects one slab's keys for the bucket; then the
//       column groups add the hits' partials, group gi the slabs gi, gi + groups, .. of the 256 in order; the groups' sums are
//       added in group order.  A bucket takes at most one row a slab: bucket 0 with every target costs ceil(L / 64) adds.
// No atomics on floats: every sum's order is a function of the shapes and the integer inputs alone.
#include "parts_sum.h"
#include "tzr_bf16.h"
#include "tzr_common.h"

#define HP_THREADS 256
#define HP_SLAB TZR_HSTU_POS_SLAB
#define HP_NOKEY 0x7fffffff  // the key of a row without a bucket: sorts behind every bucket

static_assert(sizeof(TzrHstuPos) == 216, "TzrHstuPos: the layout _lib.py mirrors");
static_assert(HP_SLAB == TZR_WAVE, "one wave ranks a slab: a lane a row");

struct HpArgs {
  const void *x, *g, *pos, *ts;
  void *out, *dx, *dpos, *dts;
  int64_t xs, os, gs, dxs;  // elements between rows
  const int64_t *off, *nt, *tm, *qt;
  int32_t* bucket;
  int32_t* ukeys;  // [S][HP_SLAB]: a slab's distinct buckets, ascending, HP_NOKEY behind them
  float* parts;    // [S][HP_SLAB][E]: a slab's partial of its s-th distinct bucket
  float* hot;      // [nhot][S][E]
  int64_t L;
  int B, E, P, T, max_len, c, use_time, inter, fn, S, nhot, hot_row[2];
  float alpha, incr;
};

// ---- 16 bytes of a row: four fp32 or eight bf16, as floats ---------------------------------------------------------------
template <bool BF>
__device__ __forceinline__ void hp_ld(const void* base, int64_t e, float* v) {
  if constexpr (BF) {
    const tzr_u32x4 u = tzr_ld16(static_cast<const uint16_t*>(base) + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[2 * k] = tzr_bf16_widen((uint16_t)(u[k] & 0xffffu)), v[2 * k + 1] = tzr_bf16_widen((uint16_t)(u[k] >> 16));
  } else {
    const float4 t = tzr_ld4(static_cast<const float*>(base) + e);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
}
template <bool BF>
__device__ __forceinline__ void hp_st(void* base, int64_t e, const float* v) {  // the one rounding of a bf16 output
  if constexpr (BF)
    tzr_st16(static_cast<uint16_t*>(base) + e, tzr_pack_bf16x8(tzr_f32x4{v[0], v[1], v[2], v[3]}, tzr_f32x4{v[4], v[5], v[6], v[7]}));
  else
    tzr_st4(static_cast<float*>(base) + e, make_float4(v[0], v[1], v[2], v[3]));
}
// four fp32 sums to a table's gradient row
template <bool BF>
__device__ __forceinline__ void hp_st_sum4(void* base, int64_t e, float4 v) {
  if constexpr (BF) {
    uint2 u;
    u.x = (uint32_t)tzr_bf16_rne(v.x) | ((uint32_t)tzr_bf16_rne(v.y) << 16);
    u.y = (uint32_t)tzr_bf16_rne(v.z) | ((uint32_t)tzr_bf16_rne(v.w) << 16);
    *reinterpret_cast<uint2*>(static_cast<uint16_t*>(base) + e) = u;
  } else {
    tzr_st4(static_cast<float*>(base) + e, v);
  }
}

// ---- the index rule ------------------------------------------------------------------------------------------------------
struct HpSample {
  int64_t start, n, high;  // first row, rows, and high of the rule (positional: already capped at P - 1)
};

__device__ __forceinline__ HpSample hp_sample(const HpArgs& A, int b) {
  HpSample S;
  tzr_jagged_span(A.off, b, b + 1, A.L, &S.start, &S.n);
  int64_t t = A.nt ? A.nt[b] : 0;
  const int64_t lim = 1ll << 40;  // (the arithmetic below stays far inside int64)
  t = t < -lim ? -lim : (t > lim ? lim : t);
  S.high = S.n - (A.inter ? 2 * t : t);
  if (!A.use_time && S.high > A.P - 1) S.high = A.P - 1;
  return S;
}

// the position-table row of position i of the sample
__device__ __forceinline__ int hp_index(const HpArgs& A, const HpSample& S, int64_t i) {
  if (!A.use_time) {
    const int64_t v = i < S.high ? i : S.high;
    return (int)(v < 0 ? 0 : v);
  }
  if (i < A.c) return (int)i;  // (c <= P)
  const int64_t d = S.high - i, v = A.c + (d > 0 ? d : 0);
  return (int)(v < A.P - 1 ? v : A.P - 1);
}

// the positions [i0, i1) of the sample with hp_index == j, for a j that is NOT hot (the hot rows go through the row pass)
__device__ __forceinline__ void hp_run(const HpArgs& A, const HpSample& S, int j, int64_t* i0, int64_t* i1) {
  const int64_t np = S.n < A.max_len ? S.n : A.max_len;  // the rows the sample keeps
  int64_t a, e;
  if (!A.use_time) {
    const int64_t h0 = S.high < 0 ? 0 : S.high;
    a = j <= h0 ? j : np;
    e = j == h0 ? np : a + 1;  // the run behind high, or the one row in front of it
  } else if (j < A.c) {
    a = j, e = a + 1;
  } else {  // c < j < P - 1: the row high - (j - c), when it is behind the contextual prefix
    a = S.high - (j - A.c);
    e = a + 1;
    if (a < A.c) a = e = np;
  }
  *i0 = a < np ? a : np;
  *i1 = e < np ? e : np;
}

// the sample of row r by bisection of the clamped offsets, -1 for a row no sample owns
__device__ __forceinline__ int hp_locate(const HpArgs& A, int64_t r) {
  if (A.B == 0) return -1;
  auto at = [&](int b) {
    const int64_t v = A.off[b];
    return v < 0 ? 0 : (v > A.L ? A.L : v);
  };
  if (r < at(0) || r >= at(A.B)) return -1;
  int lo = 0, hi = A.B;  // at(lo) <= r < at(hi)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (at(mid) <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// a row's idx, -1 for a row that gets alpha x alone; *b_out, *S_out: its sample
__device__ __forceinline__ int hp_row_index(const HpArgs& A, int64_t r, int* b_out, HpSample* S_out) {
  const int b = hp_locate(A, r);
  if (b < 0) return -1;
  const HpSample S = hp_sample(A, b);
  const int64_t i = r - S.start;
  if (i < 0 || i >= S.n || i >= A.max_len) return -1;  // (offsets that are not ascending: no owner)
  *b_out = b, *S_out = S;
  return hp_index(A, S, i);
}

// the time bucket of a gap, fp32 as the reference computes it: the division and the square root are correctly rounded
__device__ __forceinline__ int hp_bucket(const HpArgs& A, int64_t gap) {
  float u = fmaxf((float)gap, 1e-6f) / A.incr;
  u = A.fn ? logf(u) : __fsqrt_rn(u);
  const float T = (float)A.T;  // (exact: T <= 2^24)
  const float f = fminf(fmaxf(u / T, 0.f), 1.f) * T;
  return (int)f;
}

// ---- forward -------------------------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(HP_THREADS) void tzr_hstu_pos_fwd_kernel(HpArgs A) {
  constexpr int NC = BF ? 8 : 4;
  __shared__ int s_idx[HP_SLAB], s_bkt[HP_SLAB];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * HP_SLAB;
  if (tid < HP_SLAB) {
    const int64_t r = r0 + tid;
    int idx = -1, bk = -1;
    if (r < A.L) {
      int b = 0;
      HpSample S;
      idx = hp_row_index(A, r, &b, &S);
      if (idx >= 0 && A.use_time) {
        const int64_t qt = A.qt ? A.qt[b] : A.tm[S.start + S.n - 1];
        bk = hp_bucket(A, (int64_t)((uint64_t)qt - (uint64_t)A.tm[r]));
      }
      if (A.use_time) A.bucket[r] = bk;
    }
    s_idx[tid] = idx, s_bkt[tid] = bk;
  }
  __syncthreads();
  const int nq = A.E / NC;
  int64_t rows = A.L - r0;
  rows = rows < HP_SLAB ? rows : HP_SLAB;
  for (int e = tid; e < (int)rows * nq; e += HP_THREADS) {
    const int row = e / nq, col = NC * (e - row * nq);
    float xv[NC], pv[NC], tv[NC], o[NC];
    hp_ld<BF>(A.x, (r0 + row) * A.xs + col, xv);
    const int idx = s_idx[row], bk = s_bkt[row];
#pragma unroll
    for (int k = 0; k < NC; ++k) pv[k] = tv[k] = 0.f;
    if (idx >= 0) hp_ld<BF>(A.pos, (int64_t)idx * A.E + col, pv);
    if (bk >= 0) hp_ld<BF>(A.ts, (int64_t)bk * A.E + col, tv);
#pragma unroll
    for (int k = 0; k < NC; ++k) o[k] = fmaf(A.alpha, xv[k], pv[k] + tv[k]);
    hp_st<BF>(A.out, (r0 + row) * A.os + col, o);
  }
}

// ---- backward (1): the row pass ------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(HP_THREADS) void tzr_hstu_pos_rows_kernel(HpArgs A) {
  constexpr int NC = BF ? 8 : 4;
  __shared__ int s_key[HP_SLAB], s_idx[HP_SLAB], s_skey[HP_SLAB], s_srow[HP_SLAB], s_start[HP_SLAB + 1], s_nslot;
  const int tid = threadIdx.x, slab = blockIdx.x;
  const int64_t r0 = (int64_t)slab * HP_SLAB;
  int key = HP_NOKEY;
  if (tid < HP_SLAB) {
    const int64_t r = r0 + tid;
    int idx = -1;
    if (r < A.L) {
      int b = 0;
      HpSample S;
      idx = hp_row_index(A, r, &b, &S);
      if (idx >= 0 && A.use_time) {
        const int bk = A.bucket[r];
        key = bk >= 0 && bk <= A.T ? bk : HP_NOKEY;  // (whatever the array holds, no access leaves the table)
      }
    }
    s_key[tid] = key, s_idx[tid] = idx;
  }
  __syncthreads();
  if (tid < HP_SLAB) {  // stable rank by (key, row); rows at or behind L hold HP_NOKEY and the largest row numbers: they sort last
    int rank = 0;
    for (int j = 0; j < HP_SLAB; ++j) rank += (s_key[j] < key || (s_key[j] == key && j < tid)) ? 1 : 0;
    s_skey[rank] = key, s_srow[rank] = tid;
  }
  __syncthreads();
  const bool head = tid < HP_SLAB && (tid == 0 || s_skey[tid] != s_skey[tid - 1]);
  const unsigned long long heads = __ballot(head);  // (wave 0's is the slab's)
  if (tid < HP_SLAB) {
    const int nslot = __popcll(heads);
    if (head) {
      const int slot = __popcll(heads & ((2ull << tid) - 1ull)) - 1;
      s_start[slot] = tid;
      if (A.use_time) A.ukeys[(int64_t)slab * HP_SLAB + slot] = s_skey[tid];
    }
    if (A.use_time && tid >= nslot) A.ukeys[(int64_t)slab * HP_SLAB + tid] = HP_NOKEY;  // (positional mode has no key list)
    if (tid == 0) s_start[nslot] = HP_SLAB, s_nslot = nslot;
  }
  __syncthreads();
  const int nq = A.E / NC, groups = HP_THREADS / nq, gi = tid / nq, col = NC * (tid - gi * nq);
  if (gi >= groups) return;
  int64_t rows = A.L - r0;
  rows = rows < HP_SLAB ? rows : HP_SLAB;
  for (int slot = gi; slot < s_nslot; slot += groups) {  // a distinct bucket: its rows in row order
    float acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.f;
    for (int p = s_start[slot]; p < s_start[slot + 1]; ++p) {
      const int row = s_srow[p];
      if (row >= rows) continue;
      float gv[NC], d[NC];
      hp_ld<BF>(A.g, (r0 + row) * A.gs + col, gv);
#pragma unroll
      for (int k = 0; k < NC; ++k) d[k] = A.alpha * gv[k], acc[k] += gv[k];
      hp_st<BF>(A.dx, (r0 + row) * A.dxs + col, d);
    }
    if (s_skey[s_start[slot]] != HP_NOKEY) {
      float* dst = A.parts + ((int64_t)slab * HP_SLAB + slot) * A.E + col;
      tzr_st4(dst, make_float4(acc[0], acc[1], acc[2], acc[3]));
      if constexpr (BF) tzr_st4(dst + 4, make_float4(acc[4], acc[5], acc[6], acc[7]));
    }
  }
  for (int h = gi; h < A.nhot; h += groups) {  // a hot position row: the slab's rows on it, in row order
    float acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.f;
    for (int row = 0; row < (int)rows; ++row) {
      if (s_idx[row] != A.hot_row[h]) continue;
      float gv[NC];
      hp_ld<BF>(A.g, (r0 + row) * A.gs + col, gv);
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] += gv[k];
    }
    float* dst = A.hot + ((int64_t)h * A.S + slab) * A.E + col;
    tzr_st4(dst, make_float4(acc[0], acc[1], acc[2], acc[3]));
    if constexpr (BF) tzr_st4(dst + 4, make_float4(acc[4], acc[5], acc[6], acc[7]));
  }
}

// the groups' sums of one table row, through LDS, added in group order; NC floats a thread, `red` [groups][E]
template <int NC>
__device__ __forceinline__ void hp_join_groups(const float* acc, float* red, int E, int nq, int groups, int gi, int col, float* sum) {
  if (gi < groups) {
#pragma unroll
    for (int k = 0; k < NC; ++k) red[gi * E + col + k] = acc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NC; ++k) sum[k] = 0.f;
  if (gi == 0)
    for (int s = 0; s < groups; ++s)
#pragma unroll
      for (int k = 0; k < NC; ++k) sum[k] += red[s * E + col + k];
}

// ---- backward (2): the position table's rows that are not hot ------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(HP_THREADS) void tzr_hstu_pos_gather_kernel(HpArgs A) {
  constexpr int NC = BF ? 8 : 4;
  __shared__ float red[HP_THREADS * NC];  // groups x E <= 256 NC
  const int tid = threadIdx.x, j = blockIdx.x;
  for (int h = 0; h < A.nhot; ++h)
    if (j == A.hot_row[h]) return;
  const int nq = A.E / NC, groups = HP_THREADS / nq, gi = tid / nq, col = NC * (tid - gi * nq);
  float acc[NC], sum[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.f;
  if (gi < groups) {
    for (int b = gi; b < A.B; b += groups) {
      const HpSample S = hp_sample(A, b);
      int64_t i0, i1;
      hp_run(A, S, j, &i0, &i1);
      for (int64_t i = i0; i < i1; ++i) {
        float gv[NC];
        hp_ld<BF>(A.g, (S.start + i) * A.gs + col, gv);
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[k] += gv[k];
      }
    }
  }
  hp_join_groups<NC>(acc, red, A.E, nq, groups, gi, col, sum);
  if (gi == 0) hp_st<BF>(A.dpos, (int64_t)j * A.E + col, sum);
}

// ---- backward (3): the hot rows, the slabs' partials in parts_sum.h's interleaved order ----------------------------------
template <bool BF>
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_hstu_pos_hot_kernel(HpArgs A) {
  __shared__ float red[TZR_FIN_THREADS];
  const int h = blockIdx.y, col = blockIdx.x * TZR_WAVE + (threadIdx.x & (TZR_WAVE - 1));
  const float r = tzr_parts_sum_interleaved(col < A.E ? A.hot + (size_t)h * A.S * A.E + col : nullptr, A.S, (size_t)A.E, red);
  if (threadIdx.x >= TZR_WAVE || col >= A.E) return;
  const int64_t e = (int64_t)A.hot_row[h] * A.E + col;
  if constexpr (BF) static_cast<uint16_t*>(A.dpos)[e] = tzr_bf16_rne(r);
  else static_cast<float*>(A.dpos)[e] = r;
}

// ---- backward (4): the timestamp table, a workgroup a bucket --------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(HP_THREADS) void tzr_hstu_pos_buckets_kernel(HpArgs A) {
  __shared__ int s_hit[HP_THREADS];
  __shared__ float red[HP_THREADS * 4];
  const int tid = threadIdx.x, bk = blockIdx.x;
  const int nq = A.E / 4, groups = HP_THREADS / nq, gi = tid / nq, col = 4 * (tid - gi * nq);  // (the partials are fp32 for both dtypes)
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, sum[4];
  for (int s0 = 0; s0 < A.S; s0 += HP_THREADS) {
    int hit = -1;
    if (s0 + tid < A.S) {  // the first key >= bk among the slab's ascending keys
      const int32_t* keys = A.ukeys + (int64_t)(s0 + tid) * HP_SLAB;
      int lo = 0, hi = HP_SLAB;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < bk) lo = mid + 1; else hi = mid;
      }
      if (lo < HP_SLAB && keys[lo] == bk) hit = lo;
    }
    s_hit[tid] = hit;
    __syncthreads();
    if (gi < groups) {
      const int cnt = A.S - s0 < HP_THREADS ? A.S - s0 : HP_THREADS;
      for (int t = gi; t < cnt; t += groups) {
        const int slot = s_hit[t];
        if (slot < 0) continue;
        const float4 v = tzr_ld4(A.parts + ((int64_t)(s0 + t) * HP_SLAB + slot) * A.E + col);
        acc[0] += v.x, acc[1] += v.y, acc[2] += v.z, acc[3] += v.w;
      }
    }
    __syncthreads();
  }
  hp_join_groups<4>(acc, red, A.E, nq, groups, gi, col, sum);
  if (gi == 0) hp_st_sum4<BF>(A.dts, (int64_t)bk * A.E + col, make_float4(sum[0], sum[1], sum[2], sum[3]));
}

// ---- host ----------------------------------------------------------------------------------------------------------------

// sizes, then limits; `A` gets the shape and the hot rows
static int hp_shape(const TzrHstuPos* m, HpArgs* A) {
  if (m->L < 0 || m->B < 0 || m->contextual_seq_len < 0) return TZR_ERR_INVALID;
  if (m->use_time && (!(m->time_bucket_increments > 0.f) || m->time_fn < 0 || m->time_fn > 1)) return TZR_ERR_INVALID;
  const bool dim_ok = m->bf16 ? tzr_dim8_ok(m->E, TZR_HSTU_POS_MAX_DIM) : tzr_dim4_ok(m->E, TZR_HSTU_POS_MAX_DIM);
  if (!dim_ok || m->P < 1 || m->max_seq_len < 1 || m->max_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->L >= (1ll << 31) || m->B >= (1ll << 31)) return TZR_ERR_UNSUPPORTED;
  if (m->use_time && (m->T < 1 || m->T > TZR_HSTU_POS_MAX_BUCKETS || m->contextual_seq_len > m->P)) return TZR_ERR_UNSUPPORTED;
  A->L = m->L, A->B = (int)m->B, A->E = m->E, A->P = m->P, A->T = m->use_time ? m->T : 0, A->max_len = m->max_seq_len;
  A->c = m->use_time ? m->contextual_seq_len : 0, A->use_time = m->use_time != 0, A->inter = m->interleave_targets != 0, A->fn = m->time_fn;
  A->alpha = m->alpha, A->incr = m->time_bucket_increments;
  A->S = (int)((m->L + HP_SLAB - 1) / HP_SLAB);
  A->nhot = 0;
  A->hot_row[0] = A->hot_row[1] = -1;
  if (A->use_time && A->c < A->P - 1) A->hot_row[A->nhot++] = A->c;
  A->hot_row[A->nhot++] = A->P - 1;
  return TZR_OK;
}

// a row operand [L, E]: 16-byte aligned, rows a multiple of 16 bytes and at least E elements apart
static int hp_rows(uint64_t ptr, int64_t stride, const TzrHstuPos* m) {
  if (!ptr || (ptr & 15)) return TZR_ERR_INVALID;
  return ((stride & (m->bf16 ? 7 : 3)) || stride < m->E) ? TZR_ERR_UNSUPPORTED : TZR_OK;
}

static bool hp_bad(uint64_t ptr, uint64_t mask, bool nullable = false) { return (!ptr && !nullable) || (ptr & mask); }

// offsets, num_targets and the tables' pointers, shared by both directions
static int hp_common(const TzrHstuPos* m, HpArgs* A) {
  if (m->B > 0 && hp_bad(m->offsets, 7)) return TZR_ERR_INVALID;
  if (hp_bad(m->num_targets, 7, true)) return TZR_ERR_INVALID;
  A->off = reinterpret_cast<const int64_t*>(m->offsets);
  A->nt = m->B > 0 ? reinterpret_cast<const int64_t*>(m->num_targets) : nullptr;
  A->bucket = reinterpret_cast<int32_t*>(m->bucket);
  if (A->use_time && m->L > 0 && hp_bad(m->bucket, 3)) return TZR_ERR_INVALID;
  return TZR_OK;
}

struct HpWs {
  size_t ukeys, parts, hot, total;
};
static HpWs hp_ws(const HpArgs& A) {
  HpWs w;
  w.ukeys = 0;
  w.parts = tzr_align_up(A.use_time ? (size_t)A.S * HP_SLAB * sizeof(int32_t) : 0);
  w.hot = w.parts + tzr_align_up(A.use_time ? (size_t)A.S * HP_SLAB * A.E * sizeof(float) : 0);
  w.total = w.hot + tzr_align_up((size_t)A.nhot * A.S * A.E * sizeof(float));
  return w;
}

extern "C" size_t tzr_hstu_pos_bwd_workspace(const TzrHstuPos* h_po) {
  HpArgs A = {};
  if (!h_po || hp_shape(h_po, &A) != TZR_OK) return 0;
  return hp_ws(A).total;
}

extern "C" int tzr_hstu_pos_fwd(const TzrHstuPos* h_po, void* stream) {
  if (!h_po) return TZR_ERR_INVALID;
  HpArgs A = {};
  TZR_TRY(hp_shape(h_po, &A));
  if (h_po->L == 0) return TZR_OK;
  TZR_TRY(hp_rows(h_po->x, h_po->x_stride, h_po));
  TZR_TRY(hp_rows(h_po->out, h_po->out_stride, h_po));
  if (hp_bad(h_po->pos, 15) || (A.use_time && (hp_bad(h_po->ts, 15) || hp_bad(h_po->timestamps, 7) || hp_bad(h_po->query_time, 7, true)))) return TZR_ERR_INVALID;
  TZR_TRY(hp_common(h_po, &A));
  A.x = reinterpret_cast<const void*>(h_po->x), A.xs = h_po->x_stride, A.out = reinterpret_cast<void*>(h_po->out), A.os = h_po->out_stride;
  A.pos = reinterpret_cast<const void*>(h_po->pos), A.ts = reinterpret_cast<const void*>(h_po->ts);
  A.tm = reinterpret_cast<const int64_t*>(h_po->timestamps);
  A.qt = h_po->B > 0 ? reinterpret_cast<const int64_t*>(h_po->query_time) : nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h_po->bf16) hipLaunchKernelGGL((tzr_hstu_pos_fwd_kernel<true>), dim3((unsigned)A.S), dim3(HP_THREADS), 0, s, A);
  else hipLaunchKernelGGL((tzr_hstu_pos_fwd_kernel<false>), dim3((unsigned)A.S), dim3(HP_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

template <bool BF>
static int hp_bwd_launch(const HpArgs& A, hipStream_t s) {
  if (A.S > 0) {
    hipLaunchKernelGGL((tzr_hstu_pos_rows_kernel<BF>), dim3((unsigned)A.S), dim3(HP_THREADS), 0, s, A);
    TZR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL((tzr_hstu_pos_gather_kernel<BF>), dim3((unsigned)A.P), dim3(HP_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL((tzr_hstu_pos_hot_kernel<BF>), dim3((unsigned)((A.E + TZR_WAVE - 1) / TZR_WAVE), (unsigned)A.nhot), dim3(TZR_FIN_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  if (A.use_time) {
    hipLaunchKernelGGL((tzr_hstu_pos_buckets_kernel<BF>), dim3((unsigned)(A.T + 1)), dim3(HP_THREADS), 0, s, A);
    TZR_CHECK_LAUNCH();
  }
  return TZR_OK;
}

extern "C" int tzr_hstu_pos_bwd(const TzrHstuPos* h_po, void* stream) {
  if (!h_po) return TZR_ERR_INVALID;
  HpArgs A = {};
  TZR_TRY(hp_shape(h_po, &A));
  if (h_po->L > 0) {
    TZR_TRY(hp_rows(h_po->grad_out, h_po->grad_out_stride, h_po));
    TZR_TRY(hp_rows(h_po->dx, h_po->dx_stride, h_po));
  }
  if (hp_bad(h_po->dpos, 15) || (A.use_time && hp_bad(h_po->dts, 15))) return TZR_ERR_INVALID;
  TZR_TRY(hp_common(h_po, &A));
  const HpWs w = hp_ws(A);
  if (w.total > 0 && (!h_po->ws || (h_po->ws & 255) || h_po->ws_bytes < w.total)) return TZR_ERR_WORKSPACE;
  A.g = reinterpret_cast<const void*>(h_po->grad_out), A.gs = h_po->grad_out_stride, A.dx = reinterpret_cast<void*>(h_po->dx), A.dxs = h_po->dx_stride;
  A.dpos = reinterpret_cast<void*>(h_po->dpos), A.dts = reinterpret_cast<void*>(h_po->dts);
  char* base = reinterpret_cast<char*>(h_po->ws);
  A.ukeys = reinterpret_cast<int32_t*>(base + w.ukeys), A.parts = reinterpret_cast<float*>(base + w.parts), A.hot = reinterpret_cast<float*>(base + w.hot);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return h_po->bf16 ? hp_bwd_launch<true>(A, s) : hp_bwd_launch<false>(A, s);
}
