// HSTU's delta attention (tzrec/ops/hstu_attention.py::delta_hstu_mha, the op under STULayer.cached_forward), forward only, fp32:
// the last `delta` rows of every sample as queries against the sample's whole key / value sequence,
//   out[b delta + r, h, :] = sum_j valid(i, j) silu(alpha <dq[b delta + r, h], k_b[j, h]>) / scale v_b[j, h, :],   i = n_b - delta + r
// with the mask of hstu_attention.hip (the index rule of include/tzrec_hip.h) on the n_b rows of the full sequence.  A serving
// step has 1 .. 32 query rows a sample against thousands of keys: the forward of hstu_attention.hip would give it B x H workgroups
// with three of four waves idle and one serial walk each.  There is no softmax, so partial sums over disjoint key ranges simply
// add: here the KEYS are split, across the waves of a workgroup and across workgroups.
//
// Keys and values come from two segments read where they lie: the cached rows (jagged by the offsets) and, behind them, the dense
// delta rows (sample b: rows b delta ..); hd_row picks the segment per key row, nothing is concatenated.  Without the delta
// segment k / v hold the full sequences (the reference's form): the same code with the second segment null.
//
// Grid chunks x ceil(delta / 16) x B x H, 256 threads.  A workgroup owns (sample, head, 16 delta rows, HD_CHUNK keys).  The Q tile
// is in registers as the B operand fragments of v_mfma_f32_16x16x4_f32 (lane (li, g): the float4s at columns 16 ch + 4 g of query
// li).  Wave w takes the 16-key tiles w, w + 4, .. of the chunk -- no two waves share a tile, so K and V go global -> registers and
// LDS caches no tile.  The score tile is computed TRANSPOSED, S^T = K Q^T (lane (li, g) loads the float4s of KEY li): accumulator
// register e of lane (li, g) is (key 4 g + e, query li), and after mask, SiLU and scale it is the A operand of P V for contraction
// step e when that step takes V's row 4 g + e as its B operand.  V's rows are read as float4s too: lane li takes the columns 64 cg
// + 4 li .. + 3 and feeds component x, y, z, w to the accumulators 4 cg + 0 .. 3 -- the output columns are permuted among the
// accumulators, which the store undoes for free (register r of accumulator 4 cg + m is (query 4 g + r, column 64 cg + 4 li + m):
// one float4 a row).  Each wave's 16 x Dv partial goes to LDS once; the four are added in wave order 0 .. 3.  With one chunk the
// workgroup stores `out`; with more it stores its partial into ws[chunk][B delta][H][Dv] and tzr_hstu_delta_finish_kernel adds the
// chunks a sample has (ceil(n / HD_CHUNK): a workgroup whose chunk starts at or behind n exits, its slot is never read) in order
// 0, 1, ..  No atomics: two runs are bit-equal, and so are the two forms on the same rows.
//
// Key tiles with no valid pair are skipped by hd_row_walk (hs_row_walk of hstu_attention.hip for the tile's rows): keys in front
// of the window, target keys in front of the rows' own.  A superset: validity is the per-element rule.  A sample with n >
// max_seq_len or n < delta gets zeros (the caller's duty, made memory-safe): no key row of it is read.
#include "tzr_common.h"

#define HD_THREADS 256
#define HD_TILE 16
#define HD_CHUNK TZR_HSTU_DELTA_CHUNK
#define HD_CT (HD_CHUNK / HD_TILE)  // tiles a chunk

static_assert(sizeof(TzrHstuDelta) == 232, "TzrHstuDelta: the layout _lib.py mirrors");
static_assert(HD_CHUNK % (4 * HD_TILE) == 0, "a chunk is whole tiles, the same number for each of the four waves");

struct HdOperand {
  float* p;
  int64_t rs, hs;  // floats between rows / between heads
};

struct HdArgs {
  HdOperand q, k, v, kd, vd, out;  // kd.p null: one segment
  const int64_t* off;
  const int64_t* nt;  // nullable
  float* ws;
  int64_t Nc;
  int B, H, Da, Dv, delta, max_len, L, c, ntile, nchunk;
  float alpha, inv_scale;
};

// The mask helpers of hstu_attention.hip, restated on this file's argument struct (as hstu_attention_bf16.hip does).
struct HdSample {
  int64_t start;
  int n, n1, max_id, nts, has_t;  // n1: cached rows (n in the one-segment form); nts: keys at or behind it are targets
  bool ok;                        // delta <= n <= max_seq_len
};

// the rows of sample b: first cached row, cached rows, and n (-1: refused)
__device__ __forceinline__ int hd_rows(const HdArgs& A, int b, int64_t* start, int64_t* len) {
  tzr_jagged_span(A.off, b, b + 1, A.Nc, start, len);
  const int64_t n = *len + (A.kd.p ? A.delta : 0);
  return n <= (int64_t)A.max_len && n >= (int64_t)A.delta ? (int)n : -1;
}

__device__ __forceinline__ HdSample hd_sample(const HdArgs& A, int b) {
  HdSample S;
  int64_t len;
  const int n = hd_rows(A, b, &S.start, &len);
  S.ok = n >= 0;
  S.n = S.ok ? n : 0;
  S.n1 = A.kd.p && S.ok ? (int)len : S.n;
  int64_t t = A.nt ? A.nt[b] : 0;
  t = t < -(int64_t)TZR_HSTU_MAX_SEQ_LEN ? -(int64_t)TZR_HSTU_MAX_SEQ_LEN : (t > TZR_HSTU_MAX_SEQ_LEN ? TZR_HSTU_MAX_SEQ_LEN : t);  // (int arithmetic below)
  S.has_t = A.nt != nullptr;
  S.max_id = (A.c > 0 ? S.n - A.c + 1 : S.n) - (int)t;
  const int nts = S.n - (int)t;
  S.nts = nts < 0 ? 0 : (nts > S.n ? S.n : nts);
  return S;
}

__device__ __forceinline__ int hd_id(const HdArgs& A, const HdSample& S, int i) {
  int v = i;
  if (A.c > 0) v = i - A.c + 1 > 0 ? i - A.c + 1 : 0;
  if (S.has_t) v = v < S.max_id ? v : S.max_id;
  return v;
}

// the index rule, row i with id ii against key j with id jj
__device__ __forceinline__ bool hd_valid(const HdArgs& A, const HdSample& S, int i, int ii, int j, int jj) {
  const int d = ii - jj;
  bool ok = i == j || d > 0;
  if (A.L > 0) ok = ok && d <= A.L;
  if (A.c > 0) ok = ok || (ii == 0 && jj < S.max_id);
  return ok && i < S.n && j < S.n;
}

// the key tiles of the query rows [r0, r1): two runs, [a0, a1) and [b0, b1)
struct HdWalk {
  int a0, a1, b0, b1;
};

__device__ __forceinline__ HdWalk hd_row_walk(const HdArgs& A, const HdSample& S, int r0, int r1) {
  HdWalk W;
  const bool ctx = A.c > 0 && r0 < A.c && S.max_id > 0;  // a contextual row walks every non-target key
  const int hi = ctx ? (r1 > S.nts ? r1 : S.nts) : r1;
  int lo = 0;
  if (A.L > 0 && !ctx) {  // the first key whose id reaches id(r0) - L
    const int target = hd_id(A, S, r0) - A.L;
    lo = target <= 0 ? 0 : target + (A.c > 0 ? A.c - 1 : 0);
  }
  const int hit = (hi + HD_TILE - 1) / HD_TILE;
  W.a0 = lo / HD_TILE;
  int a1 = hit;
  if (S.has_t) {  // tiles of targets alone in front of the rows' own: nothing valid
    a1 = (S.nts + HD_TILE - 1) / HD_TILE;
    a1 = a1 < W.a0 ? W.a0 : (a1 > hit ? hit : a1);
  }
  int b0 = r0 / HD_TILE;
  b0 = b0 < a1 ? a1 : (b0 > hit ? hit : b0);
  W.a1 = a1, W.b0 = b0, W.b1 = hit;
  return W;
}

// key row j (< n) of head h: a cached row or, behind them, a delta row
__device__ __forceinline__ const float* hd_row(const HdOperand& c, const HdOperand& d, const HdSample& S, int b, int h, int delta, int j) {
  return j < S.n1 ? c.p + (S.start + j) * c.rs + h * c.hs : d.p + ((int64_t)b * delta + (j - S.n1)) * d.rs + h * d.hs;
}

// one tile of 16 keys from k0 on: o += (masked silu(alpha K Q^T) / scale)^T V
template <int D>
__device__ __forceinline__ void hd_tile(const HdArgs& A, const HdSample& S, int b, int h, int k0, const float4* qf, int i, int ii, tzr_f32x4* o, int li, int g) {
  // K: lane (li, g) holds key k0 + li at the columns 16 ch + 4 g; V: key k0 + 4 g + e at the columns 64 cg + 4 li.  Rows at or
  // behind n are zeros; the loads are unconditional, from a clamped row and column (no branch around them).
  const int jk = k0 + li;
  const float* kp = hd_row(A.k, A.kd, S, b, h, A.delta, jk < S.n ? jk : S.n - 1);
  float4 kf[D / 16], vf[4][D / 64];
#pragma unroll
  for (int ch = 0; ch < D / 16; ++ch) {
    const int a = 16 * ch + 4 * g;
    if (16 * ch < A.Da) {
      const float4 t = tzr_ld4(kp + (a < A.Da ? a : 0));
      kf[ch] = a < A.Da && jk < S.n ? t : tzr_zero4();
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int jv = k0 + 4 * g + e;
    const float* vp = hd_row(A.v, A.vd, S, b, h, A.delta, jv < S.n ? jv : S.n - 1);
#pragma unroll
    for (int cg = 0; cg < D / 64; ++cg) {
      const int col = 64 * cg + 4 * li;
      if (64 * cg < A.Dv) {
        const float4 t = tzr_ld4(vp + (col < A.Dv ? col : 0));
        vf[e][cg] = col < A.Dv && jv < S.n ? t : tzr_zero4();
      }
    }
  }
  tzr_f32x4 acc[4];
  tzr_acc_zero(acc, 4);
#pragma unroll
  for (int ch = 0; ch < D / 16; ++ch)
    if (16 * ch < A.Da) tzr_mfma4(kf[ch], qf[ch], acc);
  const tzr_f32x4 st = tzr_join4(acc);  // (key 4 g + e, query li)
  tzr_f32x4 p;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = k0 + 4 * g + e;
    const float x = A.alpha * st[e];
    p[e] = hd_valid(A, S, i, ii, j, hd_id(A, S, j)) ? x * tzr_sigmoid(x) * A.inv_scale : 0.f;
  }
#pragma unroll
  for (int cg = 0; cg < D / 64; ++cg) {
    if (64 * cg < A.Dv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[4 * cg + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[e], vf[e][cg].x, o[4 * cg + 0], 0, 0, 0);
        o[4 * cg + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[e], vf[e][cg].y, o[4 * cg + 1], 0, 0, 0);
        o[4 * cg + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[e], vf[e][cg].z, o[4 * cg + 2], 0, 0, 0);
        o[4 * cg + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[e], vf[e][cg].w, o[4 * cg + 3], 0, 0, 0);
      }
    }
  }
}

template <int D>
__global__ __launch_bounds__(HD_THREADS) void tzr_hstu_delta_kernel(HdArgs A) {
  __shared__ float Sm[4][16][D + 4];
  const unsigned x = blockIdx.x, bh = (unsigned)A.B * (unsigned)A.H, u = x / bh, bhi = x - u * bh;
  const int b = (int)(bhi / (unsigned)A.H), h = (int)(bhi - (unsigned)b * (unsigned)A.H);
  const int ch = (int)(u / (unsigned)A.ntile), r0 = HD_TILE * (int)(u - (unsigned)ch * (unsigned)A.ntile);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int rows = A.delta - r0 < HD_TILE ? A.delta - r0 : HD_TILE, v4 = A.Dv >> 2;
  const int64_t row0 = (int64_t)b * A.delta + r0;
  // where the tile's 16 x Dv block goes: out, or this chunk's slot of the workspace
  float* dst = A.nchunk == 1 ? A.out.p + row0 * A.out.rs + h * A.out.hs : A.ws + (((int64_t)ch * A.B * A.delta + row0) * A.H + h) * A.Dv;
  const int64_t drs = A.nchunk == 1 ? A.out.rs : (int64_t)A.H * A.Dv;
  const HdSample S = hd_sample(A, b);
  if (!S.ok) {  // zeros: here with one chunk, from the finishing launch otherwise
    if (A.nchunk == 1)
      for (int e = tid; e < rows * v4; e += HD_THREADS) tzr_st4(dst + (e / v4) * drs + 4 * (e % v4), tzr_zero4());
    return;
  }
  if (ch * HD_CHUNK >= S.n) return;  // (never chunk 0: n >= delta >= 1)
  const int rq = r0 + li, i = S.n - A.delta + rq, ii = hd_id(A, S, i);  // (rq >= delta: i >= n, nothing valid)
  const float* qp = rq < A.delta ? A.q.p + (row0 + li) * A.q.rs + h * A.q.hs : nullptr;
  float4 qf[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) {
    const int a = 16 * c + 4 * g;
    qf[c] = qp && a < A.Da ? tzr_ld4(qp + a) : tzr_zero4();
  }
  tzr_f32x4 o[D / 16];
  tzr_acc_zero(o, D / 16);
  const int i0 = S.n - A.delta + r0;
  const HdWalk W = hd_row_walk(A, S, i0, i0 + rows);
  const int c0 = ch * HD_CT, c1 = c0 + HD_CT;
#pragma unroll
  for (int run = 0; run < 2; ++run) {  // the part of each run inside the chunk; wave w its tiles w, w + 4, .. (c0 is a multiple of 4)
    int lo = run ? W.b0 : W.a0, hi = run ? W.b1 : W.a1;
    lo = lo < c0 ? c0 : lo, hi = hi > c1 ? c1 : hi;
    for (int t = lo + ((wv - lo) & 3); t < hi; t += 4) hd_tile<D>(A, S, b, h, t * HD_TILE, qf, i, ii, o, li, g);
  }
  // register r of accumulator 4 cg + m is (query 4 g + r, column 64 cg + 4 li + m)
#pragma unroll
  for (int cg = 0; cg < D / 64; ++cg)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      tzr_st4(&Sm[wv][4 * g + r][64 * cg + 4 * li], make_float4(o[4 * cg][r], o[4 * cg + 1][r], o[4 * cg + 2][r], o[4 * cg + 3][r]));
  __syncthreads();
  for (int e = tid; e < rows * v4; e += HD_THREADS) {  // the four partials in wave order
    const int r = e / v4, c = 4 * (e - r * v4);
    const float4 s = tzr_add4(tzr_add4(tzr_add4(tzr_ld4(&Sm[0][r][c]), tzr_ld4(&Sm[1][r][c])), tzr_ld4(&Sm[2][r][c])), tzr_ld4(&Sm[3][r][c]));
    tzr_st4(dst + r * drs + c, s);
  }
}

// out = the chunks' partials in order 0, 1, .. -- only the chunks the sample has; zeros for a refused sample.  One thread a float4.
__global__ __launch_bounds__(HD_THREADS) void tzr_hstu_delta_finish_kernel(HdArgs A) {
  const int v4 = A.Dv >> 2;
  const int64_t x = (int64_t)blockIdx.x * HD_THREADS + threadIdx.x, rows = (int64_t)A.B * A.delta;
  if (x >= rows * A.H * v4) return;
  const int c = 4 * (int)(x % v4);
  const int64_t rh = x / v4, row = rh / A.H;
  const int h = (int)(rh - row * A.H);
  int64_t start, len;
  const int n = hd_rows(A, (int)(row / A.delta), &start, &len);
  float4 s = tzr_zero4();
  if (n >= 0) {
    const int nch = (n + HD_CHUNK - 1) / HD_CHUNK;  // (>= 1, and <= nchunk: n <= max_seq_len)
    const int64_t slot = rows * A.H * A.Dv;
    const float* p = A.ws + (row * A.H + h) * A.Dv + c;
    s = tzr_ld4(p);
    for (int k = 1; k < nch; ++k) s = tzr_add4(s, tzr_ld4(p + k * slot));
  }
  tzr_st4(A.out.p + row * A.out.rs + h * A.out.hs + c, s);
}

// ---- host ------------------------------------------------------------------------------------------------------------

// an [N, H, D] operand by row and head stride, the rule of hstu_attention.hip
static int hd_operand(uint64_t ptr, int64_t rs, int64_t hs, int H, int D, HdOperand* o) {
  if (!ptr || (ptr & 15)) return TZR_ERR_INVALID;
  if ((rs & 3) || (hs & 3) || hs < D || rs < (int64_t)(H - 1) * hs + D) return TZR_ERR_UNSUPPORTED;
  o->p = reinterpret_cast<float*>(ptr), o->rs = rs, o->hs = hs;
  return TZR_OK;
}

// sizes, then limits; `A` gets the shape
static int hd_shape(const TzrHstuDelta* m, HdArgs* A) {
  if (m->B < 0 || m->Nc < 0 || m->max_attn_len < 0 || m->contextual_seq_len < 0) return TZR_ERR_INVALID;
  if (!tzr_dim4_ok(m->Da, TZR_HSTU_MAX_DIM) || !tzr_dim4_ok(m->Dv, TZR_HSTU_MAX_DIM) || m->H < 1 || m->delta < 1 || m->max_seq_len < 1 ||
      m->max_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->max_attn_len > TZR_HSTU_MAX_SEQ_LEN || m->contextual_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->Nc >= (1ll << 31))
    return TZR_ERR_UNSUPPORTED;
  const int64_t nchunk = ((int64_t)m->max_seq_len + HD_CHUNK - 1) / HD_CHUNK, ntile = ((int64_t)m->delta + HD_TILE - 1) / HD_TILE;
  if (m->B > 0 && (m->B >= (1ll << 31) / m->delta || m->B * m->delta >= (1ll << 31) / m->H || nchunk * ntile >= (1ll << 31) / (m->B * m->H))) return TZR_ERR_UNSUPPORTED;
  A->Nc = m->Nc, A->B = (int)m->B, A->H = m->H, A->Da = m->Da, A->Dv = m->Dv, A->delta = m->delta, A->max_len = m->max_seq_len;
  A->L = m->max_attn_len, A->c = m->contextual_seq_len, A->ntile = (int)ntile, A->nchunk = (int)nchunk;
  A->alpha = m->alpha;
  A->inv_scale = 1.0f / (float)(m->scaling_seqlen > 0 ? m->scaling_seqlen : m->max_seq_len);
  return TZR_OK;
}

static size_t hd_ws_bytes(const HdArgs& A) { return A.nchunk > 1 ? (size_t)A.nchunk * A.B * A.delta * A.H * A.Dv * sizeof(float) : 0; }

// one slot [B delta][H][Dv] a chunk; nothing with one chunk (or a call that would be refused)
extern "C" size_t tzr_hstu_delta_workspace(const TzrHstuDelta* h_dl) {
  HdArgs A = {};
  if (!h_dl || hd_shape(h_dl, &A) != TZR_OK) return 0;
  return hd_ws_bytes(A);
}

extern "C" int tzr_hstu_delta_fwd(const TzrHstuDelta* h_dl, void* stream) {
  if (!h_dl) return TZR_ERR_INVALID;
  HdArgs A = {};
  TZR_TRY(hd_shape(h_dl, &A));
  if (h_dl->B == 0) return TZR_OK;
  TZR_TRY(hd_operand(h_dl->delta_q, h_dl->delta_q_stride, h_dl->delta_q_head_stride, A.H, A.Da, &A.q));
  if (A.Nc > 0) {
    TZR_TRY(hd_operand(h_dl->k, h_dl->k_stride, h_dl->k_head_stride, A.H, A.Da, &A.k));
    TZR_TRY(hd_operand(h_dl->v, h_dl->v_stride, h_dl->v_head_stride, A.H, A.Dv, &A.v));
  }
  if (!h_dl->k_delta != !h_dl->v_delta) return TZR_ERR_INVALID;
  if (h_dl->k_delta) {
    TZR_TRY(hd_operand(h_dl->k_delta, h_dl->k_delta_stride, h_dl->k_delta_head_stride, A.H, A.Da, &A.kd));
    TZR_TRY(hd_operand(h_dl->v_delta, h_dl->v_delta_stride, h_dl->v_delta_head_stride, A.H, A.Dv, &A.vd));
  }
  if (!h_dl->offsets || (h_dl->offsets & 7) || (h_dl->num_targets & 7)) return TZR_ERR_INVALID;
  TZR_TRY(hd_operand(h_dl->out, h_dl->out_stride, h_dl->out_head_stride, A.H, A.Dv, &A.out));
  if (A.nchunk > 1 && (!h_dl->ws || (h_dl->ws & 255) || h_dl->ws_bytes < hd_ws_bytes(A))) return TZR_ERR_WORKSPACE;
  A.off = reinterpret_cast<const int64_t*>(h_dl->offsets);
  A.nt = reinterpret_cast<const int64_t*>(h_dl->num_targets);
  A.ws = reinterpret_cast<float*>(h_dl->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((int64_t)A.nchunk * A.ntile * A.B * A.H));
  if ((A.Da > A.Dv ? A.Da : A.Dv) <= 64) hipLaunchKernelGGL((tzr_hstu_delta_kernel<64>), grid, dim3(HD_THREADS), 0, s, A);
  else hipLaunchKernelGGL((tzr_hstu_delta_kernel<128>), grid, dim3(HD_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  if (A.nchunk > 1) {
    const int64_t n4 = (int64_t)A.B * A.delta * A.H * (A.Dv >> 2);
    hipLaunchKernelGGL(tzr_hstu_delta_finish_kernel, dim3((unsigned)((n4 + HD_THREADS - 1) / HD_THREADS)), dim3(HD_THREADS), 0, s, A);
    TZR_CHECK_LAUNCH();
  }
  return TZR_OK;
}
