// The jagged matmul with a weight matrix per sample (tzrec/ops/jagged_tensors.py::jagged_dense_bmm_broadcast_add under
// tzrec/modules/gr/contextualize_mlps.py), fp32, on the jagged rows where they lie; the rule is restated in include/tzrec_hip.h:
//   out[r] = jagged[r] dense[b] + bias[b]          jagged [L, K], dense [B, K, N], bias [B, N], r a row sample b keeps.
// The reference pads the rows to [B, max_seq_len, K] and runs one bmm over all B x max_seq_len positions; here the work follows
// the rows.  Every product is v_mfma_f32_16x16x4_f32 in four accumulator chains (tzr_mfma4 / tzr_join4).
//
// Rows kernel (forward, and d_jagged = g dense[b]^T with K and N swapped), grid blocks x B x chunks, 256 threads.  A workgroup
// owns JB_BLOCK = 64 rows of one sample, wave v the rows 16 v .. 16 v + 15, and JB_CHUNK = 128 output columns: eight 16 x 16
// tiles of four chains each are 128 accumulator registers a lane; all of N = 512 would be 512, so N is split over workgroups
// and the rows are read once a chunk (out of L2 behind the first).  The product is computed TRANSPOSED, out^T = dense^T x^T:
// the panel is the A operand, the wave's rows the B operand -- lane (li, g) holds the float4 at columns 16 s + 4 g of row li,
// fetched from global memory a step ahead, never through LDS -- so that accumulator register r of lane (li, g) is (column
// 16 ct + 4 g + r, row li): a lane ends with four consecutive columns of one row, adds the bias's float4 and stores 16 bytes.
// dense[b]'s panel of a step (sixteen contraction indices x the chunk) goes through LDS once for the four waves: every thread
// fetches its two float4s of the NEXT step before it multiplies and stores them into the other buffer behind the multiply, one
// barrier a step.  Forward: panel rows [16][JB_CHUNK + 4], slot e of lane (li, g) reads [4 g + e][16 ct + li] (the + 4 puts the
// four g of a half wave on two bank groups of sixteen).  d_jagged: the panel is dense[b]'s rows c0 .. c0 + 127 at sixteen
// columns, [JB_CHUNK][16 + 4], and a lane reads the float4 [16 ct + li][4 g]: the transpose costs nothing.
// Blocks at or behind a sample's kept length exit; the late blocks, which only long samples have, are issued first.  Block 0
// of a sample writes the zeros: the rows behind max_seq_len, and for the first and last sample the rows outside the offsets.
//
// Weight kernel (d_dense[b] = jagged_b^T g_b, d_bias[b] = column sums of g_b), grid B x ceil(K / 64) x chunks.  A workgroup owns
// (sample, 64 k, JB_CHUNK n), wave v the k 16 v .. 16 v + 15, and walks the sample's kept rows in order, sixteen a step: the
// rows of jagged ([16][64 + 4]) and g ([16][JB_CHUNK + 4]) go through LDS by the same fetch-ahead; slot e takes row 4 g + e of
// both, g's column as the A operand, so register r of lane (li, g) is (n 16 ct + 4 g + r, k li): 16-byte stores again.  The
// workgroups of the first k tile add g's rows per column in row order: d_bias.  One owner and one fixed order per element: no
// atomics, no workspace, two runs are bit-equal; a sample that keeps no row gets zeros from the empty walk.
#include "tzr_common.h"

#define JB_THREADS 256
#define JB_BLOCK TZR_JAGGED_BMM_BLOCK
#define JB_CHUNK TZR_JAGGED_BMM_CHUNK
#define JB_CT (JB_CHUNK / 16)  // 16 x 16 tiles across a chunk
#define JB_STEP 16             // contraction indices a step
#define JB_KT 64               // k of a weight-kernel workgroup: four waves of one tile

static_assert(sizeof(TzrJaggedBmm) == 136, "TzrJaggedBmm: the layout _lib.py mirrors");
static_assert(JB_BLOCK == 64 && JB_CHUNK == 128, "four waves of 16 rows; 512 panel float4s a step over 256 threads");

struct JbArgs {
  const float *x, *dense, *bias, *jag;  // x: the rows the rows kernel reads (jagged forward, g backward)
  float *out, *dd, *db;
  int64_t xs, os, js;  // floats between rows: x, out, jag
  const int64_t* off;
  int64_t L;
  int B, K, N, max_len, nblk, nchunk, nkt;
};

// the rows sample b keeps
__device__ __forceinline__ void jb_sample(const JbArgs& A, int b, int64_t* start, int64_t* len, int* n) {
  tzr_jagged_span(A.off, b, b + 1, A.L, start, len);
  *n = (int)(*len < (int64_t)A.max_len ? *len : (int64_t)A.max_len);
}

// zeros for the columns [c0, c0 + cw) of the rows [lo, hi) of the output
__device__ __forceinline__ void jb_zero_rows(const JbArgs& A, int64_t lo, int64_t hi, int c0, int cw) {
  const int w4 = cw >> 2;
  for (int64_t i = threadIdx.x; i < (hi - lo) * w4; i += JB_THREADS) {
    const int64_t r = i / w4;
    tzr_st4(A.out + (lo + r) * A.os + c0 + 4 * (i - r * w4), tzr_zero4());
  }
}

// The panel of a step, global -> registers -> LDS; thread t owns the float4s t and t + 256 of its 512.  T false: contraction
// rows 16 s + pr of dense[b] at the chunk's columns; T true: the chunk's rows of dense[b] at the columns 16 s + pc.  What lies
// behind K or N is stored as zeros: a zero times whatever LDS held would not be one.
template <bool T>
struct JbPanel {
  static constexpr int PS = T ? JB_STEP + 4 : JB_CHUNK + 4;  // floats between panel rows
  static constexpr int SIZE = (T ? JB_CHUNK : JB_STEP) * PS;
  const float* src[2];
  int dst[2], lim[2];  // lim: contraction indices in front of which the float4 exists
  int64_t adv;         // floats between steps
  float4 pre[2];

  __device__ __forceinline__ void setup(const float* dense_b, int K, int N, int c0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int i = threadIdx.x + p * JB_THREADS;
      if (!T) {
        const int pr = i >> 5, pc = 4 * (i & 31);
        src[p] = dense_b + (int64_t)pr * N + c0 + pc, dst[p] = pr * PS + pc;
        lim[p] = c0 + pc < N ? K - pr : 0;
      } else {
        const int pr = i >> 2, pc = 4 * (i & 3);
        src[p] = dense_b + (int64_t)(c0 + pr) * N + pc, dst[p] = pr * PS + pc;
        lim[p] = c0 + pr < K ? N - pc : 0;
      }
    }
    adv = T ? JB_STEP : (int64_t)JB_STEP * N;
  }
  __device__ __forceinline__ void fetch(int s) {
#pragma unroll
    for (int p = 0; p < 2; ++p) pre[p] = JB_STEP * s < lim[p] ? tzr_ld4(src[p] + s * adv) : tzr_zero4();
  }
  __device__ __forceinline__ void stash(float* buf) const {
#pragma unroll
    for (int p = 0; p < 2; ++p) tzr_st4(buf + dst[p], pre[p]);
  }
};

// T false: out = x dense[b] + bias[b], contraction K, width N.  T true: out = x dense[b]^T, contraction N, width K.
template <bool T>
__global__ __launch_bounds__(JB_THREADS) void tzr_jagged_bmm_rows_kernel(JbArgs A) {
  using Panel = JbPanel<T>;
  constexpr int PS = Panel::PS;
  __shared__ float Sm[2][Panel::SIZE];
  const int C = T ? A.N : A.K, W = T ? A.K : A.N;
  const unsigned x = blockIdx.x, per = (unsigned)A.B * (unsigned)A.nchunk, u = x / per, v = x - u * per;
  const int blk = A.nblk - 1 - (int)u, b = (int)(v / (unsigned)A.nchunk), c0 = JB_CHUNK * (int)(v - (unsigned)b * (unsigned)A.nchunk);
  const int cw = W - c0 < JB_CHUNK ? W - c0 : JB_CHUNK;
  int64_t start, len;
  int n;
  jb_sample(A, b, &start, &len, &n);
  if (blk == 0) {
    jb_zero_rows(A, start + n, start + len, c0, cw);
    if (b == 0) jb_zero_rows(A, 0, start, c0, cw);
    if (b == A.B - 1) jb_zero_rows(A, start + len, A.L, c0, cw);
  }
  const int r0 = blk * JB_BLOCK;
  if (r0 >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int w0 = r0 + 16 * wv, i = w0 + li;
  const float* xrow = i < n ? A.x + (start + i) * A.xs + 4 * g : nullptr;  // (the lane's float4 of step s: + 16 s)
  tzr_f32x4 acc[4 * JB_CT];
  tzr_acc_zero(acc, 4 * JB_CT);
  Panel pn;
  pn.setup(A.dense + (int64_t)b * A.K * A.N, A.K, A.N, c0);
  const int steps = (C + JB_STEP - 1) / JB_STEP;
  pn.fetch(0);
  pn.stash(Sm[0]);
  float4 xf = xrow && 4 * g < C ? tzr_ld4(xrow) : tzr_zero4();
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const float* P = Sm[s & 1];
    float4 xn = tzr_zero4();
    if (s + 1 < steps) {
      pn.fetch(s + 1);
      if (xrow && JB_STEP * (s + 1) + 4 * g < C) xn = tzr_ld4(xrow + JB_STEP * (s + 1));
    }
    if (w0 < n) {  // (uniform in the wave)
#pragma unroll
      for (int ct = 0; ct < JB_CT; ++ct) {
        if (16 * ct < cw) {  // (uniform in the workgroup)
          float4 pf;
          if (!T) {
            const float* pc = P + 4 * g * PS + 16 * ct + li;
            pf = make_float4(pc[0], pc[PS], pc[2 * PS], pc[3 * PS]);
          } else {
            pf = tzr_ld4(P + (16 * ct + li) * PS + 4 * g);
          }
          tzr_mfma4(pf, xf, acc + 4 * ct);
        }
      }
    }
    if (s + 1 < steps) pn.stash(Sm[(s + 1) & 1]);
    xf = xn;
    __syncthreads();
  }
  if (i >= n) return;
  float* orow = A.out + (start + i) * A.os + c0;
  const float* brow = T ? nullptr : A.bias + (int64_t)b * A.N + c0;
#pragma unroll
  for (int ct = 0; ct < JB_CT; ++ct) {
    const int col = 16 * ct + 4 * g;
    if (col < cw) {
      const tzr_f32x4 r = tzr_join4(acc + 4 * ct);
      float4 o = make_float4(r[0], r[1], r[2], r[3]);
      if (!T) o = tzr_add4(o, tzr_ld4(brow + col));
      tzr_st4(orow + col, o);
    }
  }
}

// Sixteen rows of a sample, global -> registers -> LDS: jagged's 64 columns from k0 ([16][JB_KT + 4] at 0) and g's chunk
// ([16][JB_CHUNK + 4] at GB), 768 float4s, three a thread.  Rows at or behind n, columns at or behind K / N: zeros.
struct JbRowTiles {
  static constexpr int JS = JB_KT + 4, GS = JB_CHUNK + 4, GB = JB_STEP * JS, SIZE = GB + JB_STEP * GS;
  static constexpr int W4 = (JB_KT + JB_CHUNK) / 4;
  const float* src[3];
  int64_t rs[3];
  int row[3], dst[3];  // row -1: a column that does not exist
  float4 pre[3];

  __device__ __forceinline__ void setup(const float* jag, int64_t js, int kw, const float* g, int64_t gs, int nw) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const int i = threadIdx.x + p * JB_THREADS, r = i / W4, cc = i - r * W4;
      const bool isg = cc >= JB_KT / 4;
      const int col = 4 * (isg ? cc - JB_KT / 4 : cc);
      row[p] = col < (isg ? nw : kw) ? r : -1;
      src[p] = (isg ? g : jag) + col, rs[p] = isg ? gs : js;
      dst[p] = isg ? GB + r * GS + col : r * JS + col;
    }
  }
  __device__ __forceinline__ void fetch(int t0, int n) {
#pragma unroll
    for (int p = 0; p < 3; ++p) pre[p] = row[p] >= 0 && t0 + row[p] < n ? tzr_ld4(src[p] + (int64_t)(t0 + row[p]) * rs[p]) : tzr_zero4();
  }
  __device__ __forceinline__ void stash(float* buf) const {
#pragma unroll
    for (int p = 0; p < 3; ++p) tzr_st4(buf + dst[p], pre[p]);
  }
};

// d_dense[b] = jagged_b^T g_b for (64 k, JB_CHUNK n); the k tile 0 also d_bias[b] for its chunk.  A.x: g.
__global__ __launch_bounds__(JB_THREADS) void tzr_jagged_bmm_weight_kernel(JbArgs A) {
  using Tiles = JbRowTiles;
  __shared__ float Sm[2][Tiles::SIZE];
  const unsigned x = blockIdx.x, per = (unsigned)A.nkt * (unsigned)A.nchunk;
  const int b = (int)(x / per), rest = (int)(x - (unsigned)b * per), kt = rest / A.nchunk;
  const int k0 = JB_KT * kt, n0 = JB_CHUNK * (rest - kt * A.nchunk);
  const int kw = A.K - k0 < JB_KT ? A.K - k0 : JB_KT, nw = A.N - n0 < JB_CHUNK ? A.N - n0 : JB_CHUNK;
  int64_t start, len;
  int n;
  jb_sample(A, b, &start, &len, &n);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  tzr_f32x4 acc[4 * JB_CT];
  tzr_acc_zero(acc, 4 * JB_CT);
  float bsum = 0.f;  // thread t < JB_CHUNK of the k tile 0: column t of d_bias
  Tiles ld;
  ld.setup(A.jag + start * A.js + k0, A.js, kw, A.x + start * A.xs + n0, A.xs, nw);
  const int steps = (n + JB_STEP - 1) / JB_STEP;
  if (steps > 0) {
    ld.fetch(0, n);
    ld.stash(Sm[0]);
  }
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const float* Js = Sm[s & 1];
    const float* Gs = Js + Tiles::GB;
    if (s + 1 < steps) ld.fetch(JB_STEP * (s + 1), n);
    if (16 * wv < kw) {  // (uniform in the wave)
      const float* jc = Js + 4 * g * Tiles::JS + 16 * wv + li;
      const float4 jf = make_float4(jc[0], jc[Tiles::JS], jc[2 * Tiles::JS], jc[3 * Tiles::JS]);
#pragma unroll
      for (int ct = 0; ct < JB_CT; ++ct) {
        if (16 * ct < nw) {  // (uniform in the workgroup)
          const float* gc = Gs + 4 * g * Tiles::GS + 16 * ct + li;
          tzr_mfma4(make_float4(gc[0], gc[Tiles::GS], gc[2 * Tiles::GS], gc[3 * Tiles::GS]), jf, acc + 4 * ct);
        }
      }
    }
    if (kt == 0 && tid < nw) {
#pragma unroll
      for (int r = 0; r < JB_STEP; ++r) bsum += Gs[r * Tiles::GS + tid];
    }
    if (s + 1 < steps) ld.stash(Sm[(s + 1) & 1]);
    __syncthreads();
  }
  if (kt == 0 && tid < nw) A.db[(int64_t)b * A.N + n0 + tid] = bsum;
  const int k = 16 * wv + li;
  if (k >= kw) return;
  float* drow = A.dd + ((int64_t)b * A.K + k0 + k) * A.N + n0;
#pragma unroll
  for (int ct = 0; ct < JB_CT; ++ct) {
    const int col = 16 * ct + 4 * g;
    if (col < nw) {
      const tzr_f32x4 r = tzr_join4(acc + 4 * ct);
      tzr_st4(drow + col, make_float4(r[0], r[1], r[2], r[3]));
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------

// sizes, then limits; `A` gets the shape.  TZR_OK with A->B == 0: nothing to launch
static int jb_shape(const TzrJaggedBmm* m, JbArgs* A) {
  if (m->L < 0 || m->B < 0 || !tzr_dim4_ok(m->K, TZR_JAGGED_BMM_MAX_DIM) || !tzr_dim4_ok(m->N, TZR_JAGGED_BMM_MAX_DIM)) return TZR_ERR_INVALID;
  if (m->max_seq_len < 1 || m->max_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->L >= (1ll << 31) || m->B >= (1ll << 31)) return TZR_ERR_UNSUPPORTED;
  const int64_t nblk = ((int64_t)m->max_seq_len + JB_BLOCK - 1) / JB_BLOCK;
  const int64_t wide = m->K > m->N ? m->K : m->N, chunks = (wide + JB_CHUNK - 1) / JB_CHUNK;  // (either direction's chunks, and the k tiles)
  if (m->B > 0 && (nblk * chunks >= (1ll << 31) / m->B || 2 * chunks * chunks >= (1ll << 31) / m->B)) return TZR_ERR_UNSUPPORTED;  // the grids
  A->B = 0;
  if (m->B == 0 || m->L == 0) return TZR_OK;
  if (!m->offsets || (m->offsets & 7) || !m->dense || (m->dense & 15)) return TZR_ERR_INVALID;
  A->off = reinterpret_cast<const int64_t*>(m->offsets), A->dense = reinterpret_cast<const float*>(m->dense);
  A->L = m->L, A->B = (int)m->B, A->K = m->K, A->N = m->N, A->max_len = m->max_seq_len, A->nblk = (int)nblk;
  return TZR_OK;
}

template <bool T>
static void jb_rows_launch(JbArgs A, hipStream_t s) {
  A.nchunk = ((T ? A.K : A.N) + JB_CHUNK - 1) / JB_CHUNK;
  hipLaunchKernelGGL((tzr_jagged_bmm_rows_kernel<T>), dim3((unsigned)((int64_t)A.nblk * A.B * A.nchunk)), dim3(JB_THREADS), 0, s, A);
}

extern "C" int tzr_jagged_bmm_fwd(const TzrJaggedBmm* h_jb, void* stream) {
  if (!h_jb) return TZR_ERR_INVALID;
  JbArgs A = {};
  TZR_TRY(jb_shape(h_jb, &A));
  if (A.B == 0) return TZR_OK;
  if (!h_jb->bias || (h_jb->bias & 15)) return TZR_ERR_INVALID;
  TZR_TRY(tzr_rows_operand(h_jb->jagged, h_jb->jagged_stride, h_jb->K));
  TZR_TRY(tzr_rows_operand(h_jb->out, h_jb->out_stride, h_jb->N));
  A.x = reinterpret_cast<const float*>(h_jb->jagged), A.xs = h_jb->jagged_stride, A.bias = reinterpret_cast<const float*>(h_jb->bias);
  A.out = reinterpret_cast<float*>(h_jb->out), A.os = h_jb->out_stride;
  jb_rows_launch<false>(A, static_cast<hipStream_t>(stream));
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_jagged_bmm_bwd(const TzrJaggedBmm* h_jb, void* stream) {
  if (!h_jb) return TZR_ERR_INVALID;
  JbArgs A = {};
  TZR_TRY(jb_shape(h_jb, &A));
  if (A.B == 0) return TZR_OK;
  if (!h_jb->d_dense || (h_jb->d_dense & 15) || !h_jb->d_bias || (h_jb->d_bias & 15)) return TZR_ERR_INVALID;
  TZR_TRY(tzr_rows_operand(h_jb->jagged, h_jb->jagged_stride, h_jb->K));
  TZR_TRY(tzr_rows_operand(h_jb->grad_out, h_jb->grad_out_stride, h_jb->N));
  TZR_TRY(tzr_rows_operand(h_jb->d_jagged, h_jb->d_jagged_stride, h_jb->K));
  A.x = reinterpret_cast<const float*>(h_jb->grad_out), A.xs = h_jb->grad_out_stride;
  A.jag = reinterpret_cast<const float*>(h_jb->jagged), A.js = h_jb->jagged_stride;
  A.out = reinterpret_cast<float*>(h_jb->d_jagged), A.os = h_jb->d_jagged_stride;
  A.dd = reinterpret_cast<float*>(h_jb->d_dense), A.db = reinterpret_cast<float*>(h_jb->d_bias);
  hipStream_t s = static_cast<hipStream_t>(stream);
  jb_rows_launch<true>(A, s);
  TZR_CHECK_LAUNCH();
  A.nkt = (A.K + JB_KT - 1) / JB_KT, A.nchunk = (A.N + JB_CHUNK - 1) / JB_CHUNK;
  hipLaunchKernelGGL(tzr_jagged_bmm_weight_kernel, dim3((unsigned)((int64_t)A.B * A.nkt * A.nchunk)), dim3(JB_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
