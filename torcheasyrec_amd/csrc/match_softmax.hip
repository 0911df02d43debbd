// The similarity head of the match (retrieval) models (tzrec/models/match_model.py:50-64, 303-336, dssm.py:81-83, 147-155):
// normalize, similarity, temperature and softmax cross entropy over one positive and N sampled negatives per user row (or over
// the other rows of the batch), one launch and a finishing one forward, two launches backward.  As torch ops that is 56 launches
// a pass (measured with the rank, NOTES.md) around a [B, 1 + N] (or [B, B]) score matrix that is written and read several
// times; here the matrix is never in memory (unless the caller asks for it): the forward keeps a running maximum and sum per
// row, the backward recomputes each score tile and p = exp((s - max) - log sum) from the row's saved maximum and log of the sum
// relative to it.
//
//   cosine:    u^_i = U_i / max(|U_i|, 1e-12), v^_j likewise (F.normalize); otherwise u^ = U, v^ = V
//   SAMPLED:   M = B + N; row i has the columns 0: <u^_i, v^_i> / T and 1 + j: <u^_i, v^_{B+j}> / T; the label is column 0
//   IN_BATCH:  M = B; s_ij = <u^_i, v^_j> / T; the label is column i
//   l_i = logsumexp_j s_ij - s_i,label; loss = sum(w l) / sum(w) (0 when sum(w) is 0) or mean(l); rank_i = #{j != label: s_ij >
//   s_i,label}
//
// Tiles.  A workgroup of MS_THREADS = 512 threads (8 waves) OWNS MS_ROWS = 32 rows (two MFMA tiles): user rows in the forward
// and the backward's row pass, item rows in the backward's column pass.  Its rows lie in LDS as they are in memory; it walks the
// OTHER side in tiles of 16 rows, tile k on wave k mod 8, read from memory (L2), and the inverse norms scale the product
// afterwards: s = <u, v> * ru * rv / T, the same bits in every pass, so that sum_j exp(s_ij - lse_i) is 1 in the backward as in
// the forward.  Every product is on v_mfma_f32_16x16x4_f32 (exact fp32).  The score tile is computed TRANSPOSED, acc[r] =
// S[other 4q + r][own li] (the other side is the A operand: lane (li, q) loads the float4 at columns 16 s + 4 q of other row li,
// the four MFMAs of that load take its .x .y .z .w against the same four columns of the own row in LDS:
// the k-slot of an MFMA may stand for any column as long as A and B agree), so a lane holds ONE own row per tile and its
// running (max, sum, rank) are three registers per tile, and the backward's second product needs no transpose: with
// g[other][own] in the accumulator layout, d own^T [16 columns d][16 own] += other^T g has B operand g[4q + e][li] = acc[e] for
// step e, and A operand other[4q + e][16 dt + li], a coalesced load.
// Accumulator chains.  Scores: 4 chains (the float4's components) per own tile, 8 independent MFMAs (32 cycles issue, 40 cycles
// dependent: two would do), added pairwise.  Gradient: one chain per (own tile, 16-column block of D): 8 accumulators (D <= 64,
// two own tiles) or 16 (D <= 256, where a workgroup owns ONE tile of 16 rows in both passes: two would not fit the registers),
// the class a template parameter.  A wave adds its tiles in ascending order; the eight waves are then added
// 0..7 through LDS, and the (max, sum) pairs of the forward are combined q = 0..3 by a fixed xor tree and then waves 0..7.
// LDS per workgroup: forward 32 x 260 floats = 33.3 KB + 1.4 KB of row state (4 workgroups a CU by LDS, 2 by its 512 threads x
// 2 waves a SIMD); backward twice that, 66.6 KB (2 workgroups a CU).  The B operand's LDS reads (row stride 260 floats, columns
// 16 s + 4 q) put the lanes with equal li + q on the same banks, up to four ways: not measured apart, NOTES.md lists it.
// At B = 8192, D <= 64 there are 256 workgroups: one per CU.  The SAMPLED column pass owns 16 item rows a workgroup (RT = 1):
// the negatives are few.
// In SAMPLED mode positive item row i meets user row i alone: the row pass writes dV[i]; the column pass covers rows B..M.  The
// normalisation backward (d - x^ <x^, d>) / max(|x|, eps) runs in each pass's epilogue, the workgroup holds whole rows.
// No atomics; every sum has a fixed order, a function of the shapes alone: two runs are bit-equal.  exp of a difference is
// exp2f(x log2 e) (ms_exp; NOTES.md says why that holds the tests' bound).
#include "parts_sum.h"
#include "tzr_common.h"

#define MS_THREADS 512
#define MS_WAVES (MS_THREADS / TZR_WAVE)
#define MS_RT 2
#define MS_ROWS (16 * MS_RT)
#define MS_MAXD TZR_MATCH_SOFTMAX_MAX_D
#define MS_LS (MS_MAXD + 4)  // LDS row stride in floats (a multiple of 4: rows are read as float4)
#define MS_EPS 1e-12f
#define MS_NEG (-3.0e38f)  // the running maximum before any column (finite: -inf - -inf is NaN)

static_assert(sizeof(TzrMatchSoftmax) == 224, "TzrMatchSoftmax: the layout _lib.py mirrors");
static_assert(MS_THREADS / 16 == MS_ROWS, "prologue and epilogue: sixteen threads per own row");

typedef float ms_f4 __attribute__((ext_vector_type(4)));

struct MsArgs {
  const float* U;
  const float* V;
  const float* w;  // [B], null: none
  int64_t us, vs, B, M;
  int D, mode, cosine;
  float invT;
  float* loss;
  float* lse;
  float* rmax;
  float* lsum;
  float* pos;
  int* rank;
  float* scale;
  double* ru;
  double* rv;
  float* sim;
  int64_t sims;
  float* parts;
  const float* gloss;
  float* dU;
  float* dV;
  int64_t dus, dvs;
};

__device__ __forceinline__ ms_f4 ms_zero() {
  ms_f4 z = {0.f, 0.f, 0.f, 0.f};
  return z;
}
__device__ __forceinline__ float ms_sum16(float v) {  // over the sixteen threads of a row (a fixed xor tree)
  for (int m = 8; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// 1 / max(|x|, eps) of a row's fp32 sum of squares, in double: with 1 / T = 20 a score is 20 times a cosine, and every ulp of an
// inverse norm is an ulp of the score, which exp turns into a relative error of 20 ulp
__device__ __forceinline__ double ms_rnorm(float ss) { return 1.0 / fmax(sqrt((double)ss), (double)MS_EPS); }
__device__ __forceinline__ float ms_sq4(float4 a) { return a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w; }
__device__ __forceinline__ float ms_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 ms_scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// exp(x) for x <= 0 (up to rounding) as exp2f(x log2 e): two instructions where expf is a dozen, and per score this head does
// as much arithmetic as the D = 64 product behind it.  The argument is a DIFFERENCE to the row's maximum (or to its
// log-sum-exp), small where the term matters: rounding x log2 e costs |x| 2^-24 relative, 1e-6 only for terms below e^-15.
#define MS_LOG2E 1.44269504088896340736f
__device__ __forceinline__ float ms_exp(float x) { return exp2f(x * MS_LOG2E); }

// (m1, l1) joined with (m2, l2): max and sum of exp relative to it
__device__ __forceinline__ void ms_join(float& m, float& l, float m2, float l2) {
  const float mm = fmaxf(m, m2);
  l = l * expf(m - mm) + l2 * expf(m2 - mm);
  m = mm;
}

// One score, the same bits in the forward and in both backward passes: the raw product (the same chains whichever side is the A
// operand), then in double the user row's inverse norm, the item row's, 1 / T, rounded once.
__device__ __forceinline__ float ms_score(float acc, double ru, double rv, float invT) { return (float)((double)acc * ru * rv * (double)invT); }

// acc[t][r] = <other row o0 + 4q + r, own row 16 t + li of Os>; *ss: this lane's share of |other row o0 + li|^2 (columns 16 s + 4 q ..)
template <int RT>
__device__ __forceinline__ void ms_scores(const float* Os, const float* __restrict__ Oth, int64_t os, int64_t o0, int64_t On, int D, int li, int q,
                                          ms_f4* acc, float* ss) {
  const bool ook = o0 + li < On;
  const float* op = Oth + (ook ? o0 + li : On - 1) * os;  // (a row past the end: the last row's, zeroed; no branch around a load)
  ms_f4 c[RT][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) c[t][e] = ms_zero();
  float sq = 0.f;
  for (int k0 = 0; k0 < D; k0 += 64) {
    float4 a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 16 * s + 4 * q;
      const float4 x = tzr_ld4(op + min(k, D - 4));
      a[s] = ook && k < D ? x : tzr_zero4();
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (k0 + 16 * s >= D) break;  // (uniform)
      const int k = k0 + 16 * s + 4 * q;
      const bool kok = k < D;
      sq += ms_sq4(a[s]);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const float* bp = Os + (16 * t + li) * MS_LS + (kok ? k : 0);
        const float4 b = kok ? make_float4(bp[0], bp[1], bp[2], bp[3]) : tzr_zero4();
        c[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, b.x, c[t][0], 0, 0, 0);
        c[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, b.y, c[t][1], 0, 0, 0);
        c[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, b.z, c[t][2], 0, 0, 0);
        c[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, b.w, c[t][3], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = (c[t][0] + c[t][1]) + (c[t][2] + c[t][3]);
  *ss = sq;
}

// grid ceil(B / 32)
__global__ __launch_bounds__(MS_THREADS) void tzr_match_softmax_fwd_kernel(MsArgs A) {
  __shared__ __attribute__((aligned(16))) float Os[MS_ROWS * MS_LS];
  __shared__ float Ps[MS_ROWS];
  __shared__ double Rs[MS_ROWS];
  __shared__ float Sm[MS_WAVES * MS_ROWS], Sl[MS_WAVES * MS_ROWS];
  __shared__ int Sr[MS_WAVES * MS_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, li = lane & 15;
  const int64_t b0 = (int64_t)blockIdx.x * MS_ROWS;
  const int D = A.D;
  const bool sampled = A.mode == TZR_MATCH_SAMPLED;
  {  // own rows to LDS, the positive score, the inverse norms
    const int row = tid >> 4, c = tid & 15;
    const int64_t i = b0 + row;
    const bool ok = i < A.B;
    float4 u[4], v[4];
    float su = 0.f, sv = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 4 * c + 64 * s;
      const bool kok = ok && k < D;
      u[s] = kok ? tzr_ld4(A.U + i * A.us + k) : tzr_zero4();
      v[s] = kok ? tzr_ld4(A.V + i * A.vs + k) : tzr_zero4();
      su += ms_sq4(u[s]);
      sv += ms_sq4(v[s]);
    }
    const double ru = A.cosine ? ms_rnorm(ms_sum16(su)) : 1.0;
    const double rvi = A.cosine ? ms_rnorm(ms_sum16(sv)) : 1.0;
    float dot = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 4 * c + 64 * s;
      dot += ms_dot4(u[s], v[s]);
      if (k < D) {
        float* d = Os + row * MS_LS + k;
        d[0] = u[s].x, d[1] = u[s].y, d[2] = u[s].z, d[3] = u[s].w;
      }
    }
    const float p = ms_score(ms_sum16(dot), ru, rvi, A.invT);
    if (c == 0) {
      Ps[row] = p;
      Rs[row] = ru;
      if (ok) {
        A.pos[i] = p;
        if (A.cosine) A.ru[i] = ru;
        if (A.cosine && sampled) A.rv[i] = rvi;
        if (A.sim && sampled) A.sim[i * A.sims] = p;
      }
    }
  }
  __syncthreads();
  float mypos[MS_RT], m[MS_RT], l[MS_RT];
  double myr[MS_RT];
  int rk[MS_RT];
#pragma unroll
  for (int t = 0; t < MS_RT; ++t) {
    mypos[t] = Ps[16 * t + li];
    myr[t] = Rs[16 * t + li];
    const bool col0 = sampled && wv == 0 && q == 0;  // the label column of SAMPLED mode
    m[t] = col0 ? mypos[t] : MS_NEG;
    l[t] = col0 ? 1.0f : 0.f;
    rk[t] = 0;
  }
  const int64_t obeg = sampled ? A.B : 0;
  const int64_t ntile = (A.M - obeg + 15) >> 4;
  for (int64_t tile = wv; tile < ntile; tile += MS_WAVES) {
    const int64_t o0 = obeg + 16 * tile;
    ms_f4 acc[MS_RT];
    float ss;
    ms_scores<MS_RT>(Os, A.V, A.vs, o0, A.M, D, li, q, acc, &ss);
    double rvl = 1.0;
    if (A.cosine) {
      ss += __shfl_xor(ss, 16);
      ss += __shfl_xor(ss, 32);
      rvl = ms_rnorm(ss);
      if (blockIdx.x == 0 && q == 0 && o0 + li < A.M) A.rv[o0 + li] = rvl;
    }
    double ro[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ro[r] = __shfl(rvl, 4 * q + r);
#pragma unroll
    for (int t = 0; t < MS_RT; ++t) {
      const int64_t it = b0 + 16 * t + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t j = o0 + 4 * q + r;
        const bool valid = j < A.M;
        const bool lab = !sampled && j == it;
        const float s = lab ? mypos[t] : ms_score(acc[t][r], myr[t], ro[r], A.invT);
        if (A.sim && valid && it < A.B) A.sim[it * A.sims + (sampled ? 1 + j - A.B : j)] = s;
        if (valid) {
          rk[t] += !lab && s > mypos[t] ? 1 : 0;
          const float d = s - m[t];
          const float e = ms_exp(-fabsf(d));
          l[t] = d > 0.f ? l[t] * e + 1.0f : l[t] + e;
          m[t] = fmaxf(m[t], s);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < MS_RT; ++t) {
    for (int mask = 16; mask <= 32; mask <<= 1) {
      const float m2 = __shfl_xor(m[t], mask), l2 = __shfl_xor(l[t], mask);
      ms_join(m[t], l[t], m2, l2);
      rk[t] += __shfl_xor(rk[t], mask);
    }
    if (q == 0) {
      Sm[wv * MS_ROWS + 16 * t + li] = m[t];
      Sl[wv * MS_ROWS + 16 * t + li] = l[t];
      Sr[wv * MS_ROWS + 16 * t + li] = rk[t];
    }
  }
  __syncthreads();
  if (tid < TZR_WAVE) {
    float a = 0.f, b = 0.f;
    const int64_t i = b0 + tid;
    if (tid < MS_ROWS && i < A.B) {
      float mm = Sm[tid], ll = Sl[tid];
      int rr = Sr[tid];
      for (int w = 1; w < MS_WAVES; ++w) {
        ms_join(mm, ll, Sm[w * MS_ROWS + tid], Sl[w * MS_ROWS + tid]);
        rr += Sr[w * MS_ROWS + tid];
      }
      const float ls = logf(ll);
      A.lse[i] = mm + ls;
      A.rmax[i] = mm;  // (kept apart: mm + ls rounds at the size of the scores, and the backward needs s - lse where it is near 0)
      A.lsum[i] = ls;
      A.rank[i] = rr;
      b = A.w ? A.w[i] : 1.0f;
      a = b * ((mm - Ps[tid]) + ls);
    }
    a = tzr_wave_sum(a);
    b = tzr_wave_sum(b);
    if (tid == 0) {
      A.parts[2 * blockIdx.x] = a;
      A.parts[2 * blockIdx.x + 1] = b;
    }
  }
}

// one workgroup: loss = sum(w l) / sum(w) (0 when the weights add to 0) or sum(l) / B; scale = the reciprocal the backward needs
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_match_softmax_finish_kernel(const float* __restrict__ parts, int G, int has_w, float rows,
                                                                                   float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ float red[TZR_FIN_THREADS];
  __shared__ float tot[2];
  const int col = threadIdx.x & (TZR_WAVE - 1);
  const float r = tzr_parts_sum_interleaved(col < 2 ? parts + col : nullptr, G, 2, red);
  if (threadIdx.x < 2) tot[threadIdx.x] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float sw = has_w ? tot[1] : rows;
    const bool ok = sw != 0.f;  // div_no_nan
    *loss = ok ? tot[0] / sw : 0.f;
    *scale = ok ? 1.0f / sw : 0.f;
  }
}

// ROWPASS: own = user rows, other = item rows (SAMPLED: B..M; the positive pair in the epilogue); writes dU (SAMPLED: and dV[0..B)).
// Column pass: own = item rows (SAMPLED: B..M, IN_BATCH: all), other = every user row in ascending tiles; writes dV.
// NDT: the class's bound on D / 16 rounded up (4, 16).  grid ceil(own rows / 32).
template <int NDT, bool ROWPASS, int RT>
__global__ __launch_bounds__(MS_THREADS) void tzr_match_softmax_bwd_kernel(MsArgs A) {
  __shared__ __attribute__((aligned(16))) float Os[MS_ROWS * MS_LS];
  __shared__ __attribute__((aligned(16))) float Ds[MS_ROWS * MS_LS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, li = lane & 15;
  const int D = A.D;
  const bool sampled = A.mode == TZR_MATCH_SAMPLED;
  const int64_t nbeg = sampled ? A.B : 0;  // the first item row of a tile walk
  const int64_t own0 = (ROWPASS ? 0 : nbeg) + (int64_t)blockIdx.x * (16 * RT);
  const int64_t ownN = ROWPASS ? A.B : A.M;
  const float* Own = ROWPASS ? A.U : A.V;
  const int64_t owns = ROWPASS ? A.us : A.vs;
  const double* rown = ROWPASS ? A.ru : A.rv;
  const float* Oth = ROWPASS ? A.V : A.U;
  const int64_t oths = ROWPASS ? A.vs : A.us;
  const double* roth = ROWPASS ? A.rv : A.ru;
  const int64_t obeg = ROWPASS ? nbeg : 0, oend = ROWPASS ? A.M : A.B;
  const float gs = A.gloss[0] * A.scale[0] * A.invT;  // dL/dl_i / w_i, with the 1 / T of ds/d<u^, v^>
  const int erow = tid >> 4, ec = tid & 15;
  const int64_t ei = own0 + erow;
  const bool eok = erow < 16 * RT && ei < ownN;
  const float er = (float)(A.cosine && eok ? rown[ei] : 1.0);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = 4 * ec + 64 * s;
    if (k < D && erow < 16 * RT) {
      const float4 x = eok ? tzr_ld4(Own + ei * owns + k) : tzr_zero4();
      float* d = Os + erow * MS_LS + k;
      d[0] = x.x, d[1] = x.y, d[2] = x.z, d[3] = x.w;
    }
  }
  __syncthreads();
  float mx_t[RT], ls_t[RT], wp_t[RT], pos_t[RT];  // (ROWPASS: of the lane's own user rows)
  double rown_t[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t it = own0 + 16 * t + li;
    const bool ok = ROWPASS && it < A.B;
    rown_t[t] = A.cosine && it < ownN ? rown[it] : 1.0;
    mx_t[t] = ok ? A.rmax[it] : 0.f;
    ls_t[t] = ok ? A.lsum[it] : 0.f;
    pos_t[t] = ok ? A.pos[it] : 0.f;
    wp_t[t] = ok ? (A.w ? A.w[it] : 1.0f) * gs : 0.f;
  }
  ms_f4 dacc[RT][NDT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dacc[t][dt] = ms_zero();
  const int64_t ntile = (oend - obeg + 15) >> 4;
  for (int64_t tile = wv; tile < ntile; tile += MS_WAVES) {
    const int64_t o0 = obeg + 16 * tile;
    ms_f4 acc[RT];
    float ss;
    // what the tile's other rows bring, loaded ahead of the product and without a branch per load (a row past the end reads the
    // last row's; its g is zeroed below): a conditional load each made four more load latencies a tile (NOTES.md)
    double ro[4] = {1.0, 1.0, 1.0, 1.0};
    float mx_r[4], ls_r[4], wp_r[4], pos_r[4];
    int64_t oc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) oc[r] = o0 + 4 * q + r < oend ? o0 + 4 * q + r : oend - 1;
    if (A.cosine) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ro[r] = roth[oc[r]];
    }
    if (!ROWPASS) {
#pragma unroll
      for (int r = 0; r < 4; ++r) mx_r[r] = A.rmax[oc[r]], ls_r[r] = A.lsum[oc[r]], pos_r[r] = A.pos[oc[r]], wp_r[r] = gs;
      if (A.w) {
#pragma unroll
        for (int r = 0; r < 4; ++r) wp_r[r] = A.w[oc[r]] * gs;
      }
    }
    ms_scores<RT>(Os, Oth, oths, o0, oend, D, li, q, acc, &ss);
    const bool diag = !sampled && o0 < own0 + 16 * RT && o0 + 16 > own0;  // (uniform) the tile holds a label column
    ms_f4 G[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int64_t ownrow = own0 + 16 * t + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t o = o0 + 4 * q + r;
        const bool lab = !sampled && o == ownrow;  // (user row == item row)
        const float mx = ROWPASS ? mx_t[t] : mx_r[r], ls = ROWPASS ? ls_t[t] : ls_r[r];
        const float wp = ROWPASS ? wp_t[t] : wp_r[r], pos = ROWPASS ? pos_t[t] : pos_r[r];
        const float s = lab ? pos : ROWPASS ? ms_score(acc[t][r], rown_t[t], ro[r], A.invT) : ms_score(acc[t][r], ro[r], rown_t[t], A.invT);
        const float x = (s - mx) - ls;  // log p
        float pm = ms_exp(x);  // p - [label]
        if (diag) pm = lab ? expm1f(x) : pm;
        const float g = pm * wp * (float)ro[r];
        G[t][r] = o < oend && ownrow < ownN ? g : 0.f;
      }
    }
    // 64 columns of d own^ at a time: its sixteen operand loads first, with no branch between them (one branch per load made
    // sixteen load latencies a tile, 5.8 us: NOTES.md), then the MFMAs
#pragma unroll
    for (int d0 = 0; d0 < NDT; d0 += 4) {
      if (16 * d0 < D) {  // (uniform)
        float a[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int dd = 0; dd < 4; ++dd) {
            const int64_t o = o0 + 4 * q + e;
            const int d = 16 * (d0 + dd) + li;
            const bool ok = o < oend && d < D;
            const float x = Oth[ok ? o * oths + d : 0];
            a[e][dd] = ok ? x : 0.f;
          }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int dd = 0; dd < 4; ++dd)
#pragma unroll
            for (int t = 0; t < RT; ++t) dacc[t][d0 + dd] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e][dd], G[t][e], dacc[t][d0 + dd], 0, 0, 0);
      }
    }
  }
  // the waves' sums, added 0..7: Ds[own row][d]
  for (int w = 0; w < MS_WAVES; ++w) {
    if (wv == w) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int d = 16 * dt + 4 * q + r;
            if (d < D) {
              float* p = Ds + (16 * t + li) * MS_LS + d;
              *p = w == 0 ? dacc[t][dt][r] : *p + dacc[t][dt][r];
            }
          }
    }
    __syncthreads();
  }
  // epilogue: sixteen threads a row; SAMPLED row pass: the positive pair; the normalisation backward
  float4 x[4], dx[4], v[4], dv[4];
  const bool pair = ROWPASS && sampled;
  float g0 = 0.f, rvi = 1.0f;
  if (pair && eok) {
    const float wp = (A.w ? A.w[ei] : 1.0f) * gs;
    g0 = expm1f((A.pos[ei] - A.rmax[ei]) - A.lsum[ei]) * wp;
    rvi = (float)(A.cosine ? A.rv[ei] : 1.0);
  }
  float xd = 0.f, vd = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = 4 * ec + 64 * s;
    const bool kok = k < D;
    const float* xp = Os + erow * MS_LS + (kok ? k : 0);
    const float* dp = Ds + erow * MS_LS + (kok ? k : 0);
    x[s] = kok ? ms_scale4(make_float4(xp[0], xp[1], xp[2], xp[3]), er) : tzr_zero4();
    dx[s] = kok ? make_float4(dp[0], dp[1], dp[2], dp[3]) : tzr_zero4();
    if (pair) {
      v[s] = kok && eok ? ms_scale4(tzr_ld4(A.V + ei * A.vs + k), rvi) : tzr_zero4();
      dx[s] = tzr_fma4(g0, v[s], dx[s]);
      dv[s] = ms_scale4(x[s], g0);
      vd += ms_dot4(v[s], dv[s]);
    }
    xd += ms_dot4(x[s], dx[s]);
  }
  xd = ms_sum16(xd);
  if (pair) vd = ms_sum16(vd);
  // (a norm below eps was clamped: x^ = x / eps, and the gradient is d / eps)
  const bool xproj = A.cosine && er < 0.5f / MS_EPS, vproj = A.cosine && rvi < 0.5f / MS_EPS;
  float* dOwn = ROWPASS ? A.dU : A.dV;
  const int64_t downs = ROWPASS ? A.dus : A.dvs;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = 4 * ec + 64 * s;
    if (k < D && eok) {
      float4 o = xproj ? tzr_fma4(-xd, x[s], dx[s]) : dx[s];
      tzr_st4(dOwn + ei * downs + k, ms_scale4(o, er));
      if (pair) {
        float4 ov = vproj ? tzr_fma4(-vd, v[s], dv[s]) : dv[s];
        tzr_st4(A.dV + ei * A.dvs + k, ms_scale4(ov, rvi));
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static inline int64_t ms_blocks(int64_t rows) { return (rows + MS_ROWS - 1) / MS_ROWS; }

// limits first (nothing else is looked at for a shape this build has no kernel for), then pointers
static int ms_check(const TzrMatchSoftmax* m, MsArgs* A) {
  if (m->mode != TZR_MATCH_SAMPLED && m->mode != TZR_MATCH_IN_BATCH) return TZR_ERR_UNSUPPORTED;
  if (m->D < 4 || (m->D & 3) || m->D > MS_MAXD || m->B < 1 || m->M < m->B || m->B >= (1ll << 31) || m->M >= (1ll << 31)) return TZR_ERR_UNSUPPORTED;
  if (m->mode == TZR_MATCH_IN_BATCH && m->M != m->B) return TZR_ERR_UNSUPPORTED;
  if (m->cosine != 0 && m->cosine != 1) return TZR_ERR_UNSUPPORTED;
  TZR_TRY(tzr_rows_operand(m->u, m->u_stride, m->D));
  TZR_TRY(tzr_rows_operand(m->v, m->v_stride, m->D));
  if (!m->lse || !m->pos || !m->scale || (m->w & 3) || (m->lse & 3) || (m->pos & 3) || (m->scale & 3)) return TZR_ERR_INVALID;
  if (!m->rmax || !m->lsum || (m->rmax & 3) || (m->lsum & 3)) return TZR_ERR_INVALID;
  if (m->cosine && (!m->ru || !m->rv || (m->ru & 7) || (m->rv & 7))) return TZR_ERR_INVALID;
  A->U = reinterpret_cast<const float*>(m->u);
  A->V = reinterpret_cast<const float*>(m->v);
  A->w = reinterpret_cast<const float*>(m->w);
  A->us = m->u_stride, A->vs = m->v_stride, A->B = m->B, A->M = m->M;
  A->D = m->D, A->mode = m->mode, A->cosine = m->cosine, A->invT = m->inv_temperature;
  A->lse = reinterpret_cast<float*>(m->lse);
  A->rmax = reinterpret_cast<float*>(m->rmax);
  A->lsum = reinterpret_cast<float*>(m->lsum);
  A->pos = reinterpret_cast<float*>(m->pos);
  A->scale = reinterpret_cast<float*>(m->scale);
  A->ru = reinterpret_cast<double*>(m->ru);
  A->rv = reinterpret_cast<double*>(m->rv);
  return TZR_OK;
}

extern "C" size_t tzr_match_softmax_workspace(const TzrMatchSoftmax* h_ms) {
  if (!h_ms || h_ms->B < 1) return 256;
  return tzr_align_up((size_t)ms_blocks(h_ms->B) * 2 * sizeof(float)) + 256;
}

extern "C" int tzr_match_softmax_fwd(const TzrMatchSoftmax* h_ms, void* stream) {
  if (!h_ms) return TZR_ERR_INVALID;
  MsArgs A = {};
  TZR_TRY(ms_check(h_ms, &A));
  if (!h_ms->loss || (h_ms->loss & 3) || !h_ms->rank || (h_ms->rank & 3) || (h_ms->sim & 3)) return TZR_ERR_INVALID;
  if (h_ms->sim && h_ms->sim_stride < (h_ms->mode == TZR_MATCH_SAMPLED ? 1 + h_ms->M - h_ms->B : h_ms->M)) return TZR_ERR_UNSUPPORTED;
  const int64_t G = ms_blocks(h_ms->B);
  if (!h_ms->ws || (h_ms->ws & 255) || h_ms->ws_bytes < tzr_align_up((size_t)G * 2 * sizeof(float))) return TZR_ERR_WORKSPACE;
  A.loss = reinterpret_cast<float*>(h_ms->loss);
  A.rank = reinterpret_cast<int*>(h_ms->rank);
  A.sim = reinterpret_cast<float*>(h_ms->sim);
  A.sims = h_ms->sim_stride;
  A.parts = reinterpret_cast<float*>(h_ms->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tzr_match_softmax_fwd_kernel, dim3((unsigned)G), dim3(MS_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_match_softmax_finish_kernel, dim3(1), dim3(TZR_FIN_THREADS), 0, s, A.parts, (int)G, A.w ? 1 : 0, (float)h_ms->B, A.loss,
                     A.scale);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_match_softmax_bwd(const TzrMatchSoftmax* h_ms, void* stream) {
  if (!h_ms) return TZR_ERR_INVALID;
  MsArgs A = {};
  TZR_TRY(ms_check(h_ms, &A));
  if (!h_ms->grad_loss || (h_ms->grad_loss & 3)) return TZR_ERR_INVALID;
  TZR_TRY(tzr_rows_operand(h_ms->du, h_ms->du_stride, h_ms->D));
  TZR_TRY(tzr_rows_operand(h_ms->dv, h_ms->dv_stride, h_ms->D));
  A.gloss = reinterpret_cast<const float*>(h_ms->grad_loss);
  A.dU = reinterpret_cast<float*>(h_ms->du);
  A.dV = reinterpret_cast<float*>(h_ms->dv);
  A.dus = h_ms->du_stride, A.dvs = h_ms->dv_stride;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t cols = h_ms->mode == TZR_MATCH_SAMPLED ? h_ms->M - h_ms->B : h_ms->M;
  // Rows a workgroup owns in the backward: 32, but 16 (RT = 1) in the SAMPLED column pass -- the negatives are few (the example's
  // 1024: 64 workgroups instead of 32 on 256 compute units) -- and in both passes of the D > 64 class, whose 16 gradient
  // accumulators per own tile do not fit the registers twice (with RT = 2 it spilled 26 / 57 VGPRs to scratch; NOTES.md)
#define MS_PASS(NDT_, ROWPASS_, RT_, rows_)                                                                                              \
  do {                                                                                                                                    \
    hipLaunchKernelGGL((tzr_match_softmax_bwd_kernel<NDT_, ROWPASS_, RT_>), dim3((unsigned)(((rows_) + 16 * RT_ - 1) / (16 * RT_))),      \
                       dim3(MS_THREADS), 0, s, A);                                                                                        \
    TZR_CHECK_LAUNCH();                                                                                                                   \
  } while (0)
  if (h_ms->D <= 64) {
    MS_PASS(4, true, MS_RT, h_ms->B);
    if (cols > 0 && h_ms->mode == TZR_MATCH_SAMPLED) MS_PASS(4, false, 1, cols);
    else if (cols > 0) MS_PASS(4, false, MS_RT, cols);
  } else {
    MS_PASS(16, true, 1, h_ms->B);
    if (cols > 0) MS_PASS(16, false, 1, cols);
  }
#undef MS_PASS
  return TZR_OK;
}
