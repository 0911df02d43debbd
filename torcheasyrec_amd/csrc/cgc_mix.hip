// The gate-and-mix step of one CGC (customized gate control) level of PLE (tzrec/modules/extraction_net.py:98-139):
//
//     out_g[b, :] = sum_j softmax(logits_g[b, 0:n_g])_j * expert[sel_g[j]][b, :]          for every gate g of the level
//
// A level has T * P task experts and S shared ones; task gate t mixes its own P experts and the shared ones, the shared gate
// (absent on the last level) all of them: every gate its own SUBSET of the experts, which tzr_moe_mix_* (moe_ops.hip: every
// gate over every expert) cannot express.  The reference stacks each gate's experts ([B, n_g, H], a copy), and per gate runs
// softmax, unsqueeze and a batched matmul of B products [1, n_g] x [n_g, H]; autograd adds a batched product each for the gate
// and the experts, the softmax backward, the un-stacking copies and one add per expert that several gates share -- T + 1 times
// what moe_ops.hip's header counts for one MMoE.  Here: ONE launch per direction for the whole level; every expert row is read
// once for all gates, nothing is stacked, the probabilities are kept for the backward ([B, n_g] per gate), and a shared
// expert's gradient is the sum over its gates in ascending gate order, stored once (no atomics, no zero-fill).
//
// Mapping: moe_ops.hip's -- a group of lgp = 2^k >= H / 4 lanes (at most 64) per row, a lane its float4 column(s).  Membership
// is data: the host turns the member lists into col[g][e] = the logit column of expert e in gate g, or -1.  It travels in the
// kernel arguments, so every test of it is wave-uniform (scalar); the per-lane arrays p[g][e] are only ever indexed by the
// unrolled loop counters (registers, never scratch), and a non-member is skipped by a uniform branch -- not multiplied by a
// zero weight, which would let a NaN of one expert into gates that do not mix it.  The softmax of a row's logits is computed
// redundantly by every lane of the group; the backward's dot products <grad_out_g[b, :], expert_e[b, :]> are reduced over the
// group by shuffles.
#include "tzr_common.h"

#define CG_THREADS 256
#define CG_E TZR_CGC_MAX_EXPERTS
#define CG_G TZR_CGC_MAX_GATES
#define CG_MAX_GRID 1024  // 4 workgroups of 4 waves per CU; the rows beyond one pass are taken by the row loop

static_assert(sizeof(TzrCgcMix) == 1248, "TzrCgcMix: the layout _lib.py mirrors");

struct CgArgs {
  const float* expert[CG_E];
  int64_t expert_stride[CG_E];
  float* d_expert[CG_E];  // backward
  int64_t d_expert_stride[CG_E];
  const float* logits[CG_G];  // forward
  int64_t logits_stride[CG_G];
  float* probs[CG_G];  // [B, n_sel[g]] contiguous: written by the forward, read by the backward
  float* out[CG_G];    // forward: mixed rows [B, H]; backward: d(loss)/d(logits_g) [B, n_sel[g]]
  int64_t out_stride[CG_G];
  const float* g[CG_G];  // backward: d(loss)/d(out_g)
  int64_t g_stride[CG_G];
  int32_t n_sel[CG_G];
  int8_t col[CG_G][CG_E];  // logit column of expert e in gate g; -1: not a member
};

// GG / EE: compile-time bounds of the gate / expert loops (the smallest instantiated pair covering G, E)
template <int GG, int EE>
__global__ __launch_bounds__(CG_THREADS) void tzr_cgc_mix_fwd_kernel(CgArgs A, int64_t B, int H, int E, int G, int lgp) {
  const int N4 = H >> 2;
  const int rpw = TZR_WAVE / lgp;
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int gi = lane / lgp, c = lane - gi * lgp;
  const int64_t wave = (int64_t)blockIdx.x * (CG_THREADS / TZR_WAVE) + threadIdx.x / TZR_WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (CG_THREADS / TZR_WAVE);
  for (int64_t b = wave * rpw + gi; b < B; b += n_waves * rpw) {
    float p[GG][EE];
#pragma unroll
    for (int g = 0; g < GG; ++g) {
      if (g >= G) continue;  // (not `break`: the loop must unroll)
      const float* lg = A.logits[g] + b * A.logits_stride[g];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? A.col[g][e] : -1;
        p[g][e] = j >= 0 ? lg[j] : -INFINITY;
        mx = fmaxf(mx, p[g][e]);
      }
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? A.col[g][e] : -1;
        p[g][e] = j >= 0 ? expf(p[g][e] - mx) : 0.f;
        s += p[g][e];
      }
      const float inv = 1.0f / s;
      float* pr = A.probs[g] + b * A.n_sel[g];
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? A.col[g][e] : -1;
        p[g][e] *= inv;
        if (c == 0 && j >= 0) pr[j] = p[g][e];
      }
    }
    for (int cc = c; cc < N4; cc += lgp) {
      float4 x[EE];
#pragma unroll
      for (int e = 0; e < EE; ++e) x[e] = e < E ? tzr_ld4(A.expert[e] + b * A.expert_stride[e] + 4 * cc) : tzr_zero4();
#pragma unroll
      for (int g = 0; g < GG; ++g) {
        if (g >= G) continue;  // (not `break`: the loop must unroll)
        float4 o = tzr_zero4();
#pragma unroll
        for (int e = 0; e < EE; ++e)
          if (e < E && A.col[g][e] >= 0) o = tzr_fma4(p[g][e], x[e], o);
        tzr_st4(A.out[g] + b * A.out_stride[g] + 4 * cc, o);
      }
    }
  }
}

template <int GG, int EE>
__global__ __launch_bounds__(CG_THREADS) void tzr_cgc_mix_bwd_kernel(CgArgs A, int64_t B, int H, int E, int G, int lgp) {
  const int N4 = H >> 2;
  const int rpw = TZR_WAVE / lgp;
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int gi = lane / lgp, c = lane - gi * lgp;
  const int64_t wave = (int64_t)blockIdx.x * (CG_THREADS / TZR_WAVE) + threadIdx.x / TZR_WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (CG_THREADS / TZR_WAVE);
  // (every lane of a wave runs the same number of iterations: the shuffles below are wave-wide)
  for (int64_t b0 = wave * rpw; b0 < B; b0 += n_waves * rpw) {
    const int64_t b = b0 + gi;
    const bool on = b < B;
    float p[GG][EE], dp[GG][EE];
#pragma unroll
    for (int g = 0; g < GG; ++g)
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = (g < G && e < E) ? A.col[g][e] : -1;
        p[g][e] = (on && j >= 0) ? A.probs[g][b * A.n_sel[g] + j] : 0.f;
        dp[g][e] = 0.f;
      }
    for (int cc = c; cc < N4 + c; cc += lgp) {  // (c < lgp: the same trip count for every lane; columns >= N4 are idle)
      const bool colon = on && cc < N4;
      float4 go[GG];
#pragma unroll
      for (int g = 0; g < GG; ++g) go[g] = (colon && g < G) ? tzr_ld4(A.g[g] + b * A.g_stride[g] + 4 * cc) : tzr_zero4();
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        if (e >= E) continue;  // (not `break`: the loop must unroll, p and dp are registers)
        const float4 x = colon ? tzr_ld4(A.expert[e] + b * A.expert_stride[e] + 4 * cc) : tzr_zero4();
        float4 o = tzr_zero4();  // (an expert of no gate: zeros)
#pragma unroll
        for (int g = 0; g < GG; ++g) {  // ascending gate order: the sum a shared expert gets is the same on every run
          if (g < G && A.col[g][e] >= 0) {
            o = tzr_fma4(p[g][e], go[g], o);
            dp[g][e] += go[g].x * x.x + go[g].y * x.y + go[g].z * x.z + go[g].w * x.w;
          }
        }
        if (colon) tzr_st4(A.d_expert[e] + b * A.d_expert_stride[e] + 4 * cc, o);
      }
    }
#pragma unroll
    for (int g = 0; g < GG; ++g) {
      if (g >= G) continue;  // (not `break`: the loop must unroll)
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        if (e < E && A.col[g][e] >= 0) {  // (uniform: every lane of the wave shuffles or none)
          float v = dp[g][e];
          for (int m = lgp >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, TZR_WAVE);
          dp[g][e] = v;
          dot += p[g][e] * v;
        }
      }
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? A.col[g][e] : -1;
        if (on && c == 0 && j >= 0) A.out[g][b * A.out_stride[g] + j] = p[g][e] * (dp[g][e] - dot);
      }
    }
  }
}

// a [B, H] operand: a null or misaligned pointer is an error, a row stride the float4 accesses cannot take is unsupported
static int cg_rows(uint64_t ptr, int64_t stride, int H) {
  if (!ptr || (ptr & 15)) return TZR_ERR_INVALID;
  return ((stride & 3) || stride < H) ? TZR_ERR_UNSUPPORTED : TZR_OK;
}
// a [B, n] operand read and written by scalars (logits, d_logits)
static int cg_cols(uint64_t ptr, int64_t stride, int n) {
  if (!ptr || (ptr & 3)) return TZR_ERR_INVALID;
  return stride < n ? TZR_ERR_UNSUPPORTED : TZR_OK;
}
#define CG_TRY(expr)                 \
  do {                               \
    const int rc_ = (expr);          \
    if (rc_ != TZR_OK) return rc_;   \
  } while (0)

// sizes, limits, the experts, the member lists and the probabilities: what both directions need.  B == 0 is the caller's.
static int cg_check(const TzrCgcMix* m, CgArgs* A) {
  if (m->B < 0 || m->H <= 0 || m->n_experts <= 0 || m->n_gates <= 0) return TZR_ERR_INVALID;
  if (m->n_experts > CG_E || m->n_gates > CG_G || (m->H & 3) || m->H > 4096) return TZR_ERR_UNSUPPORTED;
  for (int g = 0; g < m->n_gates; ++g) {
    if (m->n_sel[g] <= 0) return TZR_ERR_INVALID;
    if (m->n_sel[g] > CG_E) return TZR_ERR_UNSUPPORTED;
  }
  for (int e = 0; e < m->n_experts; ++e) {
    CG_TRY(cg_rows(m->expert[e], m->expert_stride[e], m->H));
    A->expert[e] = reinterpret_cast<const float*>(m->expert[e]);
    A->expert_stride[e] = m->expert_stride[e];
  }
  for (int g = 0; g < m->n_gates; ++g) {
    for (int e = 0; e < CG_E; ++e) A->col[g][e] = -1;
    for (int j = 0; j < m->n_sel[g]; ++j) {
      const int e = m->sel[g][j];
      if (e < 0 || e >= m->n_experts || A->col[g][e] >= 0) return TZR_ERR_INVALID;  // out of range, or twice in one gate
      A->col[g][e] = (int8_t)j;
    }
    if (!m->probs[g] || (m->probs[g] & 3)) return TZR_ERR_INVALID;
    A->n_sel[g] = m->n_sel[g];
    A->probs[g] = reinterpret_cast<float*>(m->probs[g]);
  }
  return TZR_OK;
}

static void cg_geometry(const TzrCgcMix* m, int* lgp, unsigned* grid) {
  int l = 1;
  while (l < (m->H >> 2) && l < TZR_WAVE) l <<= 1;
  const int rpw = TZR_WAVE / l;
  const int64_t rows_per_wg = (int64_t)rpw * (CG_THREADS / TZR_WAVE);
  *lgp = l;
  *grid = (unsigned)std::min<int64_t>((m->B + rows_per_wg - 1) / rows_per_wg, CG_MAX_GRID);
}

#define CG_LAUNCH(K, GG_, EE_)                                                                                              \
  hipLaunchKernelGGL((K<GG_, EE_>), dim3(grid), dim3(CG_THREADS), 0, static_cast<hipStream_t>(stream), A, h_mix->B, h_mix->H, \
                     h_mix->n_experts, h_mix->n_gates, lgp)
#define CG_BY_E(K, GG_)                                   \
  do {                                                    \
    if (h_mix->n_experts <= 4) CG_LAUNCH(K, GG_, 4);      \
    else if (h_mix->n_experts <= 8) CG_LAUNCH(K, GG_, 8); \
    else CG_LAUNCH(K, GG_, 16);                           \
  } while (0)
#define CG_DISPATCH(K)                            \
  do {                                            \
    if (h_mix->n_gates <= 1) CG_BY_E(K, 1);       \
    else if (h_mix->n_gates <= 3) CG_BY_E(K, 3);  \
    else CG_BY_E(K, 5);                           \
  } while (0)

extern "C" int tzr_cgc_mix_fwd(const TzrCgcMix* h_mix, void* stream) {
  if (!h_mix) return TZR_ERR_INVALID;
  if (h_mix->B == 0) return TZR_OK;
  CgArgs A = {};
  CG_TRY(cg_check(h_mix, &A));
  for (int g = 0; g < h_mix->n_gates; ++g) {
    CG_TRY(cg_cols(h_mix->logits[g], h_mix->logits_stride[g], h_mix->n_sel[g]));
    CG_TRY(cg_rows(h_mix->out[g], h_mix->out_stride[g], h_mix->H));
    A.logits[g] = reinterpret_cast<const float*>(h_mix->logits[g]);
    A.logits_stride[g] = h_mix->logits_stride[g];
    A.out[g] = reinterpret_cast<float*>(h_mix->out[g]);
    A.out_stride[g] = h_mix->out_stride[g];
  }
  int lgp;
  unsigned grid;
  cg_geometry(h_mix, &lgp, &grid);
  CG_DISPATCH(tzr_cgc_mix_fwd_kernel);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_cgc_mix_bwd(const TzrCgcMix* h_mix, void* stream) {
  if (!h_mix) return TZR_ERR_INVALID;
  if (h_mix->B == 0) return TZR_OK;
  CgArgs A = {};
  CG_TRY(cg_check(h_mix, &A));
  for (int e = 0; e < h_mix->n_experts; ++e) {
    CG_TRY(cg_rows(h_mix->d_expert[e], h_mix->d_expert_stride[e], h_mix->H));
    A.d_expert[e] = reinterpret_cast<float*>(h_mix->d_expert[e]);
    A.d_expert_stride[e] = h_mix->d_expert_stride[e];
  }
  for (int g = 0; g < h_mix->n_gates; ++g) {
    CG_TRY(cg_rows(h_mix->grad_out[g], h_mix->grad_out_stride[g], h_mix->H));
    CG_TRY(cg_cols(h_mix->d_logits[g], h_mix->d_logits_stride[g], h_mix->n_sel[g]));
    A.g[g] = reinterpret_cast<const float*>(h_mix->grad_out[g]);
    A.g_stride[g] = h_mix->grad_out_stride[g];
    A.out[g] = reinterpret_cast<float*>(h_mix->d_logits[g]);
    A.out_stride[g] = h_mix->d_logits_stride[g];
  }
  int lgp;
  unsigned grid;
  cg_geometry(h_mix, &lgp, &grid);
  CG_DISPATCH(tzr_cgc_mix_bwd_kernel);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
