// Softmax gates that mix expert rows, every gate of a layer in one launch per direction:
//
//     out_g[b, :] = sum_j softmax(logits_g[b, 0:n_g])_j * expert[sel_g[j]][b, :]          for every gate g
//
// Two ABIs, one kernel body:
//   tzr_moe_mix_*  MMoE's mixing step (tzrec/modules/mmoe.py:63-76): every gate (task) lists every expert in logit-column order.
//                  tzr_gate_mix_{fwd,bwd}_kernel<GG, EE, false>, GG in {1, 2, 4} by EE in {2, 4, 8}, at most 4096 workgroups.
//   tzr_cgc_mix_*  one CGC level of PLE (tzrec/modules/extraction_net.py:98-139): T * P task experts and S shared ones; task gate
//                  t mixes its own P experts and the shared ones, the shared gate (absent on the last level) all of them.
//                  tzr_gate_mix_{fwd,bwd}_kernel<GG, EE, true>, GG in {1, 3, 5} by EE in {4, 8, 16}, at most 1024 workgroups.
//
// The reference stacks each gate's experts ([B, n_g, H], a copy), and per gate runs softmax, unsqueeze and a batched matmul of
// B products [1, n_g] x [n_g, H]; autograd adds a batched product each for the gate and the experts, the softmax backward, the
// un-stacking copies and the sum of an expert's gradients over the gates that share it.  For one MMoE at B = 8192, E = 3,
// H = 128 that is ~20 launches of 5-19 us for 12 MB of data (profiles/r05y: the three strided-batched GEMMs alone 18.6 + 14.1 +
// 11.8 us per task); a CGC level costs T + 1 times that.  Here: ONE launch per direction for all gates; every expert row is read
// once for all gates, nothing is stacked, the probabilities are kept for the backward ([B, n_g] per gate), and an expert's
// gradient is the sum over its gates in ascending gate order, stored once (no atomics, no zero-fill).  HBM-light; what it buys
// is launches.
//
// Mapping: a group of lgp = 2^k >= H / 4 lanes (at most 64) per row, a lane its float4 column(s).  The softmax of a row's logits
// is computed redundantly by every lane of the group (at most 16 cached loads per gate); the backward's dot products
// <grad_out_g[b, :], expert_e[b, :]> are reduced over the group by shuffles.
//
// Membership is data: the host turns the member lists into col[g][e] = the logit column of expert e in gate g, or -1.  It
// travels in the kernel arguments, so every test of it is wave-uniform (scalar); the per-lane arrays p[g][e] are only ever
// indexed by the unrolled loop counters (registers, never scratch), and a non-member is skipped by a uniform branch -- not
// multiplied by a zero weight, which would let a NaN of one expert into gates that do not mix it.  With SUBSET = false (MMoE)
// col[g][e] is e and n_sel[g] is E at compile time: neither table is read, and every gate mixes every expert, so there is
// nothing to keep apart (GM_TAKES).  Loops over the compile-time bounds skip their tail with `continue`, not `break`: the loop
// must unroll, or p and dp leave the registers (one loop of the MMoE forward says why it differs).
#include "tzr_common.h"

#define GM_THREADS 256
#define GM_E TZR_CGC_MAX_EXPERTS  // (TZR_MOE_MAX_EXPERTS / _TASKS fit inside)
#define GM_G TZR_CGC_MAX_GATES
#define GM_MOE_MAX_GRID 4096
#define GM_CGC_MAX_GRID 1024  // 4 workgroups of 4 waves per CU; the rows beyond one pass are taken by the row loop

static_assert(TZR_MOE_MAX_EXPERTS <= GM_E && TZR_MOE_MAX_TASKS <= GM_G, "TzrMoeMix must fit the kernel arguments");
static_assert(sizeof(TzrCgcMix) == 1248, "TzrCgcMix: the layout _lib.py mirrors");

struct GmArgs {
  const float* expert[GM_E];
  int64_t expert_stride[GM_E];
  float* d_expert[GM_E];  // backward
  int64_t d_expert_stride[GM_E];
  const float* logits[GM_G];  // forward
  int64_t logits_stride[GM_G];
  float* probs[GM_G];  // [B, n_sel[g]] contiguous: written by the forward, read by the backward
  float* out[GM_G];    // forward: mixed rows [B, H]; backward: d(loss)/d(logits_g) [B, n_sel[g]]
  int64_t out_stride[GM_G];
  const float* g[GM_G];  // backward: d(loss)/d(out_g)
  int64_t g_stride[GM_G];
  int32_t n_sel[GM_G];     // SUBSET only
  int8_t col[GM_G][GM_E];  // SUBSET only: logit column of expert e in gate g; -1: not a member
};

// (macros, not helpers that take A: the argument struct must stay in the kernel's scalar registers)
#define GM_COL(g, e) (SUBSET ? (int)A.col[g][e] : (e))        // logit column of expert e < E in gate g < G
// does the arithmetic of gate g take expert e: SUBSET, a uniform branch on the bounds and the membership (the NaN rule above);
// otherwise always -- past G and E the weights, the expert rows and the output gradients are zeros that add exactly nothing,
// and no branch splits the unrolled code
#define GM_TAKES(g, e) (!SUBSET || ((g) < G && (e) < E && A.col[g][e] >= 0))
#define GM_N_SEL(g) (SUBSET ? (int)A.n_sel[g] : E)

// GG / EE: compile-time bounds of the gate / expert loops (the smallest instantiated pair covering G, E)
template <int GG, int EE, bool SUBSET>
__global__ __launch_bounds__(GM_THREADS) void tzr_gate_mix_fwd_kernel(GmArgs A, int64_t B, int H, int E, int G, int lgp) {
  const int N4 = H >> 2;
  const int rpw = TZR_WAVE / lgp;
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int gi = lane / lgp, c = lane - gi * lgp;
  const int64_t wave = (int64_t)blockIdx.x * (GM_THREADS / TZR_WAVE) + threadIdx.x / TZR_WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (GM_THREADS / TZR_WAVE);
  for (int64_t b = wave * rpw + gi; b < B; b += n_waves * rpw) {
    float p[GG][EE];
#pragma unroll
    for (int g = 0; g < GG; ++g) {
      if (g >= G) continue;
      const float* lg = A.logits[g] + b * A.logits_stride[g];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? GM_COL(g, e) : -1;
        p[g][e] = j >= 0 ? lg[j] : -INFINITY;
        mx = fmaxf(mx, p[g][e]);
      }
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? GM_COL(g, e) : -1;
        p[g][e] = j >= 0 ? expf(p[g][e] - mx) : 0.f;
        s += p[g][e];
      }
      const float inv = 1.0f / s;
      float* pr = A.probs[g] + b * GM_N_SEL(g);
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? GM_COL(g, e) : -1;
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
        if (g >= G) {
          if (SUBSET) continue;
          // MMoE, this loop alone: behind `continue` the gates' blocks join, the compiler no longer knows what is in flight
          // there, and every store waits for the one before it (s_waitcnt vmcnt(0)): 1 us of 14 at B = 8192, H = 256,
          // T = E = 4 (profiles/gate_mix).  `break` nests the blocks; the loop still unrolls (no scratch).
          break;
        }
        float4 o = tzr_zero4();
#pragma unroll
        for (int e = 0; e < EE; ++e)
          if (GM_TAKES(g, e)) o = tzr_fma4(p[g][e], x[e], o);
        tzr_st4(A.out[g] + b * A.out_stride[g] + 4 * cc, o);
      }
    }
  }
}

template <int GG, int EE, bool SUBSET>
__global__ __launch_bounds__(GM_THREADS) void tzr_gate_mix_bwd_kernel(GmArgs A, int64_t B, int H, int E, int G, int lgp) {
  const int N4 = H >> 2;
  const int rpw = TZR_WAVE / lgp;
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int gi = lane / lgp, c = lane - gi * lgp;
  const int64_t wave = (int64_t)blockIdx.x * (GM_THREADS / TZR_WAVE) + threadIdx.x / TZR_WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (GM_THREADS / TZR_WAVE);
  // (every lane of a wave runs the same number of iterations: the shuffles below are wave-wide)
  for (int64_t b0 = wave * rpw; b0 < B; b0 += n_waves * rpw) {
    const int64_t b = b0 + gi;
    const bool on = b < B;
    float p[GG][EE], dp[GG][EE];
#pragma unroll
    for (int g = 0; g < GG; ++g)
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = (g < G && e < E) ? GM_COL(g, e) : -1;
        p[g][e] = (on && j >= 0) ? A.probs[g][b * GM_N_SEL(g) + j] : 0.f;
        dp[g][e] = 0.f;
      }
    for (int cc = c; cc < N4 + c; cc += lgp) {  // (c < lgp: the same trip count for every lane; columns >= N4 are idle)
      const bool colon = on && cc < N4;
      float4 go[GG];
#pragma unroll
      for (int g = 0; g < GG; ++g) go[g] = (colon && g < G) ? tzr_ld4(A.g[g] + b * A.g_stride[g] + 4 * cc) : tzr_zero4();
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        if (e >= E) continue;
        const float4 x = colon ? tzr_ld4(A.expert[e] + b * A.expert_stride[e] + 4 * cc) : tzr_zero4();
        float4 o = tzr_zero4();  // (an expert of no gate: zeros)
#pragma unroll
        for (int g = 0; g < GG; ++g) {  // ascending gate order: the sum a shared expert gets is the same on every run
          if (GM_TAKES(g, e)) {
            o = tzr_fma4(p[g][e], go[g], o);
            dp[g][e] += go[g].x * x.x + go[g].y * x.y + go[g].z * x.z + go[g].w * x.w;
          }
        }
        if (colon) tzr_st4(A.d_expert[e] + b * A.d_expert_stride[e] + 4 * cc, o);
      }
    }
#pragma unroll
    for (int g = 0; g < GG; ++g) {
      if (g >= G) continue;
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        if (GM_TAKES(g, e)) {  // (uniform: every lane of the wave shuffles or none)
          float v = dp[g][e];
          for (int m = lgp >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, TZR_WAVE);
          dp[g][e] = v;
          dot += p[g][e] * v;
        }
      }
#pragma unroll
      for (int e = 0; e < EE; ++e) {
        const int j = e < E ? GM_COL(g, e) : -1;
        if (on && c == 0 && j >= 0) A.out[g][b * A.out_stride[g] + j] = p[g][e] * (dp[g][e] - dot);
      }
    }
  }
}
#undef GM_COL
#undef GM_TAKES
#undef GM_N_SEL

// ---- host: one launch path; each ABI its own checks and status codes -------------------------------------------------------

#define GM_LAUNCH(K, GG_, EE_, S_) \
  hipLaunchKernelGGL((K<GG_, EE_, S_>), dim3(grid), dim3(GM_THREADS), 0, static_cast<hipStream_t>(stream), A, B, H, E, G, lgp)
#define GM_BY_E(K, GG_, S_, E1, E2, E3)             \
  do {                                              \
    if (E <= E1) GM_LAUNCH(K, GG_, E1, S_);         \
    else if (E <= E2) GM_LAUNCH(K, GG_, E2, S_);    \
    else GM_LAUNCH(K, GG_, E3, S_);                 \
  } while (0)
// the smallest instantiated class (G1 < G2 < G3) x (E1 < E2 < E3) that covers G gates and E experts
#define GM_DISPATCH(K, S_, G1, G2, G3, E1, E2, E3)       \
  do {                                                   \
    if (G <= G1) GM_BY_E(K, G1, S_, E1, E2, E3);         \
    else if (G <= G2) GM_BY_E(K, G2, S_, E1, E2, E3);    \
    else GM_BY_E(K, G3, S_, E1, E2, E3);                 \
  } while (0)

static void gm_geometry(int64_t B, int H, int max_grid, int* lgp, unsigned* grid) {
  int l = 1;
  while (l < (H >> 2) && l < TZR_WAVE) l <<= 1;
  const int rpw = TZR_WAVE / l;
  const int64_t rows_per_wg = (int64_t)rpw * (GM_THREADS / TZR_WAVE);
  *lgp = l;
  *grid = (unsigned)std::min<int64_t>((B + rows_per_wg - 1) / rows_per_wg, max_grid);
}

// the operands of one direction (both ABI structs name them alike), then the launch; everything is checked by now
template <class Mix>
static int gm_run(const Mix* m, int G, bool subset, bool fwd, GmArgs& A, void* stream) {
  const int64_t B = m->B;
  const int H = m->H, E = m->n_experts;
  for (int e = 0; e < E; ++e) {
    A.expert[e] = reinterpret_cast<const float*>(m->expert[e]);
    A.expert_stride[e] = m->expert_stride[e];
    if (!fwd) {
      A.d_expert[e] = reinterpret_cast<float*>(m->d_expert[e]);
      A.d_expert_stride[e] = m->d_expert_stride[e];
    }
  }
  for (int g = 0; g < G; ++g) {
    A.probs[g] = reinterpret_cast<float*>(m->probs[g]);
    if (fwd) {
      A.logits[g] = reinterpret_cast<const float*>(m->logits[g]);
      A.logits_stride[g] = m->logits_stride[g];
    } else {
      A.g[g] = reinterpret_cast<const float*>(m->grad_out[g]);
      A.g_stride[g] = m->grad_out_stride[g];
    }
    A.out[g] = reinterpret_cast<float*>(fwd ? m->out[g] : m->d_logits[g]);
    A.out_stride[g] = fwd ? m->out_stride[g] : m->d_logits_stride[g];
  }
  int lgp;
  unsigned grid;
  gm_geometry(B, H, subset ? GM_CGC_MAX_GRID : GM_MOE_MAX_GRID, &lgp, &grid);
  if (subset) {
    if (fwd) GM_DISPATCH(tzr_gate_mix_fwd_kernel, true, 1, 3, 5, 4, 8, 16);
    else GM_DISPATCH(tzr_gate_mix_bwd_kernel, true, 1, 3, 5, 4, 8, 16);
  } else {
    if (fwd) GM_DISPATCH(tzr_gate_mix_fwd_kernel, false, 1, 2, 4, 2, 4, 8);
    else GM_DISPATCH(tzr_gate_mix_bwd_kernel, false, 1, 2, 4, 2, 4, 8);
  }
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// tzr_moe_mix_*: whatever is wrong with an operand is TZR_ERR_INVALID; a row stride below H is not looked at
static bool mx_rows_bad(uint64_t ptr, int64_t stride) { return !ptr || (stride & 3) || (ptr & 15); }

static int mx_mix(const TzrMoeMix* m, bool fwd, void* stream) {
  if (!m || m->B <= 0 || m->n_experts <= 0 || m->n_tasks <= 0 || m->H <= 0) return TZR_ERR_INVALID;
  if (m->n_experts > TZR_MOE_MAX_EXPERTS || m->n_tasks > TZR_MOE_MAX_TASKS || (m->H & 3) || m->H > 4096) return TZR_ERR_UNSUPPORTED;
  for (int e = 0; e < m->n_experts; ++e)
    if (mx_rows_bad(m->expert[e], m->expert_stride[e]) || (!fwd && mx_rows_bad(m->d_expert[e], m->d_expert_stride[e]))) return TZR_ERR_INVALID;
  for (int t = 0; t < m->n_tasks; ++t) {
    if (!m->probs[t]) return TZR_ERR_INVALID;
    if (fwd ? (!m->logits[t] || mx_rows_bad(m->out[t], m->out_stride[t]) || m->logits_stride[t] < m->n_experts)
            : (!m->d_logits[t] || mx_rows_bad(m->grad_out[t], m->grad_out_stride[t]) || m->d_logits_stride[t] < m->n_experts))
      return TZR_ERR_INVALID;
  }
  GmArgs A = {};
  return gm_run(m, m->n_tasks, false, fwd, A, stream);
}

extern "C" int tzr_moe_mix_fwd(const TzrMoeMix* h_mix, void* stream) { return mx_mix(h_mix, true, stream); }
extern "C" int tzr_moe_mix_bwd(const TzrMoeMix* h_mix, void* stream) { return mx_mix(h_mix, false, stream); }

// tzr_cgc_mix_*: a null or misaligned pointer is an error, a stride the accesses cannot take is unsupported (include/tzrec_hip.h)
// a [B, n] operand read and written by scalars (logits, d_logits)
static int cg_cols(uint64_t ptr, int64_t stride, int n) {
  if (!ptr || (ptr & 3)) return TZR_ERR_INVALID;
  return stride < n ? TZR_ERR_UNSUPPORTED : TZR_OK;
}

static int cg_mix(const TzrCgcMix* m, bool fwd, void* stream) {
  if (!m) return TZR_ERR_INVALID;
  if (m->B == 0) return TZR_OK;
  if (m->B < 0 || m->H <= 0 || m->n_experts <= 0 || m->n_gates <= 0) return TZR_ERR_INVALID;
  if (m->n_experts > GM_E || m->n_gates > GM_G || (m->H & 3) || m->H > 4096) return TZR_ERR_UNSUPPORTED;
  for (int g = 0; g < m->n_gates; ++g) {
    if (m->n_sel[g] <= 0) return TZR_ERR_INVALID;
    if (m->n_sel[g] > GM_E) return TZR_ERR_UNSUPPORTED;
  }
  for (int e = 0; e < m->n_experts; ++e) TZR_TRY(tzr_rows_operand(m->expert[e], m->expert_stride[e], m->H));
  GmArgs A = {};
  for (int g = 0; g < m->n_gates; ++g) {
    for (int e = 0; e < GM_E; ++e) A.col[g][e] = -1;
    for (int j = 0; j < m->n_sel[g]; ++j) {
      const int e = m->sel[g][j];
      if (e < 0 || e >= m->n_experts || A.col[g][e] >= 0) return TZR_ERR_INVALID;  // out of range, or twice in one gate
      A.col[g][e] = (int8_t)j;
    }
    if (!m->probs[g] || (m->probs[g] & 3)) return TZR_ERR_INVALID;
    A.n_sel[g] = m->n_sel[g];
  }
  if (!fwd)
    for (int e = 0; e < m->n_experts; ++e) TZR_TRY(tzr_rows_operand(m->d_expert[e], m->d_expert_stride[e], m->H));
  for (int g = 0; g < m->n_gates; ++g) {
    if (fwd) {
      TZR_TRY(cg_cols(m->logits[g], m->logits_stride[g], m->n_sel[g]));
      TZR_TRY(tzr_rows_operand(m->out[g], m->out_stride[g], m->H));
    } else {
      TZR_TRY(tzr_rows_operand(m->grad_out[g], m->grad_out_stride[g], m->H));
      TZR_TRY(cg_cols(m->d_logits[g], m->d_logits_stride[g], m->n_sel[g]));
    }
  }
  return gm_run(m, m->n_gates, true, fwd, A, stream);
}

extern "C" int tzr_cgc_mix_fwd(const TzrCgcMix* h_mix, void* stream) { return cg_mix(h_mix, true, stream); }
extern "C" int tzr_cgc_mix_bwd(const TzrCgcMix* h_mix, void* stream) { return cg_mix(h_mix, false, stream); }
