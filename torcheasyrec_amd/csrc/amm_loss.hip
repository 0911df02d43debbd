// DAT's Adaptive-Mimic loss (tzrec/models/dat.py:212-259), both sides in one launch.  Per side s in {u, i} and sample b < B:
//   a = row b of that side's augment rows, t = row b of the OTHER tower's embedding (a constant: no gradient)
//   n = max(|a|, 1e-12), y = a / n;  tau = t / max(|t|, 1e-12) under COSINE, else t;  l_b = sum_d (y_d - tau_d)^2
//   loss_s = c_s sum_b l_b, or with weights c_s sum_b(l_b w_b) / sum_b(w_b) (0 when the weights add to 0: div_no_nan)
//   backward:  k_b = g_s c_s (with weights: g_s c_s w_b / sum(w), 0 when that sum is 0);  dy = 2 k_b (y - tau);
//   da = (dy - y <y, dy>) / n where |a| >= 1e-12, dy / 1e-12 below (torch's clamp branch);  rows b >= B of the item side: zeros
// One wave per sample handles both sides, four samples a workgroup; lane l holds the float4 at columns 4 l of every row (D <=
// 256).  Dots by the fixed xor tree; the forward leaves one partial row (sum l_u w, sum l_i w, sum w) per workgroup and a finishing
// launch adds them in the interleaved order (parts_sum.h).  One launch and a finishing one forward, one launch backward; no
// atomics: two runs are bit-equal.
#include "tzr_common.h"
#include "parts_sum.h"

#define AMM_THREADS 256
#define AMM_WAVES (AMM_THREADS / TZR_WAVE)
#define AMM_MAXD TZR_AMM_MAX_D
#define AMM_EPS 1e-12f

static_assert(AMM_MAXD <= 4 * TZR_WAVE, "one float4 a lane");

struct AmmArgs {
  const float *ua, *ia, *ue, *ie, *w;
  int64_t uas, ias, ues, ies, B, M;
  int D, cosine;
  float cu, ci;
  float *loss, *rows, *scale, *parts;
  const float *gu, *gi;
  float *dua, *dia;
  int64_t duas, dias;
};

__device__ __forceinline__ float amm_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 amm_diff(float4 a, float ra, float4 t, float rt) {
  return make_float4(a.x * ra - t.x * rt, a.y * ra - t.y * rt, a.z * ra - t.z * rt, a.w * ra - t.w * rt);
}

// one side of one sample in the forward: -> l_b; *rn = 1 / n, NEGATED where |a| < 1e-12 (the backward's clamp branch), *rt = 1 /
// max(|t|, 1e-12) under COSINE, else 1
__device__ __forceinline__ float amm_side_fwd(float4 a, float4 t, int cosine, float* rn, float* rt) {
  const float na = sqrtf(tzr_wave_sum(amm_dot4(a, a)));
  const float ra = 1.0f / fmaxf(na, AMM_EPS);
  const float r = cosine ? 1.0f / fmaxf(sqrtf(tzr_wave_sum(amm_dot4(t, t))), AMM_EPS) : 1.0f;
  const float4 d = amm_diff(a, ra, t, r);
  *rn = na >= AMM_EPS ? ra : -ra;
  *rt = r;
  return tzr_wave_sum(amm_dot4(d, d));
}

// grid ceil(B / 4).  rows [6, B]: l_u, l_i, 1/n_u, 1/n_i, 1/|t| of the user side's target, of the item side's
__global__ __launch_bounds__(AMM_THREADS) void tzr_amm_loss_fwd_kernel(AmmArgs A) {
  __shared__ float sm[AMM_WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * AMM_WAVES + wave;
  const bool rok = b < A.B;  // (a whole wave)
  const bool cok = rok && 4 * lane < A.D;
  float lu = 0.f, li = 0.f, wb = 0.f;
  if (rok) {
    const float4 au = cok ? tzr_ld4(A.ua + b * A.uas + 4 * lane) : tzr_zero4();
    const float4 ai = cok ? tzr_ld4(A.ia + b * A.ias + 4 * lane) : tzr_zero4();
    const float4 eu = cok ? tzr_ld4(A.ue + b * A.ues + 4 * lane) : tzr_zero4();
    const float4 ei = cok ? tzr_ld4(A.ie + b * A.ies + 4 * lane) : tzr_zero4();
    float rnu, rtu, rni, rti;
    lu = amm_side_fwd(au, ei, A.cosine, &rnu, &rtu);
    li = amm_side_fwd(ai, eu, A.cosine, &rni, &rti);
    if (lane == 0) {
      float* r = A.rows + b;
      r[0] = lu, r[A.B] = li, r[2 * A.B] = rnu, r[3 * A.B] = rni, r[4 * A.B] = rtu, r[5 * A.B] = rti;
    }
    wb = A.w ? A.w[b] : 1.0f;
  }
  if (lane == 0) sm[wave][0] = lu * wb, sm[wave][1] = li * wb, sm[wave][2] = wb;
  __syncthreads();
  if (threadIdx.x < 3) {
    float s = 0.f;
    for (int k = 0; k < AMM_WAVES; ++k) s += sm[k][threadIdx.x];
    A.parts[3 * (int64_t)blockIdx.x + threadIdx.x] = s;
  }
}

// one workgroup: loss_s = c_s sum(l_s w) / sum(w) (0 when the weights add to 0) or c_s sum(l_s); scale = the reciprocal the backward needs
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_amm_loss_finish_kernel(const float* __restrict__ parts, int G, int has_w, float cu, float ci,
                                                                              float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ float red[TZR_FIN_THREADS];
  __shared__ float tot[3];
  const int col = threadIdx.x & (TZR_WAVE - 1);
  const float r = tzr_parts_sum_interleaved(col < 3 ? parts + col : nullptr, G, 3, red);
  if (threadIdx.x < 3) tot[threadIdx.x] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool ok = !has_w || tot[2] != 0.f;  // div_no_nan
    const float inv = has_w ? (ok ? 1.0f / tot[2] : 0.f) : 1.0f;
    loss[0] = ok ? cu * (has_w ? tot[0] / tot[2] : tot[0]) : 0.f;
    loss[1] = ok ? ci * (has_w ? tot[1] / tot[2] : tot[1]) : 0.f;
    *scale = inv;
  }
}

// one side of one sample in the backward: k = k_b, rn / rt as the forward saved them
__device__ __forceinline__ float4 amm_side_bwd(float4 a, float4 t, float k, float rn, float rt) {
  const float ra = fabsf(rn);
  const float4 y = make_float4(a.x * ra, a.y * ra, a.z * ra, a.w * ra);
  const float k2 = 2.0f * k;
  const float4 dy = make_float4(k2 * (y.x - t.x * rt), k2 * (y.y - t.y * rt), k2 * (y.z - t.z * rt), k2 * (y.w - t.w * rt));
  const float yd = tzr_wave_sum(amm_dot4(y, dy));
  const float p = rn > 0.f ? yd : 0.f;  // (the clamp branch passes nothing through the norm)
  return make_float4((dy.x - y.x * p) * ra, (dy.y - y.y * p) * ra, (dy.z - y.z * p) * ra, (dy.w - y.w * p) * ra);
}

// grid ceil(M / 4): row r < B both sides, row B <= r < M zeros into the item side's gradient
__global__ __launch_bounds__(AMM_THREADS) void tzr_amm_loss_bwd_kernel(AmmArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * AMM_WAVES + (threadIdx.x >> 6);
  if (b >= A.M) return;  // (a whole wave)
  const bool cok = 4 * lane < A.D;
  if (b >= A.B) {
    if (cok) tzr_st4(A.dia + b * A.dias + 4 * lane, tzr_zero4());
    return;
  }
  const float4 au = cok ? tzr_ld4(A.ua + b * A.uas + 4 * lane) : tzr_zero4();
  const float4 ai = cok ? tzr_ld4(A.ia + b * A.ias + 4 * lane) : tzr_zero4();
  const float4 eu = cok ? tzr_ld4(A.ue + b * A.ues + 4 * lane) : tzr_zero4();
  const float4 ei = cok ? tzr_ld4(A.ie + b * A.ies + 4 * lane) : tzr_zero4();
  const float* r = A.rows + b;
  const float wk = A.w ? A.w[b] * A.scale[0] : 1.0f;
  const float ku = (A.gu ? A.gu[0] : 0.f) * A.cu * wk, ki = (A.gi ? A.gi[0] : 0.f) * A.ci * wk;
  const float4 du = amm_side_bwd(au, ei, ku, r[2 * A.B], r[4 * A.B]);
  const float4 di = amm_side_bwd(ai, eu, ki, r[3 * A.B], r[5 * A.B]);
  if (cok) {
    tzr_st4(A.dua + b * A.duas + 4 * lane, du);
    tzr_st4(A.dia + b * A.dias + 4 * lane, di);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static inline int64_t amm_blocks(int64_t rows) { return (rows + AMM_WAVES - 1) / AMM_WAVES; }

// limits first, then pointers
static int amm_check(const TzrAmmLoss* m, AmmArgs* A) {
  if (m->B < 0) return TZR_ERR_INVALID;
  if (m->D < 4 || (m->D & 3) || m->D > AMM_MAXD || m->M < m->B || m->B >= (1ll << 31) || m->M >= (1ll << 31)) return TZR_ERR_UNSUPPORTED;
  if (m->cosine != 0 && m->cosine != 1) return TZR_ERR_UNSUPPORTED;
  TZR_TRY(tzr_rows_operand(m->ua, m->ua_stride, m->D));
  TZR_TRY(tzr_rows_operand(m->ia, m->ia_stride, m->D));
  TZR_TRY(tzr_rows_operand(m->ue, m->ue_stride, m->D));
  TZR_TRY(tzr_rows_operand(m->ie, m->ie_stride, m->D));
  if (!m->rows || !m->scale || (m->w & 3) || (m->rows & 3) || (m->scale & 3)) return TZR_ERR_INVALID;
  A->ua = reinterpret_cast<const float*>(m->ua);
  A->ia = reinterpret_cast<const float*>(m->ia);
  A->ue = reinterpret_cast<const float*>(m->ue);
  A->ie = reinterpret_cast<const float*>(m->ie);
  A->w = reinterpret_cast<const float*>(m->w);
  A->uas = m->ua_stride, A->ias = m->ia_stride, A->ues = m->ue_stride, A->ies = m->ie_stride;
  A->B = m->B, A->M = m->M, A->D = m->D, A->cosine = m->cosine, A->cu = m->c_u, A->ci = m->c_i;
  A->rows = reinterpret_cast<float*>(m->rows);
  A->scale = reinterpret_cast<float*>(m->scale);
  return TZR_OK;
}

extern "C" size_t tzr_amm_loss_workspace(const TzrAmmLoss* h_amm) {
  if (!h_amm || h_amm->B < 1) return 256;
  return tzr_align_up((size_t)amm_blocks(h_amm->B) * 3 * sizeof(float)) + 256;
}

extern "C" int tzr_amm_loss_fwd(const TzrAmmLoss* h_amm, void* stream) {
  if (!h_amm) return TZR_ERR_INVALID;
  AmmArgs A = {};
  TZR_TRY(amm_check(h_amm, &A));
  if (!h_amm->loss || (h_amm->loss & 3)) return TZR_ERR_INVALID;
  const int64_t G = amm_blocks(h_amm->B);
  if (!h_amm->ws || (h_amm->ws & 255) || h_amm->ws_bytes < tzr_align_up((size_t)G * 3 * sizeof(float))) return TZR_ERR_WORKSPACE;
  if (h_amm->B == 0) return TZR_OK;
  A.loss = reinterpret_cast<float*>(h_amm->loss);
  A.parts = reinterpret_cast<float*>(h_amm->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tzr_amm_loss_fwd_kernel, dim3((unsigned)G), dim3(AMM_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_amm_loss_finish_kernel, dim3(1), dim3(TZR_FIN_THREADS), 0, s, A.parts, (int)G, A.w ? 1 : 0, A.cu, A.ci, A.loss, A.scale);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_amm_loss_bwd(const TzrAmmLoss* h_amm, void* stream) {
  if (!h_amm) return TZR_ERR_INVALID;
  AmmArgs A = {};
  TZR_TRY(amm_check(h_amm, &A));
  if ((h_amm->grad_u & 3) || (h_amm->grad_i & 3)) return TZR_ERR_INVALID;
  TZR_TRY(tzr_rows_operand(h_amm->dua, h_amm->dua_stride, h_amm->D));
  TZR_TRY(tzr_rows_operand(h_amm->dia, h_amm->dia_stride, h_amm->D));
  if (h_amm->B == 0) return TZR_OK;
  A.gu = reinterpret_cast<const float*>(h_amm->grad_u);
  A.gi = reinterpret_cast<const float*>(h_amm->grad_i);
  A.dua = reinterpret_cast<float*>(h_amm->dua);
  A.dia = reinterpret_cast<float*>(h_amm->dia);
  A.duas = h_amm->dua_stride, A.dias = h_amm->dia_stride;
  hipLaunchKernelGGL(tzr_amm_loss_bwd_kernel, dim3((unsigned)amm_blocks(h_amm->M)), dim3(AMM_THREADS), 0, static_cast<hipStream_t>(stream), A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
