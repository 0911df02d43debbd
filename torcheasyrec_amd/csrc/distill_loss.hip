// Rocket Launching's distillation terms (tzrec/models/rocket_launching.py:125-204): every similarity term of a step and the hint
// loss in one launch.  P layer pairs (light_p, booster_p) [B, W_p], logits_light / logits_booster [B, C], weights w [B] or none.
//   lw_b = w_b / mean(w) (0 when mean(w) is 0: div_no_nan), 1 without weights
//   COSINE:   sim_p = -0.1 mean_b(lw_b <l / max(|l|, 1e-12), t / max(|t|, 1e-12)>)        (l = light_p[b], t = booster_p[b])
//   distance: sim_p = sqrt(sum_b lw_b |t - l|^2)                                            (a root of a sum, not a mean)
//   hint = sum_b lw_b sum_c (ll_bc - lb_bc)^2 / (B C)
//   backward, into light_p and logits_light alone (every booster operand is a constant):
//   COSINE:   dy = k t / max(|t|, 1e-12), k = g_p (-0.1 / B) lw_b;  dl = (dy - y <y, dy>) / n where n = |l| >= 1e-12, dy / 1e-12
//             below (torch's clamp branch);  distance: dl = g_p lw_b (l - t) / sim_p;  hint: dll = g_h lw_b 2 (ll - lb) / (B C)
//   Distance mode with a total of exactly 0: the literal form's gradient is NaN (0 * inf); the rows written here are zeros.
// One wave per sample, four samples a workgroup; the wave walks its pairs one after the other, lane l holding the float4 at
// columns 256 j + 4 l of the row (W <= 1024: up to four a lane): rows of 32 or 64 floats leave lanes idle, which costs nothing
// where the launch itself is the price.  Dots by the fixed xor tree; the forward leaves one partial row (sum q_p w for every
// pair, sum h w, sum w) per workgroup and a finishing launch adds them in the interleaved order (parts_sum.h).  Nothing is saved
// per sample: the backward reads the rows again anyway and recomputes their norms; what it keeps is 1 + P floats (B / sum(w), and
// 1 / sim_p under distance).  One launch and a finishing one forward, one launch backward; no atomics: two runs are bit-equal.
#include "tzr_common.h"
#include "parts_sum.h"

#define DST_THREADS 256
#define DST_WAVES (DST_THREADS / TZR_WAVE)
#define DST_MAXP TZR_DISTILL_MAX_PAIRS
#define DST_MAXW TZR_DISTILL_MAX_W
#define DST_MAXC 64
#define DST_COLS (DST_MAXP + 2)
#define DST_EPS 1e-12f
#define DST_STEP (4 * TZR_WAVE)

static_assert(DST_MAXC <= TZR_WAVE, "one logit a lane");
static_assert(DST_COLS <= TZR_WAVE, "one finishing workgroup");

struct DistillArgs {
  const float* l[DST_MAXP];
  const float* t[DST_MAXP];
  int64_t ls[DST_MAXP], ts[DST_MAXP];
  int W[DST_MAXP];
  const float* g[DST_MAXP];
  float* dl[DST_MAXP];
  int64_t dls[DST_MAXP];
  const float *ll, *lb, *w, *gh;
  float* dll;
  int64_t B;
  int P, C, cosine;
  float *loss, *scale, *parts;
};

__device__ __forceinline__ float dst_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// grid ceil(B / 4).  parts [G, P + 2]: sum_b q_p w (q: the cosine of the two rows, or |t - l|^2), sum_b h w, sum_b w
__global__ __launch_bounds__(DST_THREADS) void tzr_distill_loss_fwd_kernel(DistillArgs A) {
  __shared__ float sm[DST_WAVES][DST_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * DST_WAVES + wave;
  const bool rok = b < A.B;  // (a whole wave)
  const float wb = rok ? (A.w ? A.w[b] : 1.0f) : 0.f;
  for (int p = 0; p < A.P; ++p) {
    float q = 0.f;
    if (rok) {
      const int W = A.W[p];
      const float* lr = A.l[p] + b * A.ls[p];
      const float* tr = A.t[p] + b * A.ts[p];
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int c0 = 0; c0 < W; c0 += DST_STEP) {  // (the same trips for every lane)
        const int c = c0 + 4 * lane;
        const float4 x = c < W ? tzr_ld4(lr + c) : tzr_zero4();
        const float4 y = c < W ? tzr_ld4(tr + c) : tzr_zero4();
        if (A.cosine) {
          s0 += dst_dot4(x, x), s1 += dst_dot4(y, y), s2 += dst_dot4(x, y);
        } else {
          const float4 d = make_float4(y.x - x.x, y.y - x.y, y.z - x.z, y.w - x.w);
          s0 += dst_dot4(d, d);
        }
      }
      if (A.cosine) {
        const float rl = 1.0f / fmaxf(sqrtf(tzr_wave_sum(s0)), DST_EPS), rt = 1.0f / fmaxf(sqrtf(tzr_wave_sum(s1)), DST_EPS);
        q = tzr_wave_sum(s2) * rl * rt;
      } else {
        q = tzr_wave_sum(s0);
      }
    }
    if (lane == 0) sm[wave][p] = q * wb;
  }
  float h = 0.f;
  if (rok) {
    float d = 0.f;
    if (lane < A.C) d = A.ll[b * A.C + lane] - A.lb[b * A.C + lane];
    h = tzr_wave_sum(d * d);
  }
  if (lane == 0) sm[wave][A.P] = h * wb, sm[wave][A.P + 1] = wb;
  __syncthreads();
  const int N = A.P + 2;
  if ((int)threadIdx.x < N) {
    float s = 0.f;
    for (int k = 0; k < DST_WAVES; ++k) s += sm[k][threadIdx.x];
    A.parts[(int64_t)N * blockIdx.x + threadIdx.x] = s;
  }
}

// one workgroup: the P + 1 losses from the column totals; scale[0] = B / sum(w) (0 when the weights add to 0, 1 without
// weights), scale[1 + p] = 1 / sim_p under distance (0 where sim_p is 0), else 0
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_distill_loss_finish_kernel(const float* __restrict__ parts, int G, int P, int has_w, int cosine,
                                                                                  float fB, float fBC, float* __restrict__ loss,
                                                                                  float* __restrict__ scale) {
  __shared__ float red[TZR_FIN_THREADS];
  __shared__ float tot[DST_COLS];
  const int N = P + 2;
  const int col = threadIdx.x & (TZR_WAVE - 1);
  const float r = tzr_parts_sum_interleaved(col < N ? parts + col : nullptr, G, (size_t)N, red);
  if ((int)threadIdx.x < N) tot[threadIdx.x] = r;
  __syncthreads();
  if ((int)threadIdx.x <= P) {
    const float sw = tot[P + 1];
    const float inv = has_w ? (sw != 0.f ? fB / sw : 0.f) : 1.0f;  // lw_b = w_b inv (div_no_nan)
    const int p = threadIdx.x;
    if (p == P) {
      loss[P] = tot[P] * inv / fBC;
      scale[0] = inv;
    } else if (cosine) {
      loss[p] = -0.1f * (tot[p] * inv / fB);
      scale[1 + p] = 0.f;
    } else {
      const float s = sqrtf(tot[p] * inv);
      loss[p] = s;
      scale[1 + p] = s > 0.f ? 1.0f / s : 0.f;
    }
  }
}

// grid ceil(B / 4).  A pair without dl is skipped; a pair without g gets zero rows.
__global__ __launch_bounds__(DST_THREADS) void tzr_distill_loss_bwd_kernel(DistillArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * DST_WAVES + (threadIdx.x >> 6);
  if (b >= A.B) return;  // (a whole wave)
  const float lw = A.w ? A.w[b] * A.scale[0] : 1.0f;
  for (int p = 0; p < A.P; ++p) {
    float* dr = A.dl[p];
    if (!dr) continue;
    dr += b * A.dls[p];
    const int W = A.W[p];
    const float g = A.g[p] ? A.g[p][0] : 0.f;
    const float* lr = A.l[p] + b * A.ls[p];
    const float* tr = A.t[p] + b * A.ts[p];
    if (A.cosine) {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int c0 = 0; c0 < W; c0 += DST_STEP) {
        const int c = c0 + 4 * lane;
        const float4 x = c < W ? tzr_ld4(lr + c) : tzr_zero4();
        const float4 y = c < W ? tzr_ld4(tr + c) : tzr_zero4();
        s0 += dst_dot4(x, x), s1 += dst_dot4(y, y), s2 += dst_dot4(x, y);
      }
      const float nl = sqrtf(tzr_wave_sum(s0));
      const float rl = 1.0f / fmaxf(nl, DST_EPS), rt = 1.0f / fmaxf(sqrtf(tzr_wave_sum(s1)), DST_EPS);
      const float k = g * (-0.1f / (float)A.B) * lw * rt;  // dy = k t
      // <y, dy> = k rl <l, t>; the clamp branch passes nothing through the norm
      const float pr = nl >= DST_EPS ? k * rl * tzr_wave_sum(s2) : 0.f;
      for (int c0 = 0; c0 < W; c0 += DST_STEP) {
        const int c = c0 + 4 * lane;
        if (c < W) {
          const float4 x = tzr_ld4(lr + c), y = tzr_ld4(tr + c);
          tzr_st4(dr + c, make_float4((k * y.x - x.x * rl * pr) * rl, (k * y.y - x.y * rl * pr) * rl, (k * y.z - x.z * rl * pr) * rl,
                                      (k * y.w - x.w * rl * pr) * rl));
        }
      }
    } else {
      const float k = g * lw * A.scale[1 + p];
      for (int c0 = 0; c0 < W; c0 += DST_STEP) {
        const int c = c0 + 4 * lane;
        if (c < W) {
          const float4 x = tzr_ld4(lr + c), y = tzr_ld4(tr + c);
          tzr_st4(dr + c, make_float4(k * (x.x - y.x), k * (x.y - y.y), k * (x.z - y.z), k * (x.w - y.w)));
        }
      }
    }
  }
  if (A.dll && lane < A.C) {
    const float k = (A.gh ? A.gh[0] : 0.f) * lw * (2.0f / ((float)A.B * (float)A.C));
    A.dll[b * A.C + lane] = k * (A.ll[b * A.C + lane] - A.lb[b * A.C + lane]);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static inline int64_t dst_blocks(int64_t rows) { return (rows + DST_WAVES - 1) / DST_WAVES; }

// limits first, then pointers
static int dst_check(const TzrDistillLoss* m, DistillArgs* A) {
  if (m->B < 0) return TZR_ERR_INVALID;
  if (m->P < 0 || m->P > DST_MAXP || m->C < 1 || m->C > DST_MAXC || m->B >= (1ll << 31)) return TZR_ERR_UNSUPPORTED;
  if (m->cosine != 0 && m->cosine != 1) return TZR_ERR_UNSUPPORTED;
  for (int p = 0; p < m->P; ++p)
    if (m->W[p] < 4 || (m->W[p] & 3) || m->W[p] > DST_MAXW) return TZR_ERR_UNSUPPORTED;
  for (int p = 0; p < m->P; ++p) {
    TZR_TRY(tzr_rows_operand(m->light[p], m->light_stride[p], m->W[p]));
    TZR_TRY(tzr_rows_operand(m->booster[p], m->booster_stride[p], m->W[p]));
  }
  if (!m->logits_light || !m->logits_booster || !m->scale) return TZR_ERR_INVALID;
  if ((m->logits_light & 3) || (m->logits_booster & 3) || (m->w & 3) || (m->scale & 3)) return TZR_ERR_INVALID;
  for (int p = 0; p < m->P; ++p) {
    A->l[p] = reinterpret_cast<const float*>(m->light[p]);
    A->t[p] = reinterpret_cast<const float*>(m->booster[p]);
    A->ls[p] = m->light_stride[p], A->ts[p] = m->booster_stride[p], A->W[p] = m->W[p];
  }
  A->ll = reinterpret_cast<const float*>(m->logits_light);
  A->lb = reinterpret_cast<const float*>(m->logits_booster);
  A->w = reinterpret_cast<const float*>(m->w);
  A->B = m->B, A->P = m->P, A->C = m->C, A->cosine = m->cosine;
  A->scale = reinterpret_cast<float*>(m->scale);
  return TZR_OK;
}

extern "C" size_t tzr_distill_loss_workspace(const TzrDistillLoss* h_dst) {
  if (!h_dst || h_dst->B < 1 || h_dst->P < 0 || h_dst->P > DST_MAXP) return 256;
  return tzr_align_up((size_t)dst_blocks(h_dst->B) * (h_dst->P + 2) * sizeof(float)) + 256;
}

extern "C" int tzr_distill_loss_fwd(const TzrDistillLoss* h_dst, void* stream) {
  if (!h_dst) return TZR_ERR_INVALID;
  DistillArgs A = {};
  TZR_TRY(dst_check(h_dst, &A));
  if (!h_dst->loss || (h_dst->loss & 3)) return TZR_ERR_INVALID;
  const int64_t G = dst_blocks(h_dst->B);
  if (!h_dst->ws || (h_dst->ws & 255) || h_dst->ws_bytes < tzr_align_up((size_t)G * (h_dst->P + 2) * sizeof(float))) return TZR_ERR_WORKSPACE;
  if (h_dst->B == 0) return TZR_OK;
  A.loss = reinterpret_cast<float*>(h_dst->loss);
  A.parts = reinterpret_cast<float*>(h_dst->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tzr_distill_loss_fwd_kernel, dim3((unsigned)G), dim3(DST_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_distill_loss_finish_kernel, dim3(1), dim3(TZR_FIN_THREADS), 0, s, A.parts, (int)G, A.P, A.w ? 1 : 0, A.cosine,
                     (float)A.B, (float)A.B * (float)A.C, A.loss, A.scale);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_distill_loss_bwd(const TzrDistillLoss* h_dst, void* stream) {
  if (!h_dst) return TZR_ERR_INVALID;
  DistillArgs A = {};
  TZR_TRY(dst_check(h_dst, &A));
  if ((h_dst->grad_hint & 3) || (h_dst->dlogits_light & 3)) return TZR_ERR_INVALID;
  for (int p = 0; p < h_dst->P; ++p) {
    if (h_dst->grad_sim[p] & 3) return TZR_ERR_INVALID;
    if (h_dst->dlight[p]) TZR_TRY(tzr_rows_operand(h_dst->dlight[p], h_dst->dlight_stride[p], h_dst->W[p]));
  }
  if (h_dst->B == 0) return TZR_OK;
  for (int p = 0; p < h_dst->P; ++p) {
    A.g[p] = reinterpret_cast<const float*>(h_dst->grad_sim[p]);
    A.dl[p] = reinterpret_cast<float*>(h_dst->dlight[p]);
    A.dls[p] = h_dst->dlight_stride[p];
  }
  A.gh = reinterpret_cast<const float*>(h_dst->grad_hint);
  A.dll = reinterpret_cast<float*>(h_dst->dlogits_light);
  hipLaunchKernelGGL(tzr_distill_loss_bwd_kernel, dim3((unsigned)dst_blocks(h_dst->B)), dim3(DST_THREADS), 0, static_cast<hipStream_t>(stream), A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
