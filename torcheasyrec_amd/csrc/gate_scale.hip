// The gate-and-scale step of PEPNet (tzrec/modules/personalized_net.py): every task of one PPNet level computes
//
//     out_n[b, :] = act(z_n[b, :] + bz_n) * gamma * sigmoid(g_n[b, :] + bg_n)
//
// with z_n = x W_n^T the task's Linear layer and g_n = relu(gate_input Wa_n^T + ba_n) Wb_n^T the second layer of its gate unit,
// both WITHOUT their bias (the kernel owns the two bias adds); EPNet is the same expression with act = identity, z the main
// embedding itself and no bz.  As torch ops that is two bias adds, a ReLU, a sigmoid, a scale and a multiply forward (about 4
// launches per task and level) and 6 to 8 backward, the two bias gradients among them as column reductions that re-read what
// was just written.  Here: ONE launch per direction for every slot (task) of the level, plus one finishing launch that adds the
// workgroups' partial bias-gradient rows in the interleaved order of parts_sum.h.  Nothing is kept from the forward but its
// inputs z and g: the backward recomputes the sigmoid and -- with the forward's own fp32 add -- the ReLU mask.
//
// Mapping: grid (row chunks, slots), 256 threads.  CW = min(H / 4, 256) float4 columns are swept at a time by rl = 256 / CW row
// lanes; a thread keeps its column over all rows of its workgroup's chunk, GS_UNROLL rows loaded before any is used, so the two
// bias sums of the column stay in registers.  The row lanes' sums are added through LDS in row-lane order, the workgroup's row
// of partial sums is [slot 0: dbz | dbg] [slot 1: dbz | dbg] ...  No atomics: every addition has a fixed place.
// The sigmoid: e = exp(-|x|) lies in [0, 1], r = 1 / (1 + e) in [1/2, 1]; s = r (x >= 0) or e r (x < 0), s (1 - s) = e r r --
// no overflow, no NaN or Inf for any finite x, and no cancellation: 1 - s is never formed as a difference (as `1 - s` in fp32 it
// loses every digit once s is within 2^-24 of 1, an absolute error of 6e-8 |dout act(z) gamma| in dg).  An e below the smallest
// normal fp32 (|x| > 87.3) counts as 0: there s is exactly 0 or 1 and s (1 - s) exactly 0 -- saturation, with or without
// subnormal support in exp.
#include "parts_sum.h"
#include "tzr_common.h"

#define GS_THREADS 256
#define GS_N TZR_GATE_SCALE_MAX_SLOTS
#define GS_UNROLL 4
#define GS_MAX_WG 512  // row chunks; times the slots: workgroups

static_assert(sizeof(TzrGateScale) == 952, "TzrGateScale: the layout _lib.py mirrors");

struct GsArgs {
  const float* z[GS_N];
  int64_t z_stride[GS_N];
  const float* bz[GS_N];  // null: no bias
  const float* g[GS_N];
  int64_t g_stride[GS_N];
  const float* bg[GS_N];
  float* out[GS_N];  // forward
  int64_t out_stride[GS_N];
  const float* go[GS_N];  // backward: d(loss)/d(out_n); null: none, the slot's gradients are zeros
  int64_t go_stride[GS_N];
  float* dz[GS_N];  // may be z itself (a thread reads an element before it writes it, and no other thread touches it)
  int64_t dz_stride[GS_N];
  float* dg[GS_N];  // may be g itself
  int64_t dg_stride[GS_N];
};

// s = sigmoid(x); *sq = s (1 - s)
__device__ __forceinline__ float gs_sigmoid(float x, float* sq) {
  float e = expf(-fabsf(x));
  if (e < 1.17549435e-38f) e = 0.f;
  const float r = 1.0f / (1.0f + e);
  const float er = e * r;
  *sq = er * r;
  return x >= 0.f ? r : er;
}
__device__ __forceinline__ float gs_sigmoid(float x) {
  float sq;
  return gs_sigmoid(x, &sq);
}

struct GsGeometry {
  int CW;               // float4 columns per sweep
  int rl;               // row lanes
  int64_t rows_per_wg;  // a multiple of rl * GS_UNROLL
  int64_t n_wg;         // row chunks
};

static GsGeometry gs_geometry(int64_t B, int H) {
  GsGeometry q;
  q.CW = std::min(H >> 2, GS_THREADS);
  q.rl = GS_THREADS / q.CW;
  const int64_t unit = (int64_t)q.rl * GS_UNROLL;
  q.rows_per_wg = unit;
  q.n_wg = (B + unit - 1) / unit;
  if (q.n_wg > GS_MAX_WG) {
    q.rows_per_wg = ((B + GS_MAX_WG - 1) / GS_MAX_WG + unit - 1) / unit * unit;
    q.n_wg = (B + q.rows_per_wg - 1) / q.rows_per_wg;
  }
  return q;
}

template <bool RELU>
__global__ __launch_bounds__(GS_THREADS) void tzr_gate_scale_fwd_kernel(GsArgs A, int64_t B, int H, int64_t rows_per_wg, int CW,
                                                                        float gamma) {
  const int n = blockIdx.y;
  const int N4 = H >> 2;
  const int rl = GS_THREADS / CW;
  const int c = threadIdx.x % CW, r = threadIdx.x / CW;
  const int64_t lo = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t hi = min(B, lo + rows_per_wg);
  const float* z = A.z[n];
  const float* g = A.g[n];
  const float* bz = A.bz[n];
  const float* bg = A.bg[n];
  float* out = A.out[n];
  const int64_t zs = A.z_stride[n], gs = A.g_stride[n], os = A.out_stride[n];
  if (r >= rl) return;
  for (int cc = c; cc < N4; cc += CW) {
    const float4 vbz = bz ? tzr_ld4(bz + 4 * cc) : tzr_zero4();
    const float4 vbg = tzr_ld4(bg + 4 * cc);
    for (int64_t b0 = lo + r; b0 < hi; b0 += (int64_t)rl * GS_UNROLL) {
      float4 vz[GS_UNROLL], vg[GS_UNROLL];
#pragma unroll
      for (int u = 0; u < GS_UNROLL; ++u) {
        const int64_t b = b0 + (int64_t)u * rl;
        vz[u] = b < hi ? tzr_ld4(z + b * zs + 4 * cc) : tzr_zero4();
        vg[u] = b < hi ? tzr_ld4(g + b * gs + 4 * cc) : tzr_zero4();
      }
#pragma unroll
      for (int u = 0; u < GS_UNROLL; ++u) {
        const int64_t b = b0 + (int64_t)u * rl;
        if (b >= hi) continue;
        float4 a = tzr_add4(vz[u], vbz);
        if (RELU) a = make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f));
        const float4 t = tzr_add4(vg[u], vbg);
        float4 o;
        o.x = a.x * (gamma * gs_sigmoid(t.x));
        o.y = a.y * (gamma * gs_sigmoid(t.y));
        o.z = a.z * (gamma * gs_sigmoid(t.z));
        o.w = a.w * (gamma * gs_sigmoid(t.w));
        tzr_st4(out + b * os + 4 * cc, o);
      }
    }
  }
}

// one element: dz = go * gamma * s * [a > 0] (identity: no mask), dg = go * act(a) * gamma * s * (1 - s); a = z + bz, t = g + bg
template <bool RELU>
__device__ __forceinline__ void gs_bwd1(float go, float a, float t, float gamma, float* dz, float* dg) {
  float sq;
  const float s = gs_sigmoid(t, &sq);
  const bool on = !RELU || a > 0.f;  // (a == 0: no gradient, as threshold_backward)
  *dz = on ? go * (gamma * s) : 0.f;
  *dg = on ? (go * a) * (gamma * sq) : 0.f;
}

template <bool RELU>
__global__ __launch_bounds__(GS_THREADS) void tzr_gate_scale_bwd_kernel(GsArgs A, int64_t B, int H, int64_t rows_per_wg, int CW,
                                                                        float gamma, float* parts, int P) {
  __shared__ float4 red[2 * GS_THREADS];
  const int n = blockIdx.y;
  const int N4 = H >> 2;
  const int rl = GS_THREADS / CW;
  const int c = threadIdx.x % CW, r = threadIdx.x / CW;
  const int64_t lo = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t hi = min(B, lo + rows_per_wg);
  const float* z = A.z[n];
  const float* g = A.g[n];
  const float* go = A.go[n];
  const float* bz = A.bz[n];
  const float* bg = A.bg[n];
  float* dz = A.dz[n];
  float* dg = A.dg[n];
  const int64_t zs = A.z_stride[n], gs = A.g_stride[n], gos = A.go_stride[n], dzs = A.dz_stride[n], dgs = A.dg_stride[n];
  float* my_parts = parts + (size_t)blockIdx.x * P + (size_t)n * 2 * H;
  // (c0, CW, N4 are uniform: every thread of the workgroup reaches both barriers of every sweep)
  for (int c0 = 0; c0 < N4; c0 += CW) {
    const int cc = c0 + c;
    const bool on = r < rl && cc < N4;
    float4 az = tzr_zero4(), ag = tzr_zero4();
    if (on && go) {
      const float4 vbz = bz ? tzr_ld4(bz + 4 * cc) : tzr_zero4();
      const float4 vbg = tzr_ld4(bg + 4 * cc);
      for (int64_t b0 = lo + r; b0 < hi; b0 += (int64_t)rl * GS_UNROLL) {
        float4 vz[GS_UNROLL], vg[GS_UNROLL], vo[GS_UNROLL];
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
          const int64_t b = b0 + (int64_t)u * rl;
          vz[u] = b < hi ? tzr_ld4(z + b * zs + 4 * cc) : tzr_zero4();
          vg[u] = b < hi ? tzr_ld4(g + b * gs + 4 * cc) : tzr_zero4();
          vo[u] = b < hi ? tzr_ld4(go + b * gos + 4 * cc) : tzr_zero4();
        }
#pragma unroll
        for (int u = 0; u < GS_UNROLL; ++u) {
          const int64_t b = b0 + (int64_t)u * rl;
          if (b >= hi) continue;
          const float4 a = tzr_add4(vz[u], vbz);
          const float4 t = tzr_add4(vg[u], vbg);
          float4 oz, og;
          gs_bwd1<RELU>(vo[u].x, a.x, t.x, gamma, &oz.x, &og.x);
          gs_bwd1<RELU>(vo[u].y, a.y, t.y, gamma, &oz.y, &og.y);
          gs_bwd1<RELU>(vo[u].z, a.z, t.z, gamma, &oz.z, &og.z);
          gs_bwd1<RELU>(vo[u].w, a.w, t.w, gamma, &oz.w, &og.w);
          tzr_st4(dz + b * dzs + 4 * cc, oz);
          tzr_st4(dg + b * dgs + 4 * cc, og);
          az = tzr_add4(az, oz);
          ag = tzr_add4(ag, og);
        }
      }
    } else if (on) {  // a slot without an output gradient: zeros everywhere
      for (int64_t b = lo + r; b < hi; b += rl) {
        tzr_st4(dz + b * dzs + 4 * cc, tzr_zero4());
        tzr_st4(dg + b * dgs + 4 * cc, tzr_zero4());
      }
    }
    red[threadIdx.x] = az;
    red[GS_THREADS + threadIdx.x] = ag;
    __syncthreads();
    if (r == 0 && cc < N4) {  // fixed order over the row lanes
      float4 tz = red[c], tg = red[GS_THREADS + c];
      for (int k = 1; k < rl; ++k) {
        tz = tzr_add4(tz, red[k * CW + c]);
        tg = tzr_add4(tg, red[GS_THREADS + k * CW + c]);
      }
      tzr_st4(my_parts + 4 * cc, tz);
      tzr_st4(my_parts + H + 4 * cc, tg);
    }
    __syncthreads();
  }
}

// sizes, limits, z / g and the biases: what both directions need
static int gs_check(const TzrGateScale* m, GsArgs* A) {
  if (m->B <= 0 || m->H <= 0 || m->n_slots <= 0) return TZR_ERR_INVALID;
  if (m->n_slots > GS_N || (m->H & 3) || m->H > 4096) return TZR_ERR_UNSUPPORTED;
  for (int n = 0; n < m->n_slots; ++n) {
    TZR_TRY(tzr_rows_operand(m->z[n], m->z_stride[n], m->H));
    TZR_TRY(tzr_rows_operand(m->g[n], m->g_stride[n], m->H));
    if (!m->bg[n] || (m->bg[n] & 15) || (m->bz[n] & 15)) return TZR_ERR_INVALID;
    A->z[n] = reinterpret_cast<const float*>(m->z[n]);
    A->z_stride[n] = m->z_stride[n];
    A->g[n] = reinterpret_cast<const float*>(m->g[n]);
    A->g_stride[n] = m->g_stride[n];
    A->bz[n] = reinterpret_cast<const float*>(m->bz[n]);
    A->bg[n] = reinterpret_cast<const float*>(m->bg[n]);
  }
  return TZR_OK;
}

extern "C" int tzr_gate_scale_fwd(const TzrGateScale* h_gs, void* stream) {
  if (!h_gs) return TZR_ERR_INVALID;
  GsArgs A = {};
  TZR_TRY(gs_check(h_gs, &A));
  for (int n = 0; n < h_gs->n_slots; ++n) {
    TZR_TRY(tzr_rows_operand(h_gs->out[n], h_gs->out_stride[n], h_gs->H));
    A.out[n] = reinterpret_cast<float*>(h_gs->out[n]);
    A.out_stride[n] = h_gs->out_stride[n];
  }
  const GsGeometry q = gs_geometry(h_gs->B, h_gs->H);
  const dim3 grid((unsigned)q.n_wg, (unsigned)h_gs->n_slots);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h_gs->relu)
    hipLaunchKernelGGL(tzr_gate_scale_fwd_kernel<true>, grid, dim3(GS_THREADS), 0, s, A, h_gs->B, h_gs->H, q.rows_per_wg, q.CW, h_gs->gamma);
  else
    hipLaunchKernelGGL(tzr_gate_scale_fwd_kernel<false>, grid, dim3(GS_THREADS), 0, s, A, h_gs->B, h_gs->H, q.rows_per_wg, q.CW, h_gs->gamma);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_gate_scale_bwd_workspace(int64_t B, int H, int n_slots) {
  if (B <= 0 || H <= 0 || (H & 3) || H > 4096 || n_slots <= 0 || n_slots > GS_N) return 256;
  return (size_t)gs_geometry(B, H).n_wg * (size_t)n_slots * 2 * (size_t)H * sizeof(float) + 256;
}

extern "C" int tzr_gate_scale_bwd(const TzrGateScale* h_gs, void* stream) {
  if (!h_gs) return TZR_ERR_INVALID;
  GsArgs A = {};
  TZR_TRY(gs_check(h_gs, &A));
  for (int n = 0; n < h_gs->n_slots; ++n) {
    TZR_TRY(tzr_rows_operand(h_gs->dz[n], h_gs->dz_stride[n], h_gs->H));
    TZR_TRY(tzr_rows_operand(h_gs->dg[n], h_gs->dg_stride[n], h_gs->H));
    if (h_gs->grad_out[n]) TZR_TRY(tzr_rows_operand(h_gs->grad_out[n], h_gs->grad_out_stride[n], h_gs->H));
    A.dz[n] = reinterpret_cast<float*>(h_gs->dz[n]);
    A.dz_stride[n] = h_gs->dz_stride[n];
    A.dg[n] = reinterpret_cast<float*>(h_gs->dg[n]);
    A.dg_stride[n] = h_gs->dg_stride[n];
    A.go[n] = reinterpret_cast<const float*>(h_gs->grad_out[n]);
    A.go_stride[n] = h_gs->grad_out_stride[n];
  }
  if (!h_gs->d_bias || (h_gs->d_bias & 15)) return TZR_ERR_INVALID;
  if (!h_gs->ws || (h_gs->ws & 255) || h_gs->ws_bytes < tzr_gate_scale_bwd_workspace(h_gs->B, h_gs->H, h_gs->n_slots) - 256)
    return TZR_ERR_WORKSPACE;
  const GsGeometry q = gs_geometry(h_gs->B, h_gs->H);
  const int P = h_gs->n_slots * 2 * h_gs->H;
  float* parts = reinterpret_cast<float*>(h_gs->ws);
  const dim3 grid((unsigned)q.n_wg, (unsigned)h_gs->n_slots);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h_gs->relu)
    hipLaunchKernelGGL(tzr_gate_scale_bwd_kernel<true>, grid, dim3(GS_THREADS), 0, s, A, h_gs->B, h_gs->H, q.rows_per_wg, q.CW, h_gs->gamma,
                       parts, P);
  else
    hipLaunchKernelGGL(tzr_gate_scale_bwd_kernel<false>, grid, dim3(GS_THREADS), 0, s, A, h_gs->B, h_gs->H, q.rows_per_wg, q.CW, h_gs->gamma,
                       parts, P);
  hipLaunchKernelGGL(tzr_parts_sum_finish_kernel<>, dim3((unsigned)((P + 63) / 64)), dim3(TZR_FIN_THREADS), 0, s, parts, (int)q.n_wg, P,
                     reinterpret_cast<float*>(h_gs->d_bias));
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
