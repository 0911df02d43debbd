// LayerNorm, an optional ReLU and an optional elementwise mask over rows, for up to eight outputs in one launch per direction:
// the non-GEMM work of MaskNet (tzrec/modules/masknet.py:77-85 and 142-161: `ln_emb(x) * mask_i` in front of every block,
// `LayerNorm -> ReLU` behind every block's hidden layer, the parallel blocks' concat), fp32 rows of any width D <= 1024.
//
//   forward    f_j = act(LN(x_j; gamma_j, beta_j, eps));  out_j = f_j * m_j  (or f_j, without masks)      j = 0 .. n_out-1
//   backward   gm_j = gout_j * f_j;  gf = sum_j gout_j * m_j (shared x) or gout_j * m_j (per output), through the ReLU mask;
//              gy = gamma * gf;  gx = rstd (gy - mean(gy) - xh mean(gy xh));  dgamma = sum_b gf xh;  dbeta = sum_b gf
//
// With shared_x every output reads the same row x, gamma and beta: mean and rstd are computed once and LN(x) is never
// written.  Otherwise output j has its own x_j, gamma_j, beta_j and its own slice of the grid (blockIdx.y = j), so a wave
// never holds more than one pair of dgamma / dbeta accumulators.  LN is nn.LayerNorm's: biased variance, eps inside the
// root; the variance is sum (x - mean)^2 over the registers, a second pass, never E[x^2] - E[x]^2.
//
// One wave per sample, a grid-stride loop over the samples (as cross_net.hip); lane i holds elements i, i + 64, ... of the
// row (KR = D / 64 rounded up to a power of two of them, a compile-time bound).  Loads and stores are single floats, a wave's
// consecutive: rows need 4-byte alignment only, every x_j / m_j / out_j may be a column slice of a wider tensor (the parallel
// blocks' concat buffer is written in place).  The pointers travel by value in a struct, entries picked by compare-and-select
// (no dynamic index into the struct, nothing the compiler would copy to scratch).
//
// The ReLU mask of the backward is recomputed, not read: lm_norm below is the one instruction sequence both directions run
// on the same x, the stored mean and rstd, gamma and beta, so y > 0 decides the same way in both.
//
// Reduction order: a wave adds its samples in the order of the grid-stride loop, a workgroup its four waves 0..3, and the
// finishing launch the workgroups' rows 0..G-1 in the interleaved order of parts_sum.h: a function of (B, D, n_out, shared_x)
// alone.  No atomics.
#include "parts_sum.h"
#include "row_kernels.h"

#define LM_THREADS 256
#define LM_WAVES (LM_THREADS / TZR_WAVE)
#define LM_MAXDIM 1024
#define LM_MAXOUT 8
#define LM_MAXGRID 512  // workgroups per grid slice = rows of partial sums the finishing launch adds

struct LmFwdParams {  // by value: the launch captures into a graph
  const float* x[LM_MAXOUT];
  int64_t xs[LM_MAXOUT];
  const float* gamma[LM_MAXOUT];
  const float* beta[LM_MAXOUT];
  const float* m[LM_MAXOUT];
  int64_t ms[LM_MAXOUT];
  float* out[LM_MAXOUT];
  int64_t os[LM_MAXOUT];
};

struct LmBwdParams {
  const float* gout[LM_MAXOUT];
  int64_t gs[LM_MAXOUT];
  const float* x[LM_MAXOUT];
  int64_t xs[LM_MAXOUT];
  const float* gamma[LM_MAXOUT];
  const float* beta[LM_MAXOUT];
  const float* m[LM_MAXOUT];
  int64_t ms[LM_MAXOUT];
  float* gx[LM_MAXOUT];
  int64_t gxs[LM_MAXOUT];
  float* gm[LM_MAXOUT];
  int64_t gms[LM_MAXOUT];
};

template <class T>
__device__ __forceinline__ T lm_pick(const T (&a)[LM_MAXOUT], int j) {  // a[j], j uniform, by selects
  T r = a[0];
#pragma unroll
  for (int i = 1; i < LM_MAXOUT; ++i)
    if (i == j) r = a[i];
  return r;
}

// the normalised element and the pre-activation: the forward's and the backward's one sequence
__device__ __forceinline__ float lm_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float lm_norm(float xh, float gamma, float beta) { return fmaf(xh, gamma, beta); }

// grid (G, 1) with shared_x, (G, n_out) without
template <int KR>
__global__ __launch_bounds__(LM_THREADS) void tzr_ln_mask_fwd_kernel(LmFwdParams P, int n_out, int shared_x, int has_mask, int relu,
                                                                     float eps, int64_t B, int D, float* __restrict__ stats) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int slot = shared_x ? 0 : (int)blockIdx.y;  // whose x, gamma, beta and statistics
  const int n_stat = shared_x ? 1 : n_out;
  const int nj = shared_x ? n_out : 1;
  const float* x = lm_pick(P.x, slot);
  const int64_t xs = lm_pick(P.xs, slot);
  const float* gamma = lm_pick(P.gamma, slot);
  const float* beta = lm_pick(P.beta, slot);
  const float inv_d = 1.0f / (float)D;
  for (int64_t b = (int64_t)blockIdx.x * LM_WAVES + wv; b < B; b += (int64_t)gridDim.x * LM_WAVES) {
    float f[KR];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      f[k] = c < D ? x[b * xs + c] : 0.f;
      sum += f[k];
    }
    const float mean = tzr_wave_sum(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      const float d = c < D ? f[k] - mean : 0.f;
      sq = fmaf(d, d, sq);
    }
    const float rstd = 1.0f / sqrtf(tzr_wave_sum(sq) * inv_d + eps);
    if (lane == 0) {
      stats[(b * n_stat + slot) * 2] = mean;
      stats[(b * n_stat + slot) * 2 + 1] = rstd;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      const float y = c < D ? lm_norm(lm_xhat(f[k], mean, rstd), gamma[c], beta[c]) : 0.f;
      f[k] = relu ? fmaxf(y, 0.f) : y;
    }
    for (int j = 0; j < nj; ++j) {
      const int o = slot + j;
      float* out = lm_pick(P.out, o);
      const int64_t os = lm_pick(P.os, o);
      const float* m = lm_pick(P.m, o);
      const int64_t ms = lm_pick(P.ms, o);
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        const int c = lane + TZR_WAVE * k;
        if (c < D) out[b * os + c] = has_mask ? f[k] * m[b * ms + c] : f[k];
      }
    }
  }
}

static inline unsigned lm_grid(int64_t B) { return tzr_row_grid(B, LM_WAVES, LM_MAXGRID); }

// floats of one workgroup's row of partial sums: [dgamma | dbeta]; the rows of slot s are s G .. s G + G - 1
__host__ __device__ static inline size_t lm_row_len(int D) { return 2 * (size_t)D; }

template <int KR>
__global__ __launch_bounds__(LM_THREADS) void tzr_ln_mask_bwd_kernel(LmBwdParams P, int n_out, int shared_x, int has_mask, int relu,
                                                                     int64_t B, int D, const float* __restrict__ stats,
                                                                     float* __restrict__ parts) {
  __shared__ float red[LM_WAVES][KR * TZR_WAVE];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int slot = shared_x ? 0 : (int)blockIdx.y;
  const int n_stat = shared_x ? 1 : n_out;
  const int nj = shared_x ? n_out : 1;
  const float* x = lm_pick(P.x, slot);
  const int64_t xs = lm_pick(P.xs, slot);
  const float* gamma = lm_pick(P.gamma, slot);
  const float* beta = lm_pick(P.beta, slot);
  float* gx = lm_pick(P.gx, slot);
  const int64_t gxs = lm_pick(P.gxs, slot);
  const float inv_d = 1.0f / (float)D;
  float gam[KR], bet[KR], acc_g[KR], acc_b[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int c = lane + TZR_WAVE * k;
    gam[k] = c < D ? gamma[c] : 0.f;
    bet[k] = c < D ? beta[c] : 0.f;
    acc_g[k] = 0.f;
    acc_b[k] = 0.f;
  }
  for (int64_t b = (int64_t)blockIdx.x * LM_WAVES + wv; b < B; b += (int64_t)gridDim.x * LM_WAVES) {
    const float mean = stats[(b * n_stat + slot) * 2];
    const float rstd = stats[(b * n_stat + slot) * 2 + 1];
    float xh[KR], y[KR], gf[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      xh[k] = c < D ? lm_xhat(x[b * xs + c], mean, rstd) : 0.f;
      y[k] = lm_norm(xh[k], gam[k], bet[k]);
      gf[k] = 0.f;
    }
    for (int j = 0; j < nj; ++j) {
      const int o = slot + j;
      const float* go = lm_pick(P.gout, o);
      const int64_t gs = lm_pick(P.gs, o);
      const float* m = lm_pick(P.m, o);
      const int64_t ms = lm_pick(P.ms, o);
      float* gm = lm_pick(P.gm, o);
      const int64_t gms = lm_pick(P.gms, o);
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        const int c = lane + TZR_WAVE * k;
        const float g = c < D ? go[b * gs + c] : 0.f;
        if (has_mask) {
          if (c < D) {
            gm[b * gms + c] = g * (relu ? fmaxf(y[k], 0.f) : y[k]);
            gf[k] = fmaf(g, m[b * ms + c], gf[k]);
          }
        } else {
          gf[k] += g;
        }
      }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (relu) gf[k] = y[k] > 0.f ? gf[k] : 0.f;
      acc_g[k] = fmaf(gf[k], xh[k], acc_g[k]);
      acc_b[k] += gf[k];
      gf[k] *= gam[k];  // gy
      s1 += gf[k];
      s2 = fmaf(gf[k], xh[k], s2);
    }
    s1 = tzr_wave_sum(s1) * inv_d;
    s2 = tzr_wave_sum(s2) * inv_d;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      if (c < D) gx[b * gxs + c] = rstd * ((gf[k] - s1) - xh[k] * s2);
    }
  }
  // the workgroup's row of partial sums: its waves added in the order 0..3, one vector at a time through LDS
  float* pr = parts + ((size_t)slot * gridDim.x + blockIdx.x) * lm_row_len(D);
#pragma unroll
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int k = 0; k < KR; ++k) red[wv][lane + TZR_WAVE * k] = v == 0 ? acc_g[k] : acc_b[k];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += LM_THREADS) pr[(size_t)v * D + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    __syncthreads();
  }
}

// grid (D / 64 rounded up, 2, n_stat), TZR_FIN_THREADS threads: workgroup (i, v, s) adds column tile i of vector v (0: dgamma,
// 1: dbeta) of slot s over the G rows of partial sums (parts_sum.h: interleaved).
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_ln_mask_bwd_finish_kernel(const float* __restrict__ parts, int G, int D,
                                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[TZR_FIN_THREADS];
  const int v = blockIdx.y, slot = blockIdx.z;
  const int c = blockIdx.x * TZR_WAVE + (threadIdx.x & (TZR_WAVE - 1));
  const size_t R = lm_row_len(D);
  const float tot = tzr_parts_sum_interleaved(c < D ? parts + (size_t)slot * G * R + (size_t)v * D + c : nullptr, G, R, red);
  if (threadIdx.x < TZR_WAVE && c < D) (v == 0 ? dgamma : dbeta)[(size_t)slot * D + c] = tot;
}

static int lm_check(int64_t B, int D, int n_out) {
  if (B < 0 || D <= 0 || n_out <= 0) return TZR_ERR_INVALID;
  if (D > LM_MAXDIM || n_out > LM_MAXOUT) return TZR_ERR_UNSUPPORTED;
  return TZR_OK;
}

// n pointers and their row strides (in floats, >= D) from the host arrays into the struct's arrays
template <class T>
static int lm_rows(T* const* h_p, const int64_t* h_s, int n, int D, T** p, int64_t* s) {
  if (!h_p || !h_s) return TZR_ERR_INVALID;
  for (int j = 0; j < LM_MAXOUT; ++j) {
    p[j] = j < n ? h_p[j] : nullptr;
    s[j] = j < n ? h_s[j] : 0;
    if (j < n && !p[j]) return TZR_ERR_INVALID;
  }
  return TZR_OK;
}

static int lm_strides_ok(const int64_t* h_s, int n, int D) {  // (a null array is the null check's to report)
  if (h_s)
    for (int j = 0; j < n; ++j)
      if (h_s[j] < D) return 0;
  return 1;
}

static int lm_vectors(const float* const* h_g, const float* const* h_b, int n, const float** g, const float** b) {
  if (!h_g || !h_b) return TZR_ERR_INVALID;
  for (int j = 0; j < LM_MAXOUT; ++j) {
    g[j] = j < n ? h_g[j] : nullptr;
    b[j] = j < n ? h_b[j] : nullptr;
    if (j < n && (!g[j] || !b[j])) return TZR_ERR_INVALID;
  }
  return TZR_OK;
}

extern "C" int tzr_ln_mask_fwd(const float* const* h_x, const int64_t* h_x_stride, const float* const* h_gamma,
                               const float* const* h_beta, const float* const* h_m, const int64_t* h_m_stride, float* const* h_out,
                               const int64_t* h_out_stride, int n_out, int shared_x, int relu, float eps, int64_t B, int D,
                               float* d_stats, void* stream) {
  if (const int rc = lm_check(B, D, n_out)) return rc;
  const int n_x = shared_x ? 1 : n_out;
  if (!lm_strides_ok(h_x_stride, n_x, D) || !lm_strides_ok(h_out_stride, n_out, D) || (h_m && !lm_strides_ok(h_m_stride, n_out, D)))
    return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  LmFwdParams P;
  if (!d_stats || lm_rows(h_x, h_x_stride, n_x, D, P.x, P.xs) != TZR_OK || lm_vectors(h_gamma, h_beta, n_x, P.gamma, P.beta) != TZR_OK ||
      lm_rows(h_out, h_out_stride, n_out, D, P.out, P.os) != TZR_OK)
    return TZR_ERR_INVALID;
  if (h_m) {
    if (lm_rows(h_m, h_m_stride, n_out, D, P.m, P.ms) != TZR_OK) return TZR_ERR_INVALID;
  } else {
    for (int j = 0; j < LM_MAXOUT; ++j) P.m[j] = nullptr, P.ms[j] = 0;
  }
  const dim3 grid(lm_grid(B), shared_x ? 1u : (unsigned)n_out);
#define LM_FWD(KR_)                                                                                                              \
  hipLaunchKernelGGL((tzr_ln_mask_fwd_kernel<KR_>), grid, dim3(LM_THREADS), 0, static_cast<hipStream_t>(stream), P, n_out, shared_x ? 1 : 0, \
                     h_m ? 1 : 0, relu ? 1 : 0, eps, B, D, d_stats)
  TZR_BY_KR(LM_FWD);
#undef LM_FWD
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_ln_mask_bwd_workspace(int64_t B, int D, int n_out, int shared_x) {
  if (lm_check(B, D, n_out) != TZR_OK) return 256;
  return (size_t)(shared_x ? 1 : n_out) * lm_grid(B) * lm_row_len(D) * sizeof(float) + 256;
}

extern "C" int tzr_ln_mask_bwd(const float* const* h_gout, const int64_t* h_gout_stride, const float* const* h_x,
                               const int64_t* h_x_stride, const float* const* h_gamma, const float* const* h_beta,
                               const float* const* h_m, const int64_t* h_m_stride, const float* d_stats, int n_out, int shared_x,
                               int relu, int64_t B, int D, float* const* h_gx, const int64_t* h_gx_stride, float* const* h_gm,
                               const int64_t* h_gm_stride, float* d_dgamma, float* d_dbeta, void* ws, size_t ws_size, void* stream) {
  if (const int rc = lm_check(B, D, n_out)) return rc;
  const int n_x = shared_x ? 1 : n_out;
  if (!lm_strides_ok(h_gout_stride, n_out, D) || !lm_strides_ok(h_x_stride, n_x, D) || !lm_strides_ok(h_gx_stride, n_x, D) ||
      (h_m && (!lm_strides_ok(h_m_stride, n_out, D) || !lm_strides_ok(h_gm_stride, n_out, D))))
    return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  LmBwdParams P;
  if (!d_stats || !d_dgamma || !d_dbeta || !ws || (reinterpret_cast<uintptr_t>(ws) & 255) ||
      lm_rows(h_gout, h_gout_stride, n_out, D, P.gout, P.gs) != TZR_OK || lm_rows(h_x, h_x_stride, n_x, D, P.x, P.xs) != TZR_OK ||
      lm_vectors(h_gamma, h_beta, n_x, P.gamma, P.beta) != TZR_OK || lm_rows(h_gx, h_gx_stride, n_x, D, P.gx, P.gxs) != TZR_OK)
    return TZR_ERR_INVALID;
  if (h_m) {
    if (lm_rows(h_m, h_m_stride, n_out, D, P.m, P.ms) != TZR_OK || lm_rows(h_gm, h_gm_stride, n_out, D, P.gm, P.gms) != TZR_OK)
      return TZR_ERR_INVALID;
  } else {
    for (int j = 0; j < LM_MAXOUT; ++j) P.m[j] = nullptr, P.ms[j] = 0, P.gm[j] = nullptr, P.gms[j] = 0;
  }
  if (ws_size < tzr_ln_mask_bwd_workspace(B, D, n_out, shared_x) - 256) return TZR_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned G = lm_grid(B);
  float* parts = static_cast<float*>(ws);
  const dim3 grid(G, (unsigned)n_x);
#define LM_BWD(KR_)                                                                                                               \
  hipLaunchKernelGGL((tzr_ln_mask_bwd_kernel<KR_>), grid, dim3(LM_THREADS), 0, st, P, n_out, shared_x ? 1 : 0, h_m ? 1 : 0, relu ? 1 : 0, B, \
                     D, d_stats, parts)
  TZR_BY_KR(LM_BWD);
#undef LM_BWD
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_ln_mask_bwd_finish_kernel, dim3((unsigned)((D + TZR_WAVE - 1) / TZR_WAVE), 2u, (unsigned)n_x), dim3(TZR_FIN_THREADS),
                     0, st, parts, (int)G, D, d_dgamma, d_dbeta);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
