// The cross network of Deep & Cross (v1), the whole stack of L layers in one launch per direction.  Replaces Cross.forward of
// the reference (tzrec/modules/interaction.py:94-132: per layer a [B, D] x [D, 1] product, a broadcast multiply and two adds,
// about twice that in autograd, every x_l saved) for fp32 rows of any width D <= 1024 and L <= 8 layers:
//
//   forward    x_0 = x;  s_l = x_l . w_l;  x_{l+1} = s_l x_0 + b_l + x_l  (l = 0 .. L-1);  y = x_L;  the scalars s -> [B, L]
//   backward   a = g, d0 = 0;  for l = L-1 .. 0:  t_l = a . x_0;  d0 += s_l a;  a += t_l w_l;   dx = a + d0
//              dw_l = sum_b t_{b,l} x_{l,b},  db_l = sum_b a_{b,l}  (a as it stands when layer l is reached)
//
// No x_l is kept: x_l = c_l x_0 + sum_{j<l} b_j with c_l = 1 + sum_{j<l} s_j, so
//
//   dw_l = sum_b (t_{b,l} c_{b,l}) x_{0,b} + (sum_b t_{b,l}) sum_{j<l} b_j        db_l = colsum(g) + sum_{j>l} (sum_b t_{b,j}) w_j
//
// and the sums over the batch are L + 1 vectors (A_l = sum_b t c x_0, G = colsum(g)) and L scalars (T_l = sum_b t_{b,l}).
//
// One wave per sample, a grid-stride loop over the samples (as jagged_encoders.hip); lane i holds elements i, i + 64, ... of
// the sample's row (KR = D / 64 rounded up to a power of two of them, a compile-time bound: the row, the running x_l / a and
// the wave's L + 1 accumulators are register arrays with constant indices only).  Loads and stores are single floats, a
// wave's consecutive: rows need 4-byte alignment only (a Criteo-shaped group is 429 wide).  w_l and b_l (at most 64 KB
// together) are read per sample and stay in the caches.
//
// Reduction order: a wave adds its samples in the order of the grid-stride loop, a workgroup its four waves 0..3, and the
// finishing launch the workgroups' rows 0..G-1 in the interleaved order of parts_sum.h: a function of (B, D, L) alone.  No atomics.
#include "parts_sum.h"
#include "row_kernels.h"

#define CN_THREADS 256
#define CN_WAVES (CN_THREADS / TZR_WAVE)
#define CN_MAXDIM 1024
#define CN_MAXL 8
#define CN_MAXGRID 512  // workgroups of a launch = rows of partial sums the finishing launch adds

struct CnParams {  // the layers' parameters: L separate [1, D] / [D] tensors, passed by value
  const float* w[CN_MAXL];
  const float* b[CN_MAXL];
};

template <int KR>
__global__ __launch_bounds__(CN_THREADS) void tzr_cross_fwd_kernel(const float* __restrict__ x, int64_t xs, CnParams P, int L, int64_t B,
                                                                   int D, float* __restrict__ y, int64_t ys, float* __restrict__ s) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  for (int64_t b = (int64_t)blockIdx.x * CN_WAVES + wv; b < B; b += (int64_t)gridDim.x * CN_WAVES) {
    float x0[KR], x1[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      x0[k] = c < D ? x[b * xs + c] : 0.f;
      x1[k] = x0[k];
    }
#pragma unroll
    for (int l = 0; l < CN_MAXL; ++l) {
      if (l >= L) break;
      float wl[KR], bl[KR];
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        const int c = lane + TZR_WAVE * k;
        wl[k] = c < D ? P.w[l][c] : 0.f;
        bl[k] = c < D ? P.b[l][c] : 0.f;
      }
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < KR; ++k) dot = fmaf(x1[k], wl[k], dot);
      const float sl = tzr_wave_sum(dot);
#pragma unroll
      for (int k = 0; k < KR; ++k) x1[k] = fmaf(sl, x0[k], bl[k]) + x1[k];
      if (s && lane == 0) s[b * L + l] = sl;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      if (c < D) y[b * ys + c] = x1[k];
    }
  }
}

// floats of one workgroup's row of partial sums: [A_0 .. A_{L-1} | G] (D each), then T_0 .. T_{L-1}
__host__ __device__ static inline size_t cn_row_len(int D, int L) { return (size_t)(L + 1) * (size_t)D + (size_t)L; }

static inline unsigned cn_grid(int64_t B) { return tzr_row_grid(B, CN_WAVES, CN_MAXGRID); }

// LL: compile-time bound of the layer loops (the smallest instantiated one covering L)
template <int KR, int LL>
__global__ __launch_bounds__(CN_THREADS) void tzr_cross_bwd_kernel(const float* __restrict__ g, int64_t gs, const float* __restrict__ x,
                                                                   int64_t xs, const float* __restrict__ s, CnParams P, int L, int64_t B,
                                                                   int D, float* __restrict__ dx, int64_t dxs, float* __restrict__ parts) {
  __shared__ float red[CN_WAVES][KR * TZR_WAVE];
  __shared__ float redt[CN_WAVES][CN_MAXL];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  float acc[LL + 1][KR];  // A_0 .. A_{LL-1}, G
  float T[LL];
#pragma unroll
  for (int v = 0; v <= LL; ++v)
#pragma unroll
    for (int k = 0; k < KR; ++k) acc[v][k] = 0.f;
#pragma unroll
  for (int l = 0; l < LL; ++l) T[l] = 0.f;
  for (int64_t b = (int64_t)blockIdx.x * CN_WAVES + wv; b < B; b += (int64_t)gridDim.x * CN_WAVES) {
    float x0[KR], a[KR], d0[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      x0[k] = c < D ? x[b * xs + c] : 0.f;
      a[k] = c < D ? g[b * gs + c] : 0.f;
      d0[k] = 0.f;
      acc[LL][k] += a[k];
    }
    float sl[LL], cl[LL];  // s_l and c_l = 1 + s_0 + .. + s_{l-1}
    float c_run = 1.0f;
#pragma unroll
    for (int l = 0; l < LL; ++l) {
      sl[l] = l < L ? s[b * L + l] : 0.f;
      cl[l] = c_run;
      c_run += sl[l];
    }
#pragma unroll
    for (int l = LL - 1; l >= 0; --l) {
      if (l < L) {  // (uniform)
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < KR; ++k) dot = fmaf(a[k], x0[k], dot);
        const float t = tzr_wave_sum(dot);
        const float u = t * cl[l];
        T[l] += t;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const int c = lane + TZR_WAVE * k;
          d0[k] = fmaf(sl[l], a[k], d0[k]);
          acc[l][k] = fmaf(u, x0[k], acc[l][k]);
          a[k] = fmaf(t, c < D ? P.w[l][c] : 0.f, a[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + TZR_WAVE * k;
      if (c < D) dx[b * dxs + c] = a[k] + d0[k];
    }
  }
  // the workgroup's row of partial sums: its waves added in the order 0..3, one vector at a time through LDS
  float* pr = parts + (size_t)blockIdx.x * cn_row_len(D, L);
#pragma unroll
  for (int v = 0; v <= LL; ++v) {
    if (v < L || v == LL) {  // (uniform)
#pragma unroll
      for (int k = 0; k < KR; ++k) red[wv][lane + TZR_WAVE * k] = acc[v][k];
      __syncthreads();
      float* dst = pr + (size_t)(v == LL ? L : v) * D;
      for (int c = threadIdx.x; c < D; c += CN_THREADS) dst[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
      __syncthreads();
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < LL; ++l) redt[wv][l] = T[l];
  }
  __syncthreads();
  if ((int)threadIdx.x < L) {
    const int l = threadIdx.x;
    pr[(size_t)(L + 1) * D + l] = ((redt[0][l] + redt[1][l]) + redt[2][l]) + redt[3][l];
  }
}

// grid (D / 64 rounded up, L + 1), TZR_FIN_THREADS threads: workgroup (i, v) adds column tile i of vector v over the G rows of
// partial sums (parts_sum.h: interleaved) and writes dw_v (v < L) or, from G, every db_l (v == L).  T_l: wave l adds the rows
// lane, lane + 64, ..., then a fixed tree over the lanes.
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_cross_bwd_finish_kernel(const float* __restrict__ parts, int G, CnParams P, int L,
                                                                               int D, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float Ts[CN_MAXL];
  __shared__ float red[TZR_FIN_THREADS];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int v = blockIdx.y;
  const int c = blockIdx.x * TZR_WAVE + lane;
  const size_t R = cn_row_len(D, L);
  if (wv < L) {  // (uniform per wave)
    const float* src = parts + (size_t)(L + 1) * D + wv;
    float t = 0.f;
#pragma unroll 8
    for (int w = lane; w < G; w += TZR_WAVE) t += src[(size_t)w * R];
    t = tzr_wave_sum(t);
    if (lane == 0) Ts[wv] = t;
  }
  const float tot = tzr_parts_sum_interleaved<true>(c < D ? parts + (size_t)v * D + c : nullptr, G, R, red);  // (Ts: behind its barrier)
  if (wv != 0 || c >= D) return;
  if (v < L) {  // dw_v = A_v + T_v (b_0 + .. + b_{v-1})
    float bs = 0.f;
#pragma unroll
    for (int j = 0; j < CN_MAXL; ++j)
      if (j < v) bs += P.b[j][c];
    dw[(size_t)v * D + c] = fmaf(Ts[v], bs, tot);
  } else {  // db_l = G + sum_{j>l} T_j w_j
    float acc = tot;
#pragma unroll
    for (int l = CN_MAXL - 1; l >= 0; --l)
      if (l < L) {
        db[(size_t)l * D + c] = acc;
        acc = fmaf(Ts[l], P.w[l][c], acc);
      }
  }
}

static int cn_check(int64_t B, int D, int L) {
  if (B < 0 || D <= 0 || L <= 0) return TZR_ERR_INVALID;
  if (D > CN_MAXDIM || L > CN_MAXL) return TZR_ERR_UNSUPPORTED;
  return TZR_OK;
}

static int cn_params(const float* const* h_w, const float* const* h_b, int L, CnParams* P) {
  if (!h_w || !h_b) return TZR_ERR_INVALID;
  for (int l = 0; l < CN_MAXL; ++l) {
    P->w[l] = l < L ? h_w[l] : nullptr;
    P->b[l] = l < L ? h_b[l] : nullptr;
    if (l < L && (!P->w[l] || !P->b[l])) return TZR_ERR_INVALID;
  }
  return TZR_OK;
}

extern "C" int tzr_cross_fwd(const float* d_x, int64_t x_stride, const float* const* h_w, const float* const* h_b, int L, int64_t B,
                             int D, float* d_y, int64_t y_stride, float* d_s, void* stream) {
  if (const int rc = cn_check(B, D, L)) return rc;
  if (x_stride < D || y_stride < D) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  CnParams P;
  if (!d_x || !d_y || cn_params(h_w, h_b, L, &P) != TZR_OK) return TZR_ERR_INVALID;
#define CN_FWD(KR_)                                                                                                               \
  hipLaunchKernelGGL((tzr_cross_fwd_kernel<KR_>), dim3(cn_grid(B)), dim3(CN_THREADS), 0, static_cast<hipStream_t>(stream), d_x, x_stride, \
                     P, L, B, D, d_y, y_stride, d_s)
  TZR_BY_KR(CN_FWD);
#undef CN_FWD
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_cross_bwd_workspace(int64_t B, int D, int L) {
  if (cn_check(B, D, L) != TZR_OK) return 256;
  return (size_t)cn_grid(B) * cn_row_len(D, L) * sizeof(float) + 256;
}

extern "C" int tzr_cross_bwd(const float* d_grad_y, int64_t gy_stride, const float* d_x, int64_t x_stride, const float* d_s,
                             const float* const* h_w, const float* const* h_b, int L, int64_t B, int D, float* d_dx, int64_t dx_stride,
                             float* d_dw, float* d_db, void* ws, size_t ws_size, void* stream) {
  if (const int rc = cn_check(B, D, L)) return rc;
  if (gy_stride < D || x_stride < D || dx_stride < D) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  CnParams P;
  if (!d_grad_y || !d_x || !d_s || !d_dx || !d_dw || !d_db || !ws || (reinterpret_cast<uintptr_t>(ws) & 255) ||
      cn_params(h_w, h_b, L, &P) != TZR_OK)
    return TZR_ERR_INVALID;
  if (ws_size < tzr_cross_bwd_workspace(B, D, L) - 256) return TZR_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = cn_grid(B);
  float* parts = static_cast<float*>(ws);
#define CN_BWD_L(KR_, LL_)                                                                                                         \
  hipLaunchKernelGGL((tzr_cross_bwd_kernel<KR_, LL_>), dim3(grid), dim3(CN_THREADS), 0, st, d_grad_y, gy_stride, d_x, x_stride, d_s, P, L, \
                     B, D, d_dx, dx_stride, parts)
#define CN_BWD(KR_)                    \
  do {                                 \
    if (L <= 2) CN_BWD_L(KR_, 2);      \
    else if (L <= 4) CN_BWD_L(KR_, 4); \
    else CN_BWD_L(KR_, 8);             \
  } while (0)
  TZR_BY_KR(CN_BWD);
#undef CN_BWD
#undef CN_BWD_L
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_cross_bwd_finish_kernel, dim3((unsigned)((D + TZR_WAVE - 1) / TZR_WAVE), (unsigned)(L + 1)), dim3(TZR_FIN_THREADS), 0,
                     st, parts, (int)grid, P, L, D, d_dw, d_db);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
