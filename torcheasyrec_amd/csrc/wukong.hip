// The two per-sample operations of a WuKong layer outside its GEMMs (tzrec/modules/interaction.py:236-378), fp32:
//
//   FM front   (FactorizationMachineBlock.forward up to and including self.norm)      X [F, D], W [F, k]
//     forward    P = X^T W [D, k];  Z = X P [F, k];  out = LN(vec(Z); gamma, beta, eps) over the F k values
//     backward   zh = (Z - mean) rstd;  gy = gout gamma;  gZ = rstd (gy - mean(gy) - zh mean(gy zh));
//                dP = X^T gZ;  gX = gZ P^T + W dP^T;  dW = sum_b X dP;  dgamma = sum_b gout zh;  dbeta = sum_b gout
//   mix        (lcb, residual_projection, the concat, the add and self.norm of WuKongLayer.forward)   Fm [Ff, D], Fo = Ff + Fl
//     forward    Wc[f, o] = Wr[f, o] (Wr null: f == o) + (o >= Ff ? Wl[f, o - Ff] : 0);
//                pre[o, :] = (o < Ff ? Fm[o, :] : 0) + sum_f Wc[f, o] X[f, :];  out[o, :] = LN(pre[o, :]; gamma, beta, eps) over D
//     backward   gpre from LN's backward per row;  gFm = gpre[:Ff];  gX = Wc gpre;  dWc = sum_b X gpre^T;  dWr = dWc;
//                dWl = dWc[:, Ff:];  dgamma, dbeta [D] over all B Fo rows
//
// LN is nn.LayerNorm's: biased variance, eps inside the root, the variance a second pass over (z - mean)^2 (as ln_mask.hip).
// Neither P, Z, Wc nor pre reaches memory: the forward writes the output and (mean, rstd), the backward recomputes the rest
// from X (and Fm) by the forward's instruction sequence.
//
// A workgroup of 256 threads takes one sample at a time in a grid-stride loop; X is staged once per sample into LDS, W / Wc
// once per workgroup.  Every product is wk_tile: a 16 x 16 output tile on v_mfma_f32_16x16x4_f32 (exact fp32) whose operands
// are LDS arrays read through a (row, column) stride pair, so a transpose is a swap of the pair and nothing is transposed in
// memory; tiles go round-robin over the four waves; a tail in F, D, k, Fo is a zero operand (selected, never multiplied in).
// dW / dWc live in MFMA accumulators across the whole loop (wave w owns the tiles w, w + 4, ..), dgamma / dbeta in registers.
//
// LDS.  The emulator's __shared__ is a function-local static, so the arrays are static and sized by a template class:
// S (F, Fo, k <= 32) and L (<= 64), D <= 128 in both.  Row strides are padded (wk_pad: 33, 72, 136) so that both the
// "16 rows x 4 columns" and the "4 rows x 16 columns" operand reads of a wave are at most 2-way bank conflicts.
//                  X          P (+ dP)       Z, W / pre, Wc        total     workgroups per CU (160 KB)
//   fm  fwd  S    17.0 KB    16.5 KB         4.1 + 4.1 KB          42 KB     3
//   fm  bwd  S    17.0 KB    33.0 KB         4.1 + 4.1 KB          58 KB     2
//   mix fwd  S    17.0 KB       -            17.0 + 4.1 KB         38 KB     4
//   mix bwd  S    17.0 KB       -            17.0 + 4.1 KB         38 KB     4
//   fm  fwd  L    34.0 KB    36.0 KB         18.0 + 18.0 KB        106 KB    1
//   fm  bwd  L    34.0 KB    72.0 KB         18.0 + 18.0 KB        142 KB    1
//   mix      L    34.0 KB       -            34.0 + 18.0 KB        86 KB     1
// The example's shapes (F = 27 then 32, k = 24, 16 + 16 outputs, D = 128) are class S.  What the static arrays cost: a class-S
// shape with a small D (say 16) still reserves the D = 128 rows, where arrays sized at launch would fit twice as many
// workgroups of the fm backward; class L runs at one workgroup (4 waves) per CU.
//
// Reduction order: a workgroup adds its samples in the order of the grid-stride loop (mix: a wave its rows w, w + 4, .. of each
// sample, then the four waves 0..3), and the finishing launch the workgroups' rows 0..G-1 in the interleaved order of
// parts_sum.h: a function of the shapes alone.  No atomics.  Loads and stores of x, fm, out and their gradients are single
// floats: 4-byte alignment, any per-sample stride >= the row's width.
#include "parts_sum.h"

#define WK_THREADS 256
#define WK_WAVES (WK_THREADS / TZR_WAVE)
#define WK_MAXF 64     // F, Fo and k
#define WK_MAXD 128
#define WK_MAXGRID 512  // workgroups of a pass over the batch = rows of partial sums the finishing launch adds

typedef float wk_f4 __attribute__((ext_vector_type(4)));

constexpr int wk_pad(int n) { return n % 64 == 0 ? n + 8 : n + 1; }

__device__ __forceinline__ wk_f4 wk_zero() {
  wk_f4 z = {0.f, 0.f, 0.f, 0.f};
  return z;
}

// acc += A[16 mt .. 16 mt + 15, 0..K) B[0..K, 16 nt .. 16 nt + 15]: A(i, k) = A[i ars + k acs] for i < M, B(k, j) = B[k brs + j bcs]
// for j < N, both in LDS; whatever lies outside is a zero operand (the address clamped to element 0, the value dropped).
// Every lane of the wave calls it with the same arguments.  q = lane >> 4, li = lane & 15.
__device__ __forceinline__ wk_f4 wk_tile(const float* A, int ars, int acs, int M, const float* B, int brs, int bcs, int N, int K, int mt, int nt,
                                         int q, int li, wk_f4 acc) {
  const int i = 16 * mt + li, j = 16 * nt + li;
  const bool iok = i < M, jok = j < N;
  const float* ap = A + (iok ? i : 0) * ars;
  const float* bp = B + (jok ? j : 0) * bcs;
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + q;
    const bool kok = k < K;
    const int kc = kok ? k : 0;
    const float a = ap[kc * acs], b = bp[kc * brs];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(iok && kok ? a : 0.f, jok && kok ? b : 0.f, acc, 0, 0, 0);
  }
  return acc;
}

// the sum of v over the workgroup, its waves added 0..3, in every thread.  red: WK_WAVES floats of LDS that nobody reads or
// writes until the next barrier after the call.
__device__ __forceinline__ float wk_block_sum(float v, float* red, int wv, int lane) {
  v = tzr_wave_sum(v);
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// X [F, D] of one sample into Xs (row stride XS); the caller's barriers are around it
__device__ __forceinline__ void wk_stage(const float* __restrict__ x, int F, int D, float* Xs, int XS) {
  for (int e = threadIdx.x; e < F * D; e += WK_THREADS) {
    const int f = e / D;
    Xs[f * XS + (e - f * D)] = x[e];
  }
}

// ---- FM front ---------------------------------------------------------------------------------------------------------

// P = X^T W -> Ps [D, k], then Z = X P -> Zs [F, k]; a barrier after each (the one in front is the caller's)
__device__ __forceinline__ void wk_fm_pz(const float* Xs, int XS, const float* Ws, float* Ps, float* Zs, int KS, int F, int D, int k, int wv, int q,
                                         int li) {
  const int NT = (k + 15) >> 4;
  const int DT = (D + 15) >> 4, FT = (F + 15) >> 4;
  for (int tile = wv; tile < DT * NT; tile += WK_WAVES) {
    const int mt = tile / NT, nt = tile - mt * NT;
    const wk_f4 acc = wk_tile(Xs, 1, XS, D, Ws, KS, 1, k, F, mt, nt, q, li, wk_zero());
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 16 * mt + 4 * q + r, c = 16 * nt + li;
      if (d < D && c < k) Ps[d * KS + c] = acc[r];
    }
  }
  __syncthreads();
  for (int tile = wv; tile < FT * NT; tile += WK_WAVES) {
    const int mt = tile / NT, nt = tile - mt * NT;
    const wk_f4 acc = wk_tile(Xs, XS, 1, F, Ps, KS, 1, k, D, mt, nt, q, li, wk_zero());
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 16 * mt + 4 * q + r, c = 16 * nt + li;
      if (f < F && c < k) Zs[f * KS + c] = acc[r];
    }
  }
  __syncthreads();
}

template <int MF>
__device__ __forceinline__ void wk_fm_stage_w(const float* __restrict__ W, int F, int k, float* Ws) {
  constexpr int KS = wk_pad(MF);
  for (int e = threadIdx.x; e < F * k; e += WK_THREADS) {
    const int f = e / k;
    Ws[f * KS + (e - f * k)] = W[e];
  }
}

// grid min(B, WK_MAXGRID).  MF: the class's bound on F and k.
template <int MF>
__global__ __launch_bounds__(WK_THREADS) void wk_fm_fwd_kernel(const float* __restrict__ x, int64_t xs, const float* __restrict__ W,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               int64_t B, int F, int D, int k, float* __restrict__ out, int64_t os,
                                                               float* __restrict__ stats) {
  constexpr int XS = wk_pad(WK_MAXD), KS = wk_pad(MF), NE = MF * MF / WK_THREADS;
  __shared__ float Xs[MF * XS];
  __shared__ float Ws[MF * KS];
  __shared__ float Ps[WK_MAXD * KS];
  __shared__ float Zs[MF * KS];
  __shared__ float red[2 * WK_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int n = F * k;
  const float inv_n = 1.0f / (float)n;
  wk_fm_stage_w<MF>(W, F, k, Ws);
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();  // (the previous sample's Xs and Zs have been read)
    wk_stage(x + b * xs, F, D, Xs, XS);
    __syncthreads();
    wk_fm_pz(Xs, XS, Ws, Ps, Zs, KS, F, D, k, wv, q, li);
    float z[NE];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = t + WK_THREADS * j;
      const int f = e / k;
      z[j] = e < n ? Zs[f * KS + (e - f * k)] : 0.f;
      sum += z[j];
    }
    const float mean = wk_block_sum(sum, red, wv, lane) * inv_n;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const float d = t + WK_THREADS * j < n ? z[j] - mean : 0.f;
      sq = fmaf(d, d, sq);
    }
    const float rstd = 1.0f / sqrtf(wk_block_sum(sq, red + WK_WAVES, wv, lane) * inv_n + eps);
    if (t == 0) {
      stats[b * 2] = mean;
      stats[b * 2 + 1] = rstd;
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = t + WK_THREADS * j;
      if (e < n) out[b * os + e] = fmaf((z[j] - mean) * rstd, gamma[e], beta[e]);
    }
  }
}

// floats of one workgroup's row of partial sums: [dW F k | dgamma F k | dbeta F k]
__host__ __device__ static inline size_t wk_fm_row_len(int F, int k) { return 3 * (size_t)F * k; }

template <int MF>
__global__ __launch_bounds__(WK_THREADS) void wk_fm_bwd_kernel(const float* __restrict__ gout, int64_t gs, const float* __restrict__ x, int64_t xs,
                                                               const float* __restrict__ W, const float* __restrict__ gamma,
                                                               const float* __restrict__ stats, int64_t B, int F, int D, int k,
                                                               float* __restrict__ gx, int64_t gxs, float* __restrict__ parts) {
  constexpr int XS = wk_pad(WK_MAXD), KS = wk_pad(MF), NE = MF * MF / WK_THREADS;
  constexpr int TPW = (MF / 16) * (MF / 16) / WK_WAVES;  // dW tiles a wave owns
  __shared__ float Xs[MF * XS];
  __shared__ float Ws[MF * KS];
  __shared__ float Ps[WK_MAXD * KS];
  __shared__ float dPs[WK_MAXD * KS];
  __shared__ float Zs[MF * KS];  // Z, then gZ
  __shared__ float red[2 * WK_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int n = F * k;
  const float inv_n = 1.0f / (float)n;
  const int NT = (k + 15) >> 4, DT = (D + 15) >> 4, FT = (F + 15) >> 4;
  wk_fm_stage_w<MF>(W, F, k, Ws);
  float gam[NE], acc_g[NE], acc_b[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int e = t + WK_THREADS * j;
    gam[j] = e < n ? gamma[e] : 0.f;
    acc_g[j] = acc_b[j] = 0.f;
  }
  wk_f4 accw[TPW];
#pragma unroll
  for (int a = 0; a < TPW; ++a) accw[a] = wk_zero();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();
    wk_stage(x + b * xs, F, D, Xs, XS);
    __syncthreads();
    wk_fm_pz(Xs, XS, Ws, Ps, Zs, KS, F, D, k, wv, q, li);
    const float mean = stats[b * 2], rstd = stats[b * 2 + 1];
    float zh[NE], gy[NE];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = t + WK_THREADS * j;
      const int f = e / k;
      const bool ok = e < n;
      zh[j] = ok ? (Zs[f * KS + (e - f * k)] - mean) * rstd : 0.f;
      const float g = ok ? gout[b * gs + e] : 0.f;
      acc_g[j] = fmaf(g, zh[j], acc_g[j]);
      acc_b[j] += g;
      gy[j] = g * gam[j];
      s1 += gy[j];
      s2 = fmaf(gy[j], zh[j], s2);
    }
    s1 = tzr_wave_sum(s1);
    s2 = tzr_wave_sum(s2);
    if (lane == 0) red[wv] = s1, red[WK_WAVES + wv] = s2;
    __syncthreads();
    s1 = (((red[0] + red[1]) + red[2]) + red[3]) * inv_n;
    s2 = (((red[4] + red[5]) + red[6]) + red[7]) * inv_n;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = t + WK_THREADS * j;
      const int f = e / k;
      if (e < n) Zs[f * KS + (e - f * k)] = rstd * ((gy[j] - s1) - zh[j] * s2);  // gZ (the thread's own elements)
    }
    __syncthreads();
    // dP = X^T gZ
    for (int tile = wv; tile < DT * NT; tile += WK_WAVES) {
      const int mt = tile / NT, nt = tile - mt * NT;
      const wk_f4 acc = wk_tile(Xs, 1, XS, D, Zs, KS, 1, k, F, mt, nt, q, li, wk_zero());
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * mt + 4 * q + r, c = 16 * nt + li;
        if (d < D && c < k) dPs[d * KS + c] = acc[r];
      }
    }
    __syncthreads();
    // gX = gZ P^T + W dP^T
    for (int tile = wv; tile < FT * DT; tile += WK_WAVES) {
      const int mt = tile / DT, nt = tile - mt * DT;
      wk_f4 acc = wk_tile(Zs, KS, 1, F, Ps, 1, KS, D, k, mt, nt, q, li, wk_zero());
      acc = wk_tile(Ws, KS, 1, F, dPs, 1, KS, D, k, mt, nt, q, li, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * mt + 4 * q + r, d = 16 * nt + li;
        if (f < F && d < D) gx[b * gxs + f * D + d] = acc[r];
      }
    }
    // dW += X dP
#pragma unroll
    for (int a = 0; a < TPW; ++a) {
      const int tile = wv + WK_WAVES * a;
      if (tile < FT * NT) {  // (uniform)
        const int mt = tile / NT, nt = tile - mt * NT;
        accw[a] = wk_tile(Xs, XS, 1, F, dPs, KS, 1, k, D, mt, nt, q, li, accw[a]);
      }
    }
  }
  float* pr = parts + (size_t)blockIdx.x * wk_fm_row_len(F, k);
#pragma unroll
  for (int a = 0; a < TPW; ++a) {
    const int tile = wv + WK_WAVES * a;
    if (tile < FT * NT) {
      const int mt = tile / NT, nt = tile - mt * NT;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * mt + 4 * q + r, c = 16 * nt + li;
        if (f < F && c < k) pr[f * k + c] = accw[a][r];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int e = t + WK_THREADS * j;
    if (e < n) {
      pr[n + e] = acc_g[j];
      pr[2 * n + e] = acc_b[j];
    }
  }
}

// ---- mix ------------------------------------------------------------------------------------------------------------

// Wc [F, Fo] into Wcs (row stride WS); wr null: the identity residual (F == Fo)
__device__ __forceinline__ void wk_mix_stage_w(const float* __restrict__ wl, const float* __restrict__ wr, int F, int Ff, int Fl, float* Wcs, int WS) {
  const int Fo = Ff + Fl;
  for (int e = threadIdx.x; e < F * Fo; e += WK_THREADS) {
    const int f = e / Fo, o = e - f * Fo;
    float v = wr ? wr[e] : (f == o ? 1.f : 0.f);
    if (o >= Ff) v += wl[f * Fl + (o - Ff)];
    Wcs[f * WS + o] = v;
  }
}

// pre [Fo, D] -> Pre (row stride XS); a barrier after it
__device__ __forceinline__ void wk_mix_pre(const float* Xs, float* Pre, int XS, const float* Wcs, int WS, const float* __restrict__ fm, int F, int D,
                                           int Ff, int Fo, int wv, int q, int li) {
  const int OT = (Fo + 15) >> 4, DT = (D + 15) >> 4;
  for (int tile = wv; tile < OT * DT; tile += WK_WAVES) {
    const int mt = tile / DT, nt = tile - mt * DT;
    const wk_f4 acc = wk_tile(Wcs, 1, WS, Fo, Xs, XS, 1, D, F, mt, nt, q, li, wk_zero());
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 16 * mt + 4 * q + r, d = 16 * nt + li;
      if (o < Fo && d < D) Pre[o * XS + d] = o < Ff ? fm[o * D + d] + acc[r] : acc[r];
    }
  }
  __syncthreads();
}

// grid min(B, WK_MAXGRID).  MF: the class's bound on F and Fo.
template <int MF>
__global__ __launch_bounds__(WK_THREADS) void wk_mix_fwd_kernel(const float* __restrict__ x, int64_t xs, const float* __restrict__ fm, int64_t fms,
                                                                const float* __restrict__ wl, const float* __restrict__ wr,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                int64_t B, int F, int D, int Ff, int Fl, float* __restrict__ out, int64_t os,
                                                                float* __restrict__ stats) {
  constexpr int XS = wk_pad(WK_MAXD), WS = wk_pad(MF);
  __shared__ float Xs[MF * XS];
  __shared__ float Pre[MF * XS];
  __shared__ float Wcs[MF * WS];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int Fo = Ff + Fl;
  const float inv_d = 1.0f / (float)D;
  wk_mix_stage_w(wl, wr, F, Ff, Fl, Wcs, WS);
  const bool ok0 = lane < D, ok1 = lane + 64 < D;
  const float g0 = ok0 ? gamma[lane] : 0.f, g1 = ok1 ? gamma[lane + 64] : 0.f;
  const float b0 = ok0 ? beta[lane] : 0.f, b1 = ok1 ? beta[lane + 64] : 0.f;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();  // (the previous sample's Xs and Pre have been read)
    wk_stage(x + b * xs, F, D, Xs, XS);
    __syncthreads();
    wk_mix_pre(Xs, Pre, XS, Wcs, WS, fm + b * fms, F, D, Ff, Fo, wv, q, li);
    for (int o = wv; o < Fo; o += WK_WAVES) {
      const float v0 = ok0 ? Pre[o * XS + lane] : 0.f, v1 = ok1 ? Pre[o * XS + lane + 64] : 0.f;
      const float mean = tzr_wave_sum(v0 + v1) * inv_d;
      const float d0 = ok0 ? v0 - mean : 0.f, d1 = ok1 ? v1 - mean : 0.f;
      const float rstd = 1.0f / sqrtf(tzr_wave_sum(fmaf(d1, d1, d0 * d0)) * inv_d + eps);
      if (lane == 0) {
        stats[(b * Fo + o) * 2] = mean;
        stats[(b * Fo + o) * 2 + 1] = rstd;
      }
      if (ok0) out[b * os + o * D + lane] = fmaf(d0 * rstd, g0, b0);
      if (ok1) out[b * os + o * D + lane + 64] = fmaf(d1 * rstd, g1, b1);
    }
  }
}

// floats of one workgroup's row of partial sums: [dWr F Fo | dWl F Fl | dgamma D | dbeta D]
__host__ __device__ static inline size_t wk_mix_row_len(int F, int D, int Ff, int Fl) { return (size_t)F * (Ff + Fl) + (size_t)F * Fl + 2 * (size_t)D; }

template <int MF>
__global__ __launch_bounds__(WK_THREADS) void wk_mix_bwd_kernel(const float* __restrict__ gout, int64_t gs, const float* __restrict__ x, int64_t xs,
                                                                const float* __restrict__ fm, int64_t fms, const float* __restrict__ wl,
                                                                const float* __restrict__ wr, const float* __restrict__ gamma,
                                                                const float* __restrict__ stats, int64_t B, int F, int D, int Ff, int Fl,
                                                                float* __restrict__ gx, int64_t gxs, float* __restrict__ gfm, int64_t gfs,
                                                                float* __restrict__ parts) {
  constexpr int XS = wk_pad(WK_MAXD), WS = wk_pad(MF);
  constexpr int TPW = (MF / 16) * (MF / 16) / WK_WAVES;  // dWc tiles a wave owns
  __shared__ float Xs[MF * XS];
  __shared__ float Pre[MF * XS];  // pre, then gpre; at the end the waves' dgamma / dbeta
  __shared__ float Wcs[MF * WS];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int Fo = Ff + Fl;
  const float inv_d = 1.0f / (float)D;
  const int FT = (F + 15) >> 4, OT = (Fo + 15) >> 4, DT = (D + 15) >> 4;
  wk_mix_stage_w(wl, wr, F, Ff, Fl, Wcs, WS);
  const bool ok0 = lane < D, ok1 = lane + 64 < D;
  const float g0 = ok0 ? gamma[lane] : 0.f, g1 = ok1 ? gamma[lane + 64] : 0.f;
  float ag0 = 0.f, ag1 = 0.f, ab0 = 0.f, ab1 = 0.f;
  wk_f4 accw[TPW];
#pragma unroll
  for (int a = 0; a < TPW; ++a) accw[a] = wk_zero();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();
    wk_stage(x + b * xs, F, D, Xs, XS);
    __syncthreads();
    wk_mix_pre(Xs, Pre, XS, Wcs, WS, fm + b * fms, F, D, Ff, Fo, wv, q, li);
    for (int o = wv; o < Fo; o += WK_WAVES) {
      const float mean = stats[(b * Fo + o) * 2], rstd = stats[(b * Fo + o) * 2 + 1];
      const float h0 = ok0 ? (Pre[o * XS + lane] - mean) * rstd : 0.f, h1 = ok1 ? (Pre[o * XS + lane + 64] - mean) * rstd : 0.f;
      const float* go = gout + b * gs + o * D;
      const float u0 = ok0 ? go[lane] : 0.f, u1 = ok1 ? go[lane + 64] : 0.f;
      ag0 = fmaf(u0, h0, ag0), ag1 = fmaf(u1, h1, ag1);
      ab0 += u0, ab1 += u1;
      const float y0 = u0 * g0, y1 = u1 * g1;
      const float s1 = tzr_wave_sum(y0 + y1) * inv_d;
      const float s2 = tzr_wave_sum(fmaf(y1, h1, y0 * h0)) * inv_d;
      const float p0 = rstd * ((y0 - s1) - h0 * s2), p1 = rstd * ((y1 - s1) - h1 * s2);
      if (ok0) Pre[o * XS + lane] = p0;
      if (ok1) Pre[o * XS + lane + 64] = p1;
      if (o < Ff) {
        if (ok0) gfm[b * gfs + o * D + lane] = p0;
        if (ok1) gfm[b * gfs + o * D + lane + 64] = p1;
      }
    }
    __syncthreads();
    // gX = Wc gpre
    for (int tile = wv; tile < FT * DT; tile += WK_WAVES) {
      const int mt = tile / DT, nt = tile - mt * DT;
      const wk_f4 acc = wk_tile(Wcs, WS, 1, F, Pre, XS, 1, D, Fo, mt, nt, q, li, wk_zero());
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * mt + 4 * q + r, d = 16 * nt + li;
        if (f < F && d < D) gx[b * gxs + f * D + d] = acc[r];
      }
    }
    // dWc += X gpre^T
#pragma unroll
    for (int a = 0; a < TPW; ++a) {
      const int tile = wv + WK_WAVES * a;
      if (tile < FT * OT) {  // (uniform)
        const int mt = tile / OT, nt = tile - mt * OT;
        accw[a] = wk_tile(Xs, XS, 1, F, Pre, 1, XS, Fo, D, mt, nt, q, li, accw[a]);
      }
    }
  }
  float* pr = parts + (size_t)blockIdx.x * wk_mix_row_len(F, D, Ff, Fl);
#pragma unroll
  for (int a = 0; a < TPW; ++a) {
    const int tile = wv + WK_WAVES * a;
    if (tile < FT * OT) {
      const int mt = tile / OT, nt = tile - mt * OT;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * mt + 4 * q + r, o = 16 * nt + li;
        if (f < F && o < Fo) {
          pr[f * Fo + o] = accw[a][r];
          if (o >= Ff) pr[F * Fo + f * Fl + (o - Ff)] = accw[a][r];
        }
      }
    }
  }
  // dgamma, dbeta: the four waves added 0..3 through LDS: red[v][w][d]
  __syncthreads();  // (every wave has read Pre)
  float* red = Pre;
  red[(0 * WK_WAVES + wv) * WK_MAXD + lane] = ag0;
  red[(0 * WK_WAVES + wv) * WK_MAXD + lane + 64] = ag1;
  red[(1 * WK_WAVES + wv) * WK_MAXD + lane] = ab0;
  red[(1 * WK_WAVES + wv) * WK_MAXD + lane + 64] = ab1;
  __syncthreads();
  float* pv = pr + (size_t)F * Fo + (size_t)F * Fl;
  for (int e = t; e < 2 * D; e += WK_THREADS) {
    const int v = e / D, d = e - v * D;
    const float* rv = red + v * WK_WAVES * WK_MAXD + d;
    pv[e] = ((rv[0] + rv[WK_MAXD]) + rv[2 * WK_MAXD]) + rv[3 * WK_MAXD];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static inline unsigned wk_grid(int64_t B) { return (unsigned)std::min<int64_t>(B, WK_MAXGRID); }

static int wk_fm_check(int64_t B, int F, int D, int k) {
  if (B < 0 || F <= 0 || D <= 0 || k <= 0) return TZR_ERR_INVALID;
  if (F > WK_MAXF || k > WK_MAXF || D > WK_MAXD || B >= ((int64_t)1 << 30)) return TZR_ERR_UNSUPPORTED;
  return TZR_OK;
}

static int wk_mix_check(int64_t B, int F, int D, int Ff, int Fl) {
  if (B < 0 || F <= 0 || D <= 0 || Ff <= 0 || Fl <= 0) return TZR_ERR_INVALID;
  if (F > WK_MAXF || Ff > WK_MAXF || Fl > WK_MAXF || Ff + Fl > WK_MAXF || D > WK_MAXD || B >= ((int64_t)1 << 30)) return TZR_ERR_UNSUPPORTED;
  return TZR_OK;
}

extern "C" int tzr_wukong_fm_fwd(const float* d_x, int64_t x_stride, const float* d_w, const float* d_gamma, const float* d_beta, float eps,
                                 int64_t B, int F, int D, int k, float* d_out, int64_t out_stride, float* d_stats, void* stream) {
  if (const int rc = wk_fm_check(B, F, D, k)) return rc;
  if (x_stride < (int64_t)F * D || out_stride < (int64_t)F * k) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_x || !d_w || !d_gamma || !d_beta || !d_out || !d_stats) return TZR_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (F <= 32 && k <= 32)
    hipLaunchKernelGGL((wk_fm_fwd_kernel<32>), dim3(wk_grid(B)), dim3(WK_THREADS), 0, st, d_x, x_stride, d_w, d_gamma, d_beta, eps, B, F, D, k, d_out,
                       out_stride, d_stats);
  else
    hipLaunchKernelGGL((wk_fm_fwd_kernel<64>), dim3(wk_grid(B)), dim3(WK_THREADS), 0, st, d_x, x_stride, d_w, d_gamma, d_beta, eps, B, F, D, k, d_out,
                       out_stride, d_stats);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_wukong_fm_bwd_workspace(int64_t B, int F, int D, int k) {
  if (wk_fm_check(B, F, D, k) != TZR_OK) return 256;
  return (size_t)wk_grid(B) * wk_fm_row_len(F, k) * sizeof(float) + 256;
}

extern "C" int tzr_wukong_fm_bwd(const float* d_gout, int64_t gout_stride, const float* d_x, int64_t x_stride, const float* d_w,
                                 const float* d_gamma, const float* d_stats, int64_t B, int F, int D, int k, float* d_gx, int64_t gx_stride,
                                 float* d_dparams, void* ws, size_t ws_size, void* stream) {
  if (const int rc = wk_fm_check(B, F, D, k)) return rc;
  if (gout_stride < (int64_t)F * k || x_stride < (int64_t)F * D || gx_stride < (int64_t)F * D) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_gout || !d_x || !d_w || !d_gamma || !d_stats || !d_gx || !d_dparams) return TZR_ERR_INVALID;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_size < tzr_wukong_fm_bwd_workspace(B, F, D, k) - 256) return TZR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned G = wk_grid(B);
  float* parts = static_cast<float*>(ws);
  if (F <= 32 && k <= 32)
    hipLaunchKernelGGL((wk_fm_bwd_kernel<32>), dim3(G), dim3(WK_THREADS), 0, st, d_gout, gout_stride, d_x, x_stride, d_w, d_gamma, d_stats, B, F, D, k,
                       d_gx, gx_stride, parts);
  else
    hipLaunchKernelGGL((wk_fm_bwd_kernel<64>), dim3(G), dim3(WK_THREADS), 0, st, d_gout, gout_stride, d_x, x_stride, d_w, d_gamma, d_stats, B, F, D, k,
                       d_gx, gx_stride, parts);
  TZR_CHECK_LAUNCH();
  const int N = (int)wk_fm_row_len(F, k);
  hipLaunchKernelGGL((tzr_parts_sum_finish_kernel<>), dim3((unsigned)((N + TZR_WAVE - 1) / TZR_WAVE)), dim3(TZR_FIN_THREADS), 0, st,
                     (const float*)parts, (int)G, N, d_dparams);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_wukong_mix_fwd(const float* d_x, int64_t x_stride, const float* d_fm, int64_t fm_stride, const float* d_wl, const float* d_wr,
                                  const float* d_gamma, const float* d_beta, float eps, int64_t B, int F, int D, int Ff, int Fl, float* d_out,
                                  int64_t out_stride, float* d_stats, void* stream) {
  if (const int rc = wk_mix_check(B, F, D, Ff, Fl)) return rc;
  const int Fo = Ff + Fl;
  if (x_stride < (int64_t)F * D || fm_stride < (int64_t)Ff * D || out_stride < (int64_t)Fo * D || (!d_wr && F != Fo)) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_x || !d_fm || !d_wl || !d_gamma || !d_beta || !d_out || !d_stats) return TZR_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (F <= 32 && Fo <= 32)
    hipLaunchKernelGGL((wk_mix_fwd_kernel<32>), dim3(wk_grid(B)), dim3(WK_THREADS), 0, st, d_x, x_stride, d_fm, fm_stride, d_wl, d_wr, d_gamma, d_beta,
                       eps, B, F, D, Ff, Fl, d_out, out_stride, d_stats);
  else
    hipLaunchKernelGGL((wk_mix_fwd_kernel<64>), dim3(wk_grid(B)), dim3(WK_THREADS), 0, st, d_x, x_stride, d_fm, fm_stride, d_wl, d_wr, d_gamma, d_beta,
                       eps, B, F, D, Ff, Fl, d_out, out_stride, d_stats);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_wukong_mix_bwd_workspace(int64_t B, int F, int D, int Ff, int Fl) {
  if (wk_mix_check(B, F, D, Ff, Fl) != TZR_OK) return 256;
  return (size_t)wk_grid(B) * wk_mix_row_len(F, D, Ff, Fl) * sizeof(float) + 256;
}

extern "C" int tzr_wukong_mix_bwd(const float* d_gout, int64_t gout_stride, const float* d_x, int64_t x_stride, const float* d_fm, int64_t fm_stride,
                                  const float* d_wl, const float* d_wr, const float* d_gamma, const float* d_stats, int64_t B, int F, int D, int Ff,
                                  int Fl, float* d_gx, int64_t gx_stride, float* d_gfm, int64_t gfm_stride, float* d_dparams, void* ws,
                                  size_t ws_size, void* stream) {
  if (const int rc = wk_mix_check(B, F, D, Ff, Fl)) return rc;
  const int Fo = Ff + Fl;
  if (gout_stride < (int64_t)Fo * D || x_stride < (int64_t)F * D || fm_stride < (int64_t)Ff * D || gx_stride < (int64_t)F * D ||
      gfm_stride < (int64_t)Ff * D || (!d_wr && F != Fo))
    return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_gout || !d_x || !d_fm || !d_wl || !d_gamma || !d_stats || !d_gx || !d_gfm || !d_dparams) return TZR_ERR_INVALID;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_size < tzr_wukong_mix_bwd_workspace(B, F, D, Ff, Fl) - 256) return TZR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned G = wk_grid(B);
  float* parts = static_cast<float*>(ws);
  if (F <= 32 && Fo <= 32)
    hipLaunchKernelGGL((wk_mix_bwd_kernel<32>), dim3(G), dim3(WK_THREADS), 0, st, d_gout, gout_stride, d_x, x_stride, d_fm, fm_stride, d_wl, d_wr,
                       d_gamma, d_stats, B, F, D, Ff, Fl, d_gx, gx_stride, d_gfm, gfm_stride, parts);
  else
    hipLaunchKernelGGL((wk_mix_bwd_kernel<64>), dim3(G), dim3(WK_THREADS), 0, st, d_gout, gout_stride, d_x, x_stride, d_fm, fm_stride, d_wl, d_wr,
                       d_gamma, d_stats, B, F, D, Ff, Fl, d_gx, gx_stride, d_gfm, gfm_stride, parts);
  TZR_CHECK_LAUNCH();
  const int N = (int)wk_mix_row_len(F, D, Ff, Fl);
  hipLaunchKernelGGL((tzr_parts_sum_finish_kernel<>), dim3((unsigned)((N + TZR_WAVE - 1) / TZR_WAVE)), dim3(TZR_FIN_THREADS), 0, st,
                     (const float*)parts, (int)G, N, d_dparams);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
