// The low-rank cross network of Deep & Cross v2, the whole stack of L layers in one launch forward and two launches backward.
// Replaces CrossV2.forward of the reference (tzrec/modules/interaction.py:135-180: per layer two library GEMMs, a bias add, a
// multiply and an add, about ten more launches in autograd) for fp32 rows of any width D <= 1024, any rank r <= 64, L <= 8:
//
//   forward    x_0 = x;  t_l = x_l U_l^T [B, r];  y_l = t_l V_l^T + c_l [B, D];  x_{l+1} = x_0 * y_l + x_l;  out = x_L
//   backward   for l = L-1 .. 0, g = dL/dx_{l+1}:   dy = g * x_0;  dx0 += g * y_l (y_l again from the saved t_l: K = r);
//              dc_l = sum_b dy;  dV_l = sum_b dy^T t_l;  dt = dy V_l;  dU_l = sum_b dt^T x_l;  g <- g + dt U_l;   dx = g_0 + dx0
//
// Rows.  A workgroup of 256 threads takes a block of 16 rows (one MFMA M-tile) at a time in a grid-stride loop.  Sixteen and
// not 32: x_0 and x_l (backward: x_0, g and dx0) stay in registers in accumulator layout for every layer, 4 floats per lane
// and owned tile each, and at D = 1024 a wave owns 16 tiles -- 128 (192) registers for 16 rows, twice that for 32, which
// would leave no room for the accumulators.  Every product is on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain):
//   t_l  [16, r]   A = x_l from LDS, B = U_l from memory (L2); the four waves split K = D into four contiguous ranges (each
//                  on eight interleaved accumulator chains, added pairwise) and their partial tiles are added 0..3 through LDS
//   y_l  [16, D]   A = t_l from LDS, B = V_l from memory, K = r; the D / 16 output tiles go round-robin over the waves (wave w
//                  owns the tiles w, w + 4, .. in every layer), four accumulators at a time
//   epilogue       fmaf(x_0, acc + c_l, x_l) on the accumulator layout; the result goes to LDS only as the next layer's A
//                  operand, and to memory only as the saved copy (x_1 .. x_{L-1}) or as the output (x_L)
// The backward's row pass has the same shape: dy goes to LDS as the A operand of dt = dy V_l (split-K as t_l), dt as the A
// operand of g + dt U_l (the accumulators start at g).  It writes dx, and per layer dy_l [B, D] and dt_l [B, r] into the
// workspace.  The weight-gradient pass owns its outputs: workgroup (d-tile, V or U, layer) of 512 threads holds the 16 x r
// (r x 16) strip of dV_l (dU_l) in accumulators over the WHOLE batch, its eight waves taking the 4-row steps w, w + 8, ..,
// and adds the waves 0..7 through LDS; the V workgroups also add the columns of dy_l for dc_l.  No partial rows, no finish.
//
// A tail in B, D or r is a zero operand: the address clamped to a valid element, the value selected, never multiplied in.
// Loads and stores of rows are single floats: 4-byte alignment, any row stride >= D.
//
// LDS.  The emulator's __shared__ is a function-local static, so the arrays are static and sized by a template class over D
// (MD = 256, 512, 1024; r always 64).  Row strides: MD + 2 and 66 floats -- the A operand read of a wave is "16 rows x 4
// consecutive columns", ds_read_b32 is served in two halves of 32 lanes (16 rows x 2 columns) on 32 banks, and with a stride
// of 2 mod 32 those 32 addresses fall on 32 different banks.
//                       x_l / dy       partial t / dt    t / dt     total     workgroups per CU (160 KB)   registers (x_0, x_l | g, dx0, 4 acc)
//   rows fwd   256      16.1 KB        16.5 KB           4.1 KB     36.7 KB   4                            32 + 16
//   rows bwd   256      16.1 KB        16.5 KB           4.1 KB     36.7 KB   4                            48 + 16
//   rows fwd   512      32.1 KB        16.5 KB           4.1 KB     52.7 KB   3                            64 + 16
//   rows bwd   512      32.1 KB        16.5 KB           4.1 KB     52.7 KB   3                            96 + 16
//   rows fwd   1024     64.1 KB        16.5 KB           4.1 KB     84.7 KB   1                            128 + 16
//   rows bwd   1024     64.1 KB        16.5 KB           4.1 KB     84.7 KB   1                            192 + 16
//   wgrad               the eight waves' strips 32 KB + column sums 2 KB = 34 KB, 16 accumulator registers
// (the compiler's totals per kernel: NOTES.md).  What the static arrays cost: a D = 33 shape reserves the 256-wide rows.
//
// Reduction order.  t_l and dt_l: a wave its k range on eight interleaved chains added as a fixed tree, the waves 0..3.
// dV_l, dU_l, dc_l: a wave its 4-row steps in order (dc_l: a lane its rows on four interleaved chains, added pairwise), the
// waves 0..7 (dc_l: then the four row residues 0..3).  A function of (B, D, r, L) alone; no atomics; two runs are bit-equal.
#include "tzr_common.h"

#define CV_THREADS 256
#define CV_WAVES (CV_THREADS / TZR_WAVE)
#define CV_ROWS 16
#define CV_MAXDIM 1024
#define CV_MAXR 64
#define CV_MAXL 8
#define CV_MAXGRID 512  // workgroups of a row pass: 512 x 16 rows in flight at a time
#define CV_RS (CV_MAXR + 2)
#define CV_NT (CV_MAXR / 16)
#define CV_CHAINS 8  // independent accumulators of a wave over its range of K = D
#define CV_WG_THREADS 512
#define CV_WG_WAVES (CV_WG_THREADS / TZR_WAVE)

typedef float cv_f4 __attribute__((ext_vector_type(4)));

struct CvParams {  // the layers' parameters: L separate [r, D], [D, r] and [D] tensors, passed by value
  const float* u[CV_MAXL];
  const float* v[CV_MAXL];
  const float* c[CV_MAXL];
};

__device__ __forceinline__ cv_f4 cv_zero() {
  cv_f4 z = {0.f, 0.f, 0.f, 0.f};
  return z;
}

// The partial [16, r] tile row of A W over the wave's quarter of K = D, into Tp[wv]: A(i, k) = Xs[i XS + k] (LDS), W(k, j) =
// W[k wks + j wjs] (memory), j < R.  The same code is t_l = x_l U_l^T (wks = 1, wjs = D) and dt = dy V_l (wks = R, wjs = 1).
// One n-tile at a time on CV_CHAINS accumulators: the 4-column steps c, c + 8, .. of the range form chain c, and the eight
// chains are added pairwise: eight independent MFMAs cover the 40-cycle latency of a dependent one, and a chain is D / 32
// additions long, not D / 4 (the bias gradient at (3, 1024, 64, 8): 5.7 -> 5.4 x the literal form's distance to float64).
__device__ __forceinline__ void cv_split_k(const float* Xs, int XS, const float* __restrict__ W, int wks, int wjs, int D, int R, float* Tp, int wv,
                                           int q, int li) {
  const int NT = (R + 15) >> 4;
  const int kw = 4 * ((((D + 3) >> 2) + CV_WAVES - 1) / CV_WAVES);  // k per wave: a multiple of 4
  const int kb = wv * kw, ke = min(D, kb + kw);
  float* tp = Tp + wv * CV_ROWS * CV_RS;
#pragma unroll 1
  for (int nt = 0; nt < NT; ++nt) {
    const int j = 16 * nt + li;
    const bool jok = j < R;
    cv_f4 acc[CV_CHAINS];
#pragma unroll
    for (int c = 0; c < CV_CHAINS; ++c) acc[c] = cv_zero();
    for (int k0 = kb; k0 < ke; k0 += 4 * CV_CHAINS) {
#pragma unroll
      for (int c = 0; c < CV_CHAINS; ++c) {
        const int k = k0 + 4 * c + q;
        const bool kok = k < ke, ok = kok && jok;  // (the lane is row li of A and column j of W)
        const float a = Xs[li * XS + (kok ? k : 0)];
        const float b = W[ok ? (size_t)k * wks + (size_t)j * wjs : 0];
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kok ? a : 0.f, ok ? b : 0.f, acc[c], 0, 0, 0);
      }
    }
    const cv_f4 sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
    for (int r = 0; r < 4; ++r) tp[(4 * q + r) * CV_RS + j] = sum[r];
  }
}

// Ts[16, 16 NT] = the four waves' partial tiles added 0..3; rows and columns that exist also to out [B, R] (nullable)
__device__ __forceinline__ void cv_join_k(const float* Tp, float* Ts, int R, float* __restrict__ out, int64_t b0, int64_t B) {
  const int W = ((R + 15) >> 4) * 16;
  for (int e = threadIdx.x; e < CV_ROWS * W; e += CV_THREADS) {
    const int row = e / W, col = e - row * W;
    const float* p = Tp + row * CV_RS + col;
    const float v = ((p[0] + p[CV_ROWS * CV_RS]) + p[2 * CV_ROWS * CV_RS]) + p[3 * CV_ROWS * CV_RS];
    Ts[row * CV_RS + col] = v;
    if (out && col < R && b0 + row < B) out[(b0 + row) * R + col] = v;
  }
}

// acc[u] += Ts[16, R] W over K = R for the wave's tiles wv + 4 (c0 + u), u = 0..3: W(k, j) = W[k wks + j wjs], j < D
__device__ __forceinline__ void cv_tiles_r(const float* Ts, const float* __restrict__ W, int wks, int wjs, int D, int R, int c0, int wv, int q, int li,
                                           cv_f4* acc) {
  const int DT = (D + 15) >> 4;
  for (int k0 = 0; k0 < R; k0 += 4) {
    const int k = k0 + q;
    const bool kok = k < R;
    const int kc = kok ? k : 0;
    const float a = kok ? Ts[li * CV_RS + kc] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tile = wv + CV_WAVES * (c0 + u);
      if (tile < DT) {  // (uniform)
        const int j = 16 * tile + li;
        const bool ok = kok && j < D;
        const float b = W[ok ? (size_t)kc * wks + (size_t)j * wjs : 0];
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok ? b : 0.f, acc[u], 0, 0, 0);
      }
    }
  }
}

// grid min(B / 16 rounded up, CV_MAXGRID).  MD: the class's bound on D.  xsave [L-1, B, D] and tsave [L, B, R]: nullable.
template <int MD>
__global__ __launch_bounds__(CV_THREADS) void tzr_cross_v2_fwd_kernel(const float* __restrict__ x, int64_t xs, CvParams P, int L, int64_t B, int D,
                                                                      int R, float* __restrict__ y, int64_t ys, float* __restrict__ xsave,
                                                                      float* __restrict__ tsave) {
  constexpr int XS = MD + 2, TPW = MD / 16 / CV_WAVES;
  __shared__ float Xs[CV_ROWS * XS];
  __shared__ float Tp[CV_WAVES * CV_ROWS * CV_RS];
  __shared__ float Ts[CV_ROWS * CV_RS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int DT = (D + 15) >> 4;
  const int64_t nblk = (B + CV_ROWS - 1) / CV_ROWS;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t b0 = blk * CV_ROWS;
    cv_f4 x0[TPW], xl[TPW];
#pragma unroll
    for (int a = 0; a < TPW; ++a) {
      const int tile = wv + CV_WAVES * a, col = 16 * tile + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * q + r;
        const bool ok = col < D && b0 + row < B;
        const float v = ok ? x[(b0 + row) * xs + col] : 0.f;
        x0[a][r] = xl[a][r] = v;
        if (tile < DT) Xs[row * XS + col] = v;  // (the previous block's reads of Xs lie behind two barriers)
      }
    }
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
      const bool last = l == L - 1;
      __syncthreads();
      cv_split_k(Xs, XS, P.u[l], 1, D, D, R, Tp, wv, q, li);
      __syncthreads();
      cv_join_k(Tp, Ts, R, tsave ? tsave + (size_t)l * B * R : nullptr, b0, B);
      __syncthreads();
      const float* cl = P.c[l];
      float* xo = last ? nullptr : (xsave ? xsave + (size_t)l * B * D : nullptr);
#pragma unroll
      for (int c0 = 0; c0 < TPW; c0 += 4) {
        cv_f4 acc[4] = {cv_zero(), cv_zero(), cv_zero(), cv_zero()};
        cv_tiles_r(Ts, P.v[l], 1, R, D, R, c0, wv, q, li, acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int a = c0 + u, tile = wv + CV_WAVES * a, col = 16 * tile + li;
          if (tile < DT) {  // (uniform)
            const float cv = col < D ? cl[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 4 * q + r;
              const bool ok = col < D && b0 + row < B;
              const float v = fmaf(x0[a][r], acc[u][r] + cv, xl[a][r]);
              xl[a][r] = v;
              if (!last) {
                Xs[row * XS + col] = v;  // (Xs was read before the last two barriers; a column past D holds 0)
                if (xo && ok) xo[(b0 + row) * D + col] = v;
              } else if (ok) {
                y[(b0 + row) * ys + col] = v;
              }
            }
          }
        }
      }
    }
  }
}

// The backward's row pass.  dyw [L, B, D] and dtw [L, B, R]: the workspace.
template <int MD>
__global__ __launch_bounds__(CV_THREADS) void tzr_cross_v2_bwd_rows_kernel(const float* __restrict__ gy, int64_t gs, const float* __restrict__ x,
                                                                           int64_t xs, const float* __restrict__ tsave, CvParams P, int L, int64_t B,
                                                                           int D, int R, float* __restrict__ dx, int64_t dxs,
                                                                           float* __restrict__ dyw, float* __restrict__ dtw) {
  constexpr int XS = MD + 2, TPW = MD / 16 / CV_WAVES;
  __shared__ float Xs[CV_ROWS * XS];  // dy
  __shared__ float Tp[CV_WAVES * CV_ROWS * CV_RS];
  __shared__ float Ts[CV_ROWS * CV_RS];  // t_l, then dt
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int DT = (D + 15) >> 4, W = ((R + 15) >> 4) * 16;
  const int64_t nblk = (B + CV_ROWS - 1) / CV_ROWS;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t b0 = blk * CV_ROWS;
    cv_f4 x0[TPW], g[TPW], d0[TPW];
#pragma unroll
    for (int a = 0; a < TPW; ++a) {
      const int col = 16 * (wv + CV_WAVES * a) + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * q + r;
        const bool ok = col < D && b0 + row < B;
        x0[a][r] = ok ? x[(b0 + row) * xs + col] : 0.f;
        g[a][r] = ok ? gy[(b0 + row) * gs + col] : 0.f;
        d0[a][r] = 0.f;
      }
    }
#pragma unroll 1
    for (int l = L - 1; l >= 0; --l) {
      const float* tl = tsave + (size_t)l * B * R;
      for (int e = threadIdx.x; e < CV_ROWS * W; e += CV_THREADS) {  // (the previous reads of Ts lie behind a barrier)
        const int row = e / W, col = e - row * W;
        Ts[row * CV_RS + col] = col < R && b0 + row < B ? tl[(b0 + row) * R + col] : 0.f;
      }
      __syncthreads();
      const float* cl = P.c[l];
      float* dyl = dyw + (size_t)l * B * D;
#pragma unroll
      for (int c0 = 0; c0 < TPW; c0 += 4) {
        cv_f4 acc[4] = {cv_zero(), cv_zero(), cv_zero(), cv_zero()};
        cv_tiles_r(Ts, P.v[l], 1, R, D, R, c0, wv, q, li, acc);  // y_l - c_l by the forward's instruction sequence
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int a = c0 + u, tile = wv + CV_WAVES * a, col = 16 * tile + li;
          if (tile < DT) {  // (uniform)
            const float cv = col < D ? cl[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 4 * q + r;
              const float dy = g[a][r] * x0[a][r];
              d0[a][r] = fmaf(g[a][r], acc[u][r] + cv, d0[a][r]);
              Xs[row * XS + col] = dy;  // (a row past B, a column past D: 0)
              if (col < D && b0 + row < B) dyl[(b0 + row) * D + col] = dy;
            }
          }
        }
      }
      __syncthreads();
      cv_split_k(Xs, XS, P.v[l], R, 1, D, R, Tp, wv, q, li);
      __syncthreads();
      cv_join_k(Tp, Ts, R, dtw + (size_t)l * B * R, b0, B);
      __syncthreads();
      // g <- g + dt U_l: the product from zero and ONE addition to g.  A chain that starts at g rounds r times at g's
      // magnitude; over eight layers that measured 5.4 x the literal form's distance to float64 in the bias gradient.
#pragma unroll
      for (int c0 = 0; c0 < TPW; c0 += 4) {
        cv_f4 acc[4] = {cv_zero(), cv_zero(), cv_zero(), cv_zero()};
        cv_tiles_r(Ts, P.u[l], D, 1, D, R, c0, wv, q, li, acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) g[c0 + u] += acc[u];
      }
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < TPW; ++a) {
      const int col = 16 * (wv + CV_WAVES * a) + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * q + r;
        if (col < D && b0 + row < B) dx[(b0 + row) * dxs + col] = g[a][r] + d0[a][r];
      }
    }
  }
}

// grid (D / 16 rounded up, 2, L), CV_WG_THREADS threads.  Workgroup (i, 0, l): rows 16 i .. 16 i + 15 of dV_l [D, R] = dy_l^T t_l
// and the same entries of dc_l; (i, 1, l): columns 16 i .. 16 i + 15 of dU_l [R, D] = dt_l^T x_l (x_0 = x, x_l = xsave[l - 1]).
__global__ __launch_bounds__(CV_WG_THREADS) void tzr_cross_v2_wgrad_kernel(const float* __restrict__ dyw, const float* __restrict__ dtw,
                                                                           const float* __restrict__ x, int64_t xs,
                                                                           const float* __restrict__ xsave, const float* __restrict__ tsave,
                                                                           int64_t B, int D, int R, float* __restrict__ du, float* __restrict__ dv,
                                                                           float* __restrict__ dc) {
  __shared__ float red[CV_WG_WAVES * CV_NT * 256];
  __shared__ float redc[CV_WG_WAVES * TZR_WAVE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int l = blockIdx.z, NT = (R + 15) >> 4;
  const bool isv = blockIdx.y == 0;
  const int d = 16 * blockIdx.x + li;
  const bool dok = d < D;
  // the operand whose column is d (dV: dy_l, the A operand; dU: x_l, the B operand) and the one whose column is in 0..R
  const float* pd = isv ? dyw + (size_t)l * B * D : (l == 0 ? x : xsave + (size_t)(l - 1) * B * D);
  const int64_t pds = isv || l > 0 ? (int64_t)D : xs;
  const float* pr = (isv ? tsave : dtw) + (size_t)l * B * R;
  cv_f4 acc[CV_NT];
#pragma unroll
  for (int nt = 0; nt < CV_NT; ++nt) acc[nt] = cv_zero();
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t steps = (B + 3) >> 2;
  for (int64_t s0 = wv; s0 < steps; s0 += 4 * CV_WG_WAVES) {  // four of the wave's steps at a time: their loads in flight together
    float vd[4], vr[4][CV_NT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t b = 4 * (s0 + CV_WG_WAVES * u) + q;
      const bool bok = b < B;
      const float vd0 = pd[bok && dok ? b * pds + d : 0];
      vd[u] = bok && dok ? vd0 : 0.f;
#pragma unroll
      for (int nt = 0; nt < CV_NT; ++nt) {
        const int j = 16 * nt + li;
        const bool ok = nt < NT && bok && j < R;
        const float vr0 = pr[ok ? b * R + j : 0];
        vr[u][nt] = ok ? vr0 : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      cs[u] += vd[u];  // (dc_l: four chains per lane, a step past the batch adds +0)
#pragma unroll
      for (int nt = 0; nt < CV_NT; ++nt) {
        if (nt < NT)  // (uniform)
          acc[nt] = isv ? __builtin_amdgcn_mfma_f32_16x16x4f32(vd[u], vr[u][nt], acc[nt], 0, 0, 0)
                        : __builtin_amdgcn_mfma_f32_16x16x4f32(vr[u][nt], vd[u], acc[nt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < CV_NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wv * CV_NT + nt) * 256 + r * 64 + lane] = acc[nt][r];
  redc[wv * TZR_WAVE + lane] = (cs[0] + cs[1]) + (cs[2] + cs[3]);
  __syncthreads();
  for (int e = threadIdx.x; e < NT * 256; e += CV_WG_THREADS) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < CV_WG_WAVES; ++w) v += red[w * CV_NT * 256 + e];
    const int nt = e >> 8, r = (e >> 6) & 3, ln = e & 63;
    const int i = 4 * (ln >> 4) + r, j = ln & 15;  // the tile's row and column
    if (isv) {
      const int dd = 16 * blockIdx.x + i, c = 16 * nt + j;
      if (dd < D && c < R) dv[((size_t)l * D + dd) * R + c] = v;
    } else {
      const int rr = 16 * nt + i, dd = 16 * blockIdx.x + j;
      if (rr < R && dd < D) du[((size_t)l * R + rr) * D + dd] = v;
    }
  }
  if (isv && threadIdx.x < 16 && dok) {
    float qs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < CV_WG_WAVES; ++w) v += redc[w * TZR_WAVE + 16 * k + threadIdx.x];
      qs[k] = v;
    }
    dc[(size_t)l * D + d] = ((qs[0] + qs[1]) + qs[2]) + qs[3];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static int cv_check(int64_t B, int D, int R, int L) {
  if (B < 0 || D <= 0 || R <= 0 || L <= 0) return TZR_ERR_INVALID;
  if (D > CV_MAXDIM || R > CV_MAXR || L > CV_MAXL) return TZR_ERR_UNSUPPORTED;
  return TZR_OK;
}

static int cv_params(const float* const* h_u, const float* const* h_v, const float* const* h_c, int L, CvParams* P) {
  if (!h_u || !h_v || !h_c) return TZR_ERR_INVALID;
  for (int l = 0; l < CV_MAXL; ++l) {
    P->u[l] = l < L ? h_u[l] : nullptr;
    P->v[l] = l < L ? h_v[l] : nullptr;
    P->c[l] = l < L ? h_c[l] : nullptr;
    if (l < L && (!P->u[l] || !P->v[l] || !P->c[l])) return TZR_ERR_INVALID;
  }
  return TZR_OK;
}

static inline unsigned cv_grid(int64_t B) { return (unsigned)std::min<int64_t>((B + CV_ROWS - 1) / CV_ROWS, CV_MAXGRID); }

#define CV_BY_CLASS(LAUNCH)        \
  do {                             \
    if (D <= 256) LAUNCH(256);     \
    else if (D <= 512) LAUNCH(512); \
    else LAUNCH(1024);             \
  } while (0)

extern "C" int tzr_cross_v2_fwd(const float* d_x, int64_t x_stride, const float* const* h_u, const float* const* h_v, const float* const* h_c,
                                int L, int64_t B, int D, int R, float* d_y, int64_t y_stride, float* d_xs, float* d_t, void* stream) {
  if (const int rc = cv_check(B, D, R, L)) return rc;
  if (x_stride < D || y_stride < D) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  CvParams P;
  if (!d_x || !d_y || cv_params(h_u, h_v, h_c, L, &P) != TZR_OK) return TZR_ERR_INVALID;
#define CV_FWD(MD_)                                                                                                                      \
  hipLaunchKernelGGL((tzr_cross_v2_fwd_kernel<MD_>), dim3(cv_grid(B)), dim3(CV_THREADS), 0, static_cast<hipStream_t>(stream), d_x, x_stride, P, \
                     L, B, D, R, d_y, y_stride, d_xs, d_t)
  CV_BY_CLASS(CV_FWD);
#undef CV_FWD
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_cross_v2_bwd_workspace(int64_t B, int D, int R, int L) {
  if (cv_check(B, D, R, L) != TZR_OK) return 256;
  return (size_t)L * (size_t)B * ((size_t)D + (size_t)R) * sizeof(float) + 256;
}

extern "C" int tzr_cross_v2_bwd(const float* d_grad_y, int64_t gy_stride, const float* d_x, int64_t x_stride, const float* d_xs, const float* d_t,
                                const float* const* h_u, const float* const* h_v, const float* const* h_c, int L, int64_t B, int D, int R,
                                float* d_dx, int64_t dx_stride, float* d_du, float* d_dv, float* d_dc, void* ws, size_t ws_size, void* stream) {
  if (const int rc = cv_check(B, D, R, L)) return rc;
  if (gy_stride < D || x_stride < D || dx_stride < D) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  CvParams P;
  if (!d_grad_y || !d_x || (!d_xs && L > 1) || !d_t || !d_dx || !d_du || !d_dv || !d_dc || !ws || (reinterpret_cast<uintptr_t>(ws) & 255) ||
      cv_params(h_u, h_v, h_c, L, &P) != TZR_OK)
    return TZR_ERR_INVALID;
  if (ws_size < tzr_cross_v2_bwd_workspace(B, D, R, L) - 256) return TZR_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* dyw = static_cast<float*>(ws);
  float* dtw = dyw + (size_t)L * B * D;
#define CV_BWD(MD_)                                                                                                                       \
  hipLaunchKernelGGL((tzr_cross_v2_bwd_rows_kernel<MD_>), dim3(cv_grid(B)), dim3(CV_THREADS), 0, st, d_grad_y, gy_stride, d_x, x_stride, d_t, P, \
                     L, B, D, R, d_dx, dx_stride, dyw, dtw)
  CV_BY_CLASS(CV_BWD);
#undef CV_BWD
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_cross_v2_wgrad_kernel, dim3((unsigned)((D + 15) / 16), 2u, (unsigned)L), dim3(CV_WG_THREADS), 0, st, (const float*)dyw,
                     (const float*)dtw, d_x, x_stride, d_xs, d_t, B, D, R, d_du, d_dv, d_dc);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
