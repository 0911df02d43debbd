// The compressed interaction network of xDeepFM.  Replaces CIN.forward of the reference and its autograd
// (tzrec/modules/interaction.py:183-233: per layer z = einsum("bhd,bfd->bhfd") as a [B, H F, D] tensor, a Conv1d(kernel_size=1)
// over it, autograd keeps z) for fp32, D <= 64, F <= 64, every O_i <= 256 and L <= 4 layers.  z is never built: with a column
// n = (b, d), X0[f, n] = x[b, f D + d], H_0 = F, H_{i+1} = O_i,
//
//   forward    X^{i+1}[o, n] = c_i[o] + sum_{h,f} W_i[o, h F + f] X^i[h, n] X0[f, n];   y[b, off_i + o] = sum_d X^{i+1}[o, (b, d)]
//   backward   G_i[o, n] = gy[b, off_i + o] + dX^{i+1}[o, n]                    (i = L-1 .. 0; the second term absent for i = L-1)
//              U[(h,f), n] = sum_o W_i[o, h F + f] G_i[o, n];   dX^i[h, n] = sum_f U X0[f, n];   dX0[f, n] += sum_h U X^i[h, n]
//              dW_i[o, h F + f] = sum_n G_i[o, n] X^i[h, n] X0[f, n];   dc_i[o] = sum_n G_i[o, n]
//
// are three contractions on v_mfma_f32_16x16x4_f32 (exact fp32) in which one operand is the product of two small tiles, formed
// in registers from LDS -- one multiply per MFMA and lane:
//
//   cin_fwd_kernel    ONE launch for every layer.  A workgroup holds 32 columns (whole samples; for D > 32 one sample in two
//                     passes over d): A = W_i[16 o, 4 k] from memory, B[k, n] = X^i[h, n] X0[f, n] with k = (h, 4 f4 + lane >> 4),
//                     the output tile [O_i, 32] in accumulators (wave w owns the o-tiles w, w + 4, ..).  It goes back to LDS over
//                     X^i -- the next layer's operand, and what the pooling adds over d -- and, for i < L-1, to memory: the
//                     saved state of the backward.  X^L is only pooled.
//   cin_bwd_w_kernel  dW_i and dc_i, "a workgroup owns output, walks the contraction" (gemm_rows.hip): workgroup (o-block of 64,
//                     h, part) owns dW_i[64 o, h F .. h F + F) over its part of the columns; A = G_i[16 o, 4 n], B[n, f] =
//                     X^i[h, n] X0[f, n]; its four waves split the 4-column steps and are added 0..3 at the end.  Row h = H_i of
//                     the grid is dc_i (B = 1 in column 0).  The column range is cut into S_i parts, a function of the shapes
//                     alone (until the launch has about 1024 workgroups, a layer's parts bounded in size); the parts land in the
//                     workspace and cin_bwd_finish_kernel adds them 0..S_i-1.  No atomics.
//   cin_bwd_x_kernel  dX^i and dX0.  A workgroup holds 32 columns: A = W_i^T[16 f, 4 o] from memory, B = G_i[4 o, 16 n] from
//                     LDS, U[16 f of one h, 16 n] in accumulators and consumed there: times X0 and summed over f -> dX^i[h, n]
//                     (in the lane, then over the four row groups of the tile), times X^i[h, n] -> dX0[f, n] (wave w owns the rows
//                     h = w, w + 4, ..; the four waves are added 0..3 through LDS).  dX^i overwrites X^i in place: the saved
//                     state is consumed, no temporary of its size exists.  gx is written by the last layer and added to by the
//                     others, launch after launch.
//
// Launches: 1 forward, 2 L + 1 backward.  Every sum's order is a function of the shapes alone: bit-reproducible.
// Loads and stores of x, gx, W are single floats: 4-byte alignment, any row stride >= F D.  Tails in F, D, O, B are zero operands.
#include "tzr_common.h"

#define CIN_THREADS 256
#define CIN_MAXL 4
#define CIN_MAXD 64
#define CIN_MAXF 64
#define CIN_MAXO 256
#define CIN_NC 32        // columns a workgroup of the forward / of cin_bwd_x_kernel holds
#define CIN_MAXGRID 1024  // workgroups of those launches: they loop over their units
#define CIN_X0S 48       // LDS row stride of a [k, 32] tile read four rows at a time (rows 16 banks apart)
#define CIN_WC 64        // columns of one chunk of cin_bwd_w_kernel
#define CIN_WS 80        // LDS row stride of its [n, 64] tiles
#define CIN_TARGET_WGS 1024        // cin_bwd_w_kernel: parts of the column range until a launch has about this many workgroups,
#define CIN_PART_FLOATS (512 << 10)  // while a layer's parts stay below this many floats (or 4 parts)

typedef float cin_f4 __attribute__((ext_vector_type(4)));

struct CinParams {
  const float* w[CIN_MAXL];  // W_i [O_i, H_i F]
  const float* c[CIN_MAXL];  // c_i [O_i]
  float* xs[CIN_MAXL];       // xs[i] = X^{i+1} [B, O_i, D], i < L-1 (forward: nullable, nothing is saved)
  int O[CIN_MAXL];
};

__device__ __forceinline__ cin_f4 cin_zero() {
  cin_f4 z = {0.f, 0.f, 0.f, 0.f};
  return z;
}

// grid min(units, CIN_MAXGRID): unit u = samples [u TB, u TB + TB), TB = 32 / D (1 for D > 32, then two passes over d)
__global__ __launch_bounds__(CIN_THREADS) void cin_fwd_kernel(const float* __restrict__ x, int64_t xs, CinParams P, int L, int64_t B, int F,
                                                              int D, float* __restrict__ y, int64_t ys) {
  __shared__ float Xs[CIN_MAXO * CIN_NC];   // X^i[h][c]
  __shared__ float X0s[CIN_MAXF * CIN_X0S];  // X0[f][c], rows F .. 4 ceil(F / 4) zero
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int TB = D > CIN_NC ? 1 : CIN_NC / D;
  const int passes = D > CIN_NC ? 2 : 1;
  const int F4 = (F + 3) >> 2;
  const int64_t units = (B + TB - 1) / TB;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t b0 = u * TB;
    for (int ps = 0; ps < passes; ++ps) {
      const int d0 = ps * CIN_NC;
      const int DW = passes == 1 ? D : (ps == 0 ? CIN_NC : D - CIN_NC);
      const int ncu = TB * DW;  // columns in use
      __syncthreads();          // (the previous unit's pooling has read Xs)
      {
        const int c = t & (CIN_NC - 1);
        const int s = c / DW, dd = d0 + c - s * DW;
        const bool ok = c < ncu && b0 + s < B;
        const float* xr = x + (b0 + s) * xs + dd;
        for (int f = t >> 5; f < 4 * F4; f += CIN_THREADS / CIN_NC) {
          const float v = ok && f < F ? xr[f * D] : 0.f;
          X0s[f * CIN_X0S + c] = v;
          Xs[f * CIN_NC + c] = v;
        }
      }
      __syncthreads();
      int H = F, yoff = 0;
      for (int i = 0; i < L; ++i) {
        const int O = P.O[i], K = H * F;
        const float* __restrict__ W = P.w[i];
        // two accumulators per tile, even and odd h: halves the length of each fp32 chain (H F / 2 terms) and keeps two
        // independent MFMAs in flight per tile
        cin_f4 acc[4][2], acc1[4][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[a][nt] = acc1[a][nt] = cin_zero();
        const int OT = (O + 15) >> 4;
        // this wave's o-tiles wv, wv + 4, ..: lane reads row o = 16 ot + li of W.  Rows and columns are clamped into W and the
        // value dropped afterwards (a tail loads a valid element): no branch around a load, so the loads of step s + 1 are in
        // flight while the MFMAs of step s run
        const int na = __builtin_amdgcn_readfirstlane(OT > wv ? (OT - wv + 3) >> 2 : 0);
        const float* wrow[4];
        bool wok[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int o = 16 * (wv + 4 * a) + li;
          wok[a] = a < na && o < O;
          wrow[a] = W + (size_t)(o < O ? o : O - 1) * K;
        }
        const int fq = q < F ? q : F - 1;
        float av[4], aw[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {  // step (h2, f4) = (0, 0)
          const float v = wrow[a][fq], w = wrow[a][(H > 1 ? F : 0) + fq];
          av[a] = wok[a] && q < F ? v : 0.f;
          aw[a] = wok[a] && q < F && H > 1 ? w : 0.f;
        }
        int h2 = 0, f4 = 0;
        while (h2 < H) {
          int nf4 = f4 + 1, nh2 = h2;
          if (nf4 == F4) nf4 = 0, nh2 += 2;
          const bool more = nh2 < H;  // (the last step loads its own operands again)
          const int lh = more ? nh2 : h2, lf = 4 * (more ? nf4 : f4) + q;
          const bool lodd = lh + 1 < H, lfok = lf < F;
          const int c0 = lh * F + (lfok ? lf : F - 1), c1 = c0 + (lodd ? F : 0);
          float nav[4], naw[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const float v = wrow[a][c0], w = wrow[a][c1];
            nav[a] = wok[a] && lfok ? v : 0.f;
            naw[a] = wok[a] && lfok && lodd ? w : 0.f;
          }
          const bool odd = h2 + 1 < H;  // (uniform)
          const int f = 4 * f4 + q, hj = odd ? h2 + 1 : h2;
          const float x00 = X0s[f * CIN_X0S + li], x01 = X0s[f * CIN_X0S + 16 + li];
          const float b00 = Xs[h2 * CIN_NC + li] * x00, b01 = Xs[h2 * CIN_NC + 16 + li] * x01;
          const float b10 = Xs[hj * CIN_NC + li] * x00, b11 = Xs[hj * CIN_NC + 16 + li] * x01;  // (times aw = 0 when there is no odd row)
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            if (a < na) {  // (uniform)
              acc[a][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], b00, acc[a][0], 0, 0, 0);
              acc[a][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], b01, acc[a][1], 0, 0, 0);
              acc1[a][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[a], b10, acc1[a][0], 0, 0, 0);
              acc1[a][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[a], b11, acc1[a][1], 0, 0, 0);
            }
          }
#pragma unroll
          for (int a = 0; a < 4; ++a) av[a] = nav[a], aw[a] = naw[a];
          h2 = nh2, f4 = nf4;
        }
        __syncthreads();  // every wave has read X^i
        float* __restrict__ save = i < L - 1 ? P.xs[i] : nullptr;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          if (a < na) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
              const int c = 16 * nt + li;
              const int s = c / DW, dd = d0 + c - s * DW;
              const bool ok = c < ncu && b0 + s < B;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int o = 16 * (wv + 4 * a) + 4 * q + r;
                if (o < O) {
                  const float v = (acc[a][nt][r] + acc1[a][nt][r]) + P.c[i][o];
                  Xs[o * CIN_NC + c] = v;
                  if (save && ok) save[((b0 + s) * O + o) * D + dd] = v;
                }
              }
            }
          }
        }
        __syncthreads();
        for (int e = t; e < O * TB; e += CIN_THREADS) {
          const int o = e / TB, s = e - o * TB;
          if (b0 + s < B) {
            float sum = 0.f;
            for (int dd = 0; dd < DW; ++dd) sum += Xs[o * CIN_NC + s * DW + dd];
            float* dst = y + (b0 + s) * ys + yoff + o;
            *dst = ps == 0 ? sum : *dst + sum;
          }
        }
        yoff += O;
        H = O;
        // (the next layer's loop reads Xs rows this pooling only read: no barrier needed before it; the one after its loop
        // orders the pooling before the next overwrite)
      }
    }
  }
}

// floats of one part: per layer dW_i [O_i, H_i F] then dc_i [O_i]
static inline size_t cin_total(const int* O, int L, int F) {
  size_t tot = 0;
  int H = F;
  for (int i = 0; i < L; ++i) {
    tot += (size_t)O[i] * H * F + O[i];
    H = O[i];
  }
  return tot;
}
// parts S_i of layer i's column range: a function of the shapes alone, non-decreasing in B
static inline int cin_layer_parts(int64_t B, int D, int O, int H, int F) {
  const int64_t chunks = (B * D + CIN_WC - 1) / CIN_WC;
  const int64_t base = (int64_t)((O + 63) / 64) * (H + 1);
  const int64_t want = (CIN_TARGET_WGS + base - 1) / base;
  const int64_t cap = std::max<int64_t>(4, CIN_PART_FLOATS / ((int64_t)O * H * F + O));
  return (int)std::max<int64_t>(1, std::min(std::min(want, cap), chunks));
}
static inline size_t cin_parts_floats(int64_t B, int D, const int* O, int L, int F) {
  size_t tot = 0;
  int H = F;
  for (int i = 0; i < L; ++i) {
    tot += (size_t)cin_layer_parts(B, D, O[i], H, F) * ((size_t)O[i] * H * F + O[i]);
    H = O[i];
  }
  return tot;
}

struct CinFinish {  // per layer: where its gradients start in the output, where its parts start, their size and count
  size_t out_off[CIN_MAXL], part_off[CIN_MAXL], size[CIN_MAXL];
  int S[CIN_MAXL];
  int L;
};

// grid (ceil(O / 64), H + 1, S).  xi: X^i [B, H, D] (layer 0: null, X^i = X0 from x); dxn: dX^{i+1} [B, O, D] or null.
__global__ __launch_bounds__(CIN_THREADS) void cin_bwd_w_kernel(const float* __restrict__ gy, int64_t gs, int yoff, const float* __restrict__ dxn,
                                                                const float* __restrict__ x, int64_t xs, const float* __restrict__ xi, int64_t B,
                                                                int F, int D, int H, int O, float* __restrict__ part, size_t part_stride) {
  __shared__ float Gs[CIN_WC * CIN_WS];   // G[n][o - o0]; afterwards the waves' tiles
  __shared__ float X0s[CIN_WC * CIN_WS];  // X0[n][f]
  __shared__ float Xis[CIN_WC];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int o0 = blockIdx.x * 64, h = blockIdx.y;
  const bool bias = h == H;
  const int KT = bias ? 1 : (F + 15) >> 4;
  const int64_t N = B * D;
  const int64_t chunks = (N + CIN_WC - 1) / CIN_WC;
  const int64_t per = (chunks + gridDim.z - 1) / gridDim.z;
  const int64_t ch0 = per * blockIdx.z, ch1 = ch0 + per < chunks ? ch0 + per : chunks;
  part += (size_t)blockIdx.z * part_stride;
  cin_f4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[a][k] = cin_zero();
  for (int64_t ch = ch0; ch < ch1; ++ch) {
    __syncthreads();
    {
      const int c = t & (CIN_WC - 1);
      const int64_t n = ch * CIN_WC + c;
      const bool ok = n < N;
      const int64_t b = ok ? n / D : 0;
      const int d = (int)(n - b * D);
      for (int ol = t >> 6; ol < 64; ol += CIN_THREADS / CIN_WC) {
        const int o = o0 + ol;
        float g = 0.f;
        if (ok && o < O) {
          g = gy[b * gs + yoff + o];
          if (dxn) g += dxn[(b * O + o) * D + d];
        }
        Gs[c * CIN_WS + ol] = g;
      }
      for (int f = t >> 6; f < 16 * KT; f += CIN_THREADS / CIN_WC) {
        float v;
        if (bias) v = f == 0 ? 1.f : 0.f;
        else v = ok && f < F ? x[b * xs + f * D + d] : 0.f;
        X0s[c * CIN_WS + f] = v;
      }
      if (t < CIN_WC) Xis[c] = bias ? 1.f : (!ok ? 0.f : (xi ? xi[(b * H + h) * D + d] : x[b * xs + h * D + d]));
    }
    __syncthreads();
    for (int st = wv; st < CIN_WC / 4; st += 4) {
      const int nl = 4 * st + q;
      const float xiv = Xis[nl];
      float bv[4], av[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) bv[k] = k < KT ? xiv * X0s[nl * CIN_WS + 16 * k + li] : 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = Gs[nl * CIN_WS + 16 * a + li];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < KT) acc[a][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[k], acc[a][k], 0, 0, 0);
    }
  }
  // the four waves' tiles, added 0..3, one o-tile at a time through Gs: red[w][k][r][lane]
  const int K = H * F;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) Gs[wv * 1024 + k * 256 + r * 64 + lane] = acc[a][k][r];
    __syncthreads();
    for (int e = t; e < KT * 256; e += CIN_THREADS) {
      const float v = ((Gs[e] + Gs[1024 + e]) + Gs[2048 + e]) + Gs[3072 + e];
      const int k = e >> 8, r = (e >> 6) & 3, ln = e & 63;
      const int o = o0 + 16 * a + 4 * (ln >> 4) + r, f = 16 * k + (ln & 15);
      if (o < O) {
        if (bias) {
          if (f == 0) part[(size_t)O * K + o] = v;
        } else if (f < F) {
          part[(size_t)o * K + h * F + f] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(CIN_THREADS) void cin_bwd_finish_kernel(const float* __restrict__ parts, CinFinish Fi, size_t total,
                                                                     float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * CIN_THREADS + threadIdx.x;
  if (e >= total) return;
  size_t off = Fi.out_off[0], po = Fi.part_off[0], sz = Fi.size[0];
  int S = Fi.S[0];
#pragma unroll
  for (int i = 1; i < CIN_MAXL; ++i)
    if (i < Fi.L && e >= Fi.out_off[i]) off = Fi.out_off[i], po = Fi.part_off[i], sz = Fi.size[i], S = Fi.S[i];
  const float* p = parts + po + (e - off);
  float v = p[0];
  for (int s = 1; s < S; ++s) v += p[(size_t)s * sz];
  out[e] = v;
}

// grid min(ceil(B D / 32), CIN_MAXGRID).  xi: X^i [B, H, D], overwritten by dX^i (layer 0: null; dX^0 joins gx).  first: gx is
// written, not added to.
__global__ __launch_bounds__(CIN_THREADS) void cin_bwd_x_kernel(const float* __restrict__ gy, int64_t gs, int yoff, const float* __restrict__ dxn,
                                                                const float* __restrict__ x, int64_t xs, float* __restrict__ xi,
                                                                const float* __restrict__ W, int64_t B, int F, int D, int H, int O,
                                                                float* __restrict__ gx, int64_t gxs, int first) {
  __shared__ float Gs[CIN_MAXO * CIN_X0S];  // G[o][c]; afterwards the waves' dX0 tiles
  __shared__ float X0s[CIN_MAXF * CIN_NC];  // X0[f][c]; for layer 0 afterwards dX^0[h][c]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane >> 4, li = lane & 15;
  const int64_t N = B * D;
  const int64_t tiles = (N + CIN_NC - 1) / CIN_NC;
  const int F16 = (F + 15) >> 4, O4 = (O + 3) >> 2, K = H * F;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t n0 = tile * CIN_NC;
    __syncthreads();  // (the previous tile's sums have been read)
    {
      const int c = t & (CIN_NC - 1);
      const int64_t n = n0 + c;
      const bool ok = n < N;
      const int64_t b = ok ? n / D : 0;
      const int d = (int)(n - b * D);
      for (int o = t >> 5; o < 4 * O4; o += CIN_THREADS / CIN_NC) {
        float g = 0.f;
        if (ok && o < O) {
          g = gy[b * gs + yoff + o];
          if (dxn) g += dxn[(b * O + o) * D + d];
        }
        Gs[o * CIN_X0S + c] = g;
      }
      for (int f = t >> 5; f < 16 * F16; f += CIN_THREADS / CIN_NC) X0s[f * CIN_NC + c] = ok && f < F ? x[b * xs + f * D + d] : 0.f;
    }
    __syncthreads();
    // the lane's two columns and its sixteen rows of X0
    bool nok[2];
    int64_t nb[2];
    int nd[2];
    float x0r[2][4][4], dx0[2][4][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int64_t n = n0 + 16 * nt + li;
      nok[nt] = n < N;
      nb[nt] = nok[nt] ? n / D : 0;
      nd[nt] = (int)(n - nb[nt] * D);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x0r[nt][k][r] = k < F16 ? X0s[(16 * k + 4 * q + r) * CIN_NC + 16 * nt + li] : 0.f;
          dx0[nt][k][r] = 0.f;
        }
    }
    __syncthreads();  // (layer 0 writes dX^0 over X0s)
    for (int h = wv; h < H; h += 4) {
      // X^i[h, n]: the lanes of row group 0 load (and later store dX^i[h, n] to the same address), the others get a copy
      float xiv[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        float v = 0.f;
        if (q == 0 && nok[nt]) v = xi ? xi[(nb[nt] * H + h) * D + nd[nt]] : x[nb[nt] * xs + h * D + nd[nt]];
        xiv[nt] = __shfl(v, li);
      }
      cin_f4 U[4][2];
#pragma unroll
      for (int k = 0; k < 4; ++k) U[k][0] = U[k][1] = cin_zero();
      // W_i[o, h F + 16 k + li], row and column clamped into W and the value dropped afterwards: no branch around a load, and
      // the loads of step o4 + 1 are in flight while the MFMAs of step o4 run
      const float* wp[4];
      bool wk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        wk[k] = k < F16 && 16 * k + li < F;
        wp[k] = W + (size_t)h * F + (16 * k + li < F ? 16 * k + li : F - 1);
      }
      float av[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float v = wp[k][(size_t)(q < O ? q : O - 1) * K];
        av[k] = wk[k] && q < O ? v : 0.f;
      }
      for (int o4 = 0; o4 < O4; ++o4) {
        const int o = 4 * o4 + q;
        const int on = 4 * (o4 + 1 < O4 ? o4 + 1 : o4) + q;
        float nav[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = wp[k][(size_t)(on < O ? on : O - 1) * K];
          nav[k] = wk[k] && on < O ? v : 0.f;
        }
        const float g0 = Gs[o * CIN_X0S + li], g1 = Gs[o * CIN_X0S + 16 + li];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < F16) {  // (uniform)
            U[k][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k], g0, U[k][0], 0, 0, 0);
            U[k][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k], g1, U[k][1], 0, 0, 0);
          }
#pragma unroll
        for (int k = 0; k < 4; ++k) av[k] = nav[k];
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        float dxi = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dxi = fmaf(U[k][nt][r], x0r[nt][k][r], dxi);
            dx0[nt][k][r] = fmaf(U[k][nt][r], xiv[nt], dx0[nt][k][r]);
          }
        dxi += __shfl_xor(dxi, 16);
        dxi += __shfl_xor(dxi, 32);
        if (q == 0) {
          if (!xi) X0s[h * CIN_NC + 16 * nt + li] = dxi;
          else if (nok[nt]) xi[(nb[nt] * H + h) * D + nd[nt]] = dxi;
        }
      }
    }
    __syncthreads();  // every wave has read G
    // red[w][e], e = lane | nt << 6 | r << 7 | k << 9
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) Gs[wv * 2048 + (k << 9) + (r << 7) + (nt << 6) + lane] = dx0[nt][k][r];
    __syncthreads();
    {
      // thread t: column 16 nt + li with nt = bit 6 of t, row group q, r & 1 = bit 7
      const int c = 16 * ((t >> 6) & 1) + li;
      const int64_t n = n0 + c;
      const bool ok = n < N;
      const int64_t b = ok ? n / D : 0;
      const int d = (int)(n - b * D);
      for (int e = t; e < F16 * 512; e += CIN_THREADS) {
        const int r = (e >> 7) & 3, k = e >> 9;
        const int f = 16 * k + 4 * q + r;
        if (ok && f < F) {
          float v = ((Gs[e] + Gs[2048 + e]) + Gs[4096 + e]) + Gs[6144 + e];
          if (!xi) v += X0s[f * CIN_NC + c];
          float* dst = gx + b * gxs + f * D + d;
          *dst = first ? v : *dst + v;
        }
      }
    }
  }
}

static int cin_check(int64_t B, int F, int D, const int* h_layers, int L) {
  if (B < 0 || F <= 0 || D <= 0 || L <= 0 || !h_layers) return TZR_ERR_INVALID;
  if (L > CIN_MAXL) return TZR_ERR_UNSUPPORTED;
  for (int i = 0; i < L; ++i)
    if (h_layers[i] <= 0) return TZR_ERR_INVALID;
  if (F > CIN_MAXF || D > CIN_MAXD || B >= ((int64_t)1 << 30)) return TZR_ERR_UNSUPPORTED;
  for (int i = 0; i < L; ++i)
    if (h_layers[i] > CIN_MAXO) return TZR_ERR_UNSUPPORTED;
  return TZR_OK;
}

static int cin_params(const float* const* h_w, const float* const* h_c, float* const* h_xs, bool need_xs, const int* h_layers, int L,
                      CinParams* P) {
  if (!h_w || (need_xs && L > 1 && !h_xs)) return TZR_ERR_INVALID;
  for (int i = 0; i < CIN_MAXL; ++i) {
    P->w[i] = i < L ? h_w[i] : nullptr;
    P->c[i] = i < L && h_c ? h_c[i] : nullptr;
    P->xs[i] = i < L - 1 && h_xs ? h_xs[i] : nullptr;
    P->O[i] = i < L ? h_layers[i] : 0;
    if (i < L && !P->w[i]) return TZR_ERR_INVALID;
    if (need_xs && i < L - 1 && !P->xs[i]) return TZR_ERR_INVALID;
  }
  return TZR_OK;
}

extern "C" int tzr_cin_fwd(const float* d_x, int64_t x_stride, const float* const* h_w, const float* const* h_c, const int* h_layers, int L,
                           int64_t B, int F, int D, float* const* h_xs, float* d_y, int64_t y_stride, void* stream) {
  if (const int rc = cin_check(B, F, D, h_layers, L)) return rc;
  int sumO = 0;
  for (int i = 0; i < L; ++i) sumO += h_layers[i];
  if (x_stride < (int64_t)F * D || y_stride < sumO) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  CinParams P;
  if (!d_x || !d_y || !h_c || cin_params(h_w, h_c, h_xs, false, h_layers, L, &P) != TZR_OK) return TZR_ERR_INVALID;
  for (int i = 0; i < L; ++i)
    if (!P.c[i]) return TZR_ERR_INVALID;
  const int TB = D > CIN_NC ? 1 : CIN_NC / D;
  const int64_t units = (B + TB - 1) / TB;
  hipLaunchKernelGGL(cin_fwd_kernel, dim3((unsigned)std::min<int64_t>(units, CIN_MAXGRID)), dim3(CIN_THREADS), 0, static_cast<hipStream_t>(stream),
                     d_x, x_stride, P, L, B, F, D, d_y, y_stride);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_cin_bwd_workspace(int64_t B, int F, int D, const int* h_layers, int L) {
  if (cin_check(B, F, D, h_layers, L) != TZR_OK) return 256;
  return cin_parts_floats(B, D, h_layers, L, F) * sizeof(float) + 256;
}

extern "C" int tzr_cin_bwd(const float* d_grad_y, int64_t gy_stride, const float* d_x, int64_t x_stride, const float* const* h_w,
                           const int* h_layers, int L, int64_t B, int F, int D, float* const* h_xs, float* d_gx, int64_t gx_stride,
                           float* d_dwc, void* ws, size_t ws_size, void* stream) {
  if (const int rc = cin_check(B, F, D, h_layers, L)) return rc;
  int sumO = 0;
  for (int i = 0; i < L; ++i) sumO += h_layers[i];
  if (x_stride < (int64_t)F * D || gx_stride < (int64_t)F * D || gy_stride < sumO) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  CinParams P;
  if (!d_grad_y || !d_x || !d_gx || !d_dwc || cin_params(h_w, nullptr, h_xs, true, h_layers, L, &P) != TZR_OK) return TZR_ERR_INVALID;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_size < tzr_cin_bwd_workspace(B, F, D, h_layers, L) - 256) return TZR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t total = cin_total(h_layers, L, F);
  float* parts = static_cast<float*>(ws);
  CinFinish Fi = {};
  int Hs[CIN_MAXL], yoffs[CIN_MAXL];
  {
    size_t o = 0, po = 0;
    int H = F, yo = 0;
    for (int i = 0; i < L; ++i) {
      Hs[i] = H, yoffs[i] = yo;
      Fi.out_off[i] = o, Fi.part_off[i] = po, Fi.size[i] = (size_t)P.O[i] * H * F + P.O[i];
      Fi.S[i] = cin_layer_parts(B, D, P.O[i], H, F);
      o += Fi.size[i];
      po += (size_t)Fi.S[i] * Fi.size[i];
      yo += P.O[i];
      H = P.O[i];
    }
    Fi.L = L;
  }
  const int64_t tiles = (B * D + CIN_NC - 1) / CIN_NC;
  for (int i = L - 1; i >= 0; --i) {
    const int O = P.O[i], H = Hs[i];
    const float* dxn = i < L - 1 ? P.xs[i] : nullptr;
    float* xi = i > 0 ? P.xs[i - 1] : nullptr;
    hipLaunchKernelGGL(cin_bwd_w_kernel, dim3((unsigned)((O + 63) / 64), (unsigned)(H + 1), (unsigned)Fi.S[i]), dim3(CIN_THREADS), 0, st, d_grad_y,
                       gy_stride, yoffs[i], dxn, d_x, x_stride, (const float*)xi, B, F, D, H, O, parts + Fi.part_off[i], Fi.size[i]);
    TZR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cin_bwd_x_kernel, dim3((unsigned)std::min<int64_t>(tiles, CIN_MAXGRID)), dim3(CIN_THREADS), 0, st, d_grad_y, gy_stride,
                       yoffs[i], dxn, d_x, x_stride, xi, P.w[i], B, F, D, H, O, d_gx, gx_stride, i == L - 1 ? 1 : 0);
    TZR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(cin_bwd_finish_kernel, dim3((unsigned)((total + CIN_THREADS - 1) / CIN_THREADS)), dim3(CIN_THREADS), 0, st,
                     (const float*)parts, Fi, total, d_dwc);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
