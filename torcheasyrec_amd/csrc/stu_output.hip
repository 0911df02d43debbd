// The output stage of an STU layer (tzrec/modules/gr/stu.py behind the attention; the reference's fused form is hstu_compute_output
// of tzrec/ops/hstu_compute.py), fp32, with W = H Dv:
//   us = silu(u);  nh = (attn - mean) rstd;  y = us (nh gamma + beta);  C = [us | attn | y] keep / (1 - p);  out = x + C Wo
// Layer norm takes mean / rstd over a row's W columns, group norm over the Dv columns of each head (biased variance, eps inside
// the root).  C [L, 3 W] is never in memory: the forward forms its MFMA operand in registers from the LDS rows of us and attn,
// the backward recomputes it.  keep is the counter rule of include/tzrec_hip.h (so_keep), recomputed wherever C is.
//
// Forward (grid ceil(L / SO_BLOCK), 256 threads).  A workgroup owns SO_BLOCK = 32 rows, two 16-row tiles of
// v_mfma_f32_16x16x4_f32.  Head: the rows of u (silu applied on the way) and attn go into LDS once, float4 by float4, rows
// W + 4 floats apart; wave v takes the rows v, v + 4, .. and computes each (row, group)'s mean and rstd by the fixed xor tree,
// stored to mean / rstd [L, groups] -- which is also where the K loop reads them back (the workgroup's own stores, behind a
// barrier): a [32, H] table does not fit beside 2 x 32 x 516 floats.  K loop over the segments us, attn, y in chunks of 16
// concat columns: lane (li, g) reads the float4 at columns 16 ch + 4 g of the rows li and 16 + li, forms the A values (for y
// from both tiles, gamma, beta, mean, rstd), applies keep, and issues four MFMAs per (row tile, column tile) -- contraction
// slot e of lane group g is concat column 16 ch + 4 g + e, for A and B alike.  Wave v owns the output column tiles
// [v T, (v + 1) T) (T = tiles of E over four waves, at most 8): its Wo values go global -> registers one chunk ahead of the
// multiply (no other wave wants them), its 2 x T accumulators stay in registers over the whole K loop.  Epilogue: + x, one store.
//
// Backward, row pass (the same blocks).  g's rows go into LDS once.  Wave v owns tiles of 16 columns j of W and computes dC_u,
// dC_a, dC_y for them together (dC = g Wo^T, Wo read out-major as float4s: six accumulators), so du is finished and stored
// from the registers at once.  t = dC_y us gamma goes to LDS [32][W + 4]; dC_a stays in registers.  Behind a barrier the waves
// add each (row, group)'s two sums of the norm's backward over the LDS rows (g's tile is dead: the sums and the block's
// per-column dgamma / dbeta terms live there), behind a second one every lane finishes dattn = dC_a + rstd ((t - m1) - nh m2)
// and stores it once.  One row of partial sums [dgamma | dbeta] per workgroup (group norm: the head's columns added first, a
// wave a head), added by the finishing launch in parts_sum.h's interleaved order.
//
// Backward, weight pass (grid ceil(3 W / 16) x column groups of E).  A workgroup owns 16 concat columns x up to 4 waves x NT
// tiles of dWo and walks the whole batch in steps of 64 rows: thread (row, column) recomputes its four C values of the step
// (inputs fetched a step ahead), they go through a double-buffered LDS tile as the TRANSPOSED operand (one barrier a step), g's
// values come from memory as the B operand.  Stored once; no atomics anywhere, two runs are bit-equal.
#include "parts_sum.h"

#define SO_THREADS 256
#define SO_BLOCK TZR_STU_OUT_BLOCK
#define SO_STEP 64  // rows a step of the weight pass
#define SO_RUN 8    // K steps (of 16 columns; of SO_STEP rows in the weight pass) added in one accumulator before it joins the total

static_assert(sizeof(TzrStuOutput) == 240, "TzrStuOutput: the layout _lib.py mirrors");
static_assert(SO_BLOCK == 32, "two 16-row MFMA tiles a workgroup");

struct SoArgs {
  const float *u, *attn, *x, *gamma, *beta, *wo, *g;
  const int64_t* seed;
  float *mean, *rstd, *out, *du, *dattn, *dwo, *parts;
  int64_t us, as, xs, os, gs, dus, das, L;
  int E, W, hs, nw, group, drop;  // hs groups of nw columns a row (layer norm: one of W)
  uint32_t thr;
  float scale, eps;
};

__device__ __forceinline__ uint64_t so_mix(uint64_t x) {  // zch_mix (csrc/zch.hip): the splitmix64 step
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// keep(i, c) / (1 - p) for row i, concat column c
__device__ __forceinline__ float so_keep(const SoArgs& A, uint64_t seed, int64_t i, int c) {
  const uint64_t n = (uint64_t)i * (uint64_t)(3 * A.W) + (uint64_t)c + 1ull;
  return (uint32_t)(so_mix(seed + n * 0x9E3779B97F4A7C15ull) >> 40) >= A.thr ? A.scale : 0.f;
}
__device__ __forceinline__ int so_gidx(const SoArgs& A, int j) { return A.group ? j / A.nw : j; }  // gamma / beta of column j
__device__ __forceinline__ int so_stat(const SoArgs& A, int j) { return A.group ? j / A.nw : 0; }  // the row's group of column j

// rows [i0, i0 + 32) x w columns of src (row stride rs) -> dst rows w + 4 apart, zeros behind L; SILU: silu on the way
template <bool SILU>
__device__ __forceinline__ void so_load_rows(float* dst, const float* src, int64_t rs, int64_t i0, int64_t L, int w) {
  const int w4 = w >> 2;
  for (int idx = threadIdx.x; idx < SO_BLOCK * w4; idx += SO_THREADS) {
    const int r = idx / w4, c = 4 * (idx - r * w4);
    const int64_t i = i0 + r;
    float4 v = tzr_ld4(src + (i < L ? i : L - 1) * rs + c);
    if (SILU) v = make_float4(v.x * tzr_sigmoid(v.x), v.y * tzr_sigmoid(v.y), v.z * tzr_sigmoid(v.z), v.w * tzr_sigmoid(v.w));
    tzr_st4(dst + r * (w + 4) + c, i < L ? v : tzr_zero4());
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <int NT, int WP>
__global__ __launch_bounds__(SO_THREADS) void tzr_stu_out_fwd_kernel(SoArgs A) {
  __shared__ float Sm[2 * SO_BLOCK * (WP + 4)];
  const int W = A.W, E = A.E, ld = W + 4;
  float* Us = Sm;
  float* At = Sm + SO_BLOCK * ld;
  const int64_t i0 = (int64_t)blockIdx.x * SO_BLOCK;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  so_load_rows<true>(Us, A.u, A.us, i0, A.L, W);
  so_load_rows<false>(At, A.attn, A.as, i0, A.L, W);
  __syncthreads();
  const float inv_n = 1.0f / (float)A.nw;
  for (int r = wv; r < SO_BLOCK && i0 + r < A.L; r += SO_THREADS / TZR_WAVE) {
    for (int h = 0; h < A.hs; ++h) {
      const float* row = At + r * ld + h * A.nw;
      float s = 0.f;
      for (int c = lane; c < A.nw; c += TZR_WAVE) s += row[c];
      const float mean = tzr_wave_sum(s) * inv_n;
      float sq = 0.f;
      for (int c = lane; c < A.nw; c += TZR_WAVE) {
        const float d = row[c] - mean;
        sq = fmaf(d, d, sq);
      }
      const float rstd = 1.0f / sqrtf(tzr_wave_sum(sq) * inv_n + A.eps);
      if (lane == 0) A.mean[(i0 + r) * A.hs + h] = mean, A.rstd[(i0 + r) * A.hs + h] = rstd;
    }
  }
  __syncthreads();  // (mean / rstd of the block's rows: read back below)

  const int ntiles = (E + 15) >> 4, per = (ntiles + 3) >> 2;  // per <= NT
  int col[NT];
  bool cok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tn = wv * per + t;
    col[t] = 16 * tn + li;
    cok[t] = t < per && col[t] < E;
  }
  tzr_f32x4 acc[2][NT], tot[2][NT];  // a run of SO_RUN steps, the runs: two levels keep a sum of 3 W terms short chains
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = tot[0][t] = tot[1][t] = tzr_f32x4{0.f, 0.f, 0.f, 0.f};
  const uint64_t seed = A.drop ? (uint64_t)*A.seed : 0ull;
  const int nch = (W + 15) >> 4, steps = 3 * nch;
  int64_t irow[2], srow[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    irow[rt] = i0 + 16 * rt + li;
    srow[rt] = (irow[rt] < A.L ? irow[rt] : A.L - 1) * A.hs;
  }
  float b[NT][4], bn[NT][4];
  auto fetch = [&](int st, float(*dst)[4]) {  // Wo's values of step st: rows s W + 16 ch + 4 g + e, the wave's columns
    const int s = st / nch, j = 16 * (st - s * nch) + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = cok[t] && j + e < W;
        const float v = tzr_ldg(A.wo + (ok ? (int64_t)(s * W + j + e) * E + col[t] : 0));
        dst[t][e] = ok ? v : 0.f;
      }
    }
  };
  fetch(0, b);
  for (int st = 0; st < steps; ++st) {
    if (st + 1 < steps) fetch(st + 1, bn);
    const int s = st / nch, j = 16 * (st - s * nch) + 4 * g;
    const bool jok = j < W;
    const int jc = jok ? j : 0;
    float a[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int r = 16 * rt + li;
      float4 v;
      if (s == 0) {
        v = tzr_ld4(Us + r * ld + jc);
      } else if (s == 1) {
        v = tzr_ld4(At + r * ld + jc);
      } else {
        const float4 us4 = tzr_ld4(Us + r * ld + jc), at4 = tzr_ld4(At + r * ld + jc);
        const int64_t si = srow[rt] + so_stat(A, jc);
        const float mean = A.mean[si], rstd = A.rstd[si];
        float4 ga, be;
        if (A.group) {
          const float gm = A.gamma[jc / A.nw], bt = A.beta[jc / A.nw];
          ga = make_float4(gm, gm, gm, gm), be = make_float4(bt, bt, bt, bt);
        } else {
          ga = tzr_ld4(A.gamma + jc), be = tzr_ld4(A.beta + jc);
        }
        v.x = us4.x * fmaf((at4.x - mean) * rstd, ga.x, be.x);
        v.y = us4.y * fmaf((at4.y - mean) * rstd, ga.y, be.y);
        v.z = us4.z * fmaf((at4.z - mean) * rstd, ga.z, be.z);
        v.w = us4.w * fmaf((at4.w - mean) * rstd, ga.w, be.w);
      }
      a[rt][0] = jok ? v.x : 0.f, a[rt][1] = jok ? v.y : 0.f, a[rt][2] = jok ? v.z : 0.f, a[rt][3] = jok ? v.w : 0.f;
      if (A.drop) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[rt][e] *= so_keep(A, seed, irow[rt], s * W + jc + e);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][e], b[t][e], acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][e], b[t][e], acc[1][t], 0, 0, 0);
      }
    }
    if ((st & (SO_RUN - 1)) == SO_RUN - 1 || st + 1 == steps) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        tot[0][t] += acc[0][t], tot[1][t] += acc[1][t];
        acc[0][t] = acc[1][t] = tzr_f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) b[t][e] = bn[t][e];
    }
  }
  // accumulator register r of lane (li, g) is (row 4 g + r of the tile, column li of the tile)
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + 16 * rt + 4 * g + r;
        if (cok[t] && i < A.L) A.out[i * A.os + col[t]] = A.x[i * A.xs + col[t]] + tot[rt][t][r];
      }
    }
  }
}

// ---- backward, row pass ----------------------------------------------------------------------------------------------
// P: the LDS class, at least max(E, W)
template <int NJ, int P>
__global__ __launch_bounds__(SO_THREADS) void tzr_stu_out_bwd_rows_kernel(SoArgs A) {
  __shared__ float Sm[2 * SO_BLOCK * (P + 4)];
  const int W = A.W, E = A.E, ldg_ = E + 4, ldt = W + 4;
  float* Gs = Sm;                         // g's rows; behind the MFMA phase: cp [2 W], m1 [32 hs], m2 [32 hs]
  float* Ts = Sm + SO_BLOCK * (P + 4);    // t = dC_y us gamma
  const int64_t i0 = (int64_t)blockIdx.x * SO_BLOCK;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  so_load_rows<false>(Gs, A.g, A.gs, i0, A.L, E);
  __syncthreads();
  const uint64_t seed = A.drop ? (uint64_t)*A.seed : 0ull;
  const int ntw = (W + 15) >> 4, per = (ntw + 3) >> 2;  // per <= NJ
  const int nch = (E + 15) >> 4;
  float dca[NJ][2][4], pg[NJ], pb[NJ];
// (unroll(full): with a plain `unroll` the NJ = 8 body is left rolled and dca goes to scratch)
#pragma clang loop unroll(full)
  for (int jt = 0; jt < NJ; ++jt) {
    const int j = 16 * (wv * per + jt) + li;
    const bool jok = jt < per && j < W;
    const int jc = jok ? j : 0;
    tzr_f32x4 acc[3][2], tot[3][2];
#pragma unroll
    for (int s = 0; s < 3; ++s) acc[s][0] = acc[s][1] = tot[s][0] = tot[s][1] = tzr_f32x4{0.f, 0.f, 0.f, 0.f};
    if (jt < per) {  // (uniform in the wave)
      float4 b[3], bn[3];
      auto fetch = [&](int ch, float4* dst) {  // Wo's rows s W + j at the columns 16 ch + 4 g ..
        const int k = 16 * ch + 4 * g;
        const bool ok = jok && k < E;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const float4 v = tzr_ldg4(A.wo + (ok ? (int64_t)(s * W + jc) * E + k : 0));
          dst[s] = ok ? v : tzr_zero4();
        }
      };
      fetch(0, b);
      for (int ch = 0; ch < nch; ++ch) {
        if (ch + 1 < nch) fetch(ch + 1, bn);
        const int k = 16 * ch + 4 * g;
        const bool kok = k < E;
        float4 a0 = tzr_ld4(Gs + li * ldg_ + (kok ? k : 0)), a1 = tzr_ld4(Gs + (16 + li) * ldg_ + (kok ? k : 0));
        if (!kok) a0 = a1 = tzr_zero4();
        const float a[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const float bb[4] = {b[s].x, b[s].y, b[s].z, b[s].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][e], bb[e], acc[s][0], 0, 0, 0);
            acc[s][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][e], bb[e], acc[s][1], 0, 0, 0);
          }
        }
        if ((ch & (SO_RUN - 1)) == SO_RUN - 1 || ch + 1 == nch) {
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            tot[s][0] += acc[s][0], tot[s][1] += acc[s][1];
            acc[s][0] = acc[s][1] = tzr_f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) b[s] = bn[s];
      }
    }
    // register r of lane (li, g): (row 4 g + r of the tile, column j)
    const float gam = A.gamma[so_gidx(A, jc)], bet = A.beta[so_gidx(A, jc)];
    float sg_ = 0.f, sb_ = 0.f;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = 16 * rt + 4 * g + r;
        const int64_t i = i0 + rr, ic = i < A.L ? i : A.L - 1;
        const bool ok = jok && i < A.L;
        const float uv = A.u[ic * A.us + jc], av = A.attn[ic * A.as + jc];
        const int64_t si = ic * A.hs + so_stat(A, jc);
        const float rstd = A.rstd[si], nh = (av - A.mean[si]) * rstd;
        const float sg = tzr_sigmoid(uv), usv = uv * sg, nrm = fmaf(nh, gam, bet);
        float dcu = tot[0][rt][r], da = tot[1][rt][r], dcy = tot[2][rt][r];
        if (A.drop) {
          dcu *= so_keep(A, seed, ic, jc);
          da *= so_keep(A, seed, ic, W + jc);
          dcy *= so_keep(A, seed, ic, 2 * W + jc);
        }
        const float dus = fmaf(dcy, nrm, dcu);
        if (ok) A.du[i * A.dus + j] = dus * (sg * (1.0f + uv * (1.0f - sg)));
        const float dn = ok ? dcy * usv : 0.f;  // d / d (nh gamma + beta)
        sg_ = fmaf(dn, nh, sg_);
        sb_ += dn;
        if (jok) Ts[rr * ldt + j] = dn * gam;
        dca[jt][rt][r] = da;
      }
    }
    sg_ += __shfl_xor(sg_, 16), sg_ += __shfl_xor(sg_, 32);  // the four row groups of the column
    sb_ += __shfl_xor(sb_, 16), sb_ += __shfl_xor(sb_, 32);
    pg[jt] = sg_, pb[jt] = sb_;
  }
  __syncthreads();  // every wave is through with g's tile; t is whole
  float* cp = Gs;
  float* m1 = Gs + 2 * W;
  float* m2 = m1 + SO_BLOCK * A.hs;
#pragma clang loop unroll(full)
  for (int jt = 0; jt < NJ; ++jt) {
    const int j = 16 * (wv * per + jt) + li;
    if (jt < per && j < W && g == 0) cp[j] = pg[jt], cp[W + j] = pb[jt];
  }
  const float inv_n = 1.0f / (float)A.nw;
  for (int r = wv; r < SO_BLOCK && i0 + r < A.L; r += SO_THREADS / TZR_WAVE) {
    for (int h = 0; h < A.hs; ++h) {
      const int64_t si = (i0 + r) * A.hs + h;
      const float mean = A.mean[si], rstd = A.rstd[si];
      float s1 = 0.f, s2 = 0.f;
      for (int c = lane; c < A.nw; c += TZR_WAVE) {
        const float t = Ts[r * ldt + h * A.nw + c];
        s1 += t;
        s2 = fmaf(t, (A.attn[(i0 + r) * A.as + h * A.nw + c] - mean) * rstd, s2);
      }
      s1 = tzr_wave_sum(s1), s2 = tzr_wave_sum(s2);
      if (lane == 0) m1[r * A.hs + h] = s1 * inv_n, m2[r * A.hs + h] = s2 * inv_n;
    }
  }
  __syncthreads();
#pragma clang loop unroll(full)
  for (int jt = 0; jt < NJ; ++jt) {
    const int j = 16 * (wv * per + jt) + li;
    if (jt < per && j < W) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = 16 * rt + 4 * g + r;
          const int64_t i = i0 + rr;
          if (i < A.L) {
            const int h = so_stat(A, j);
            const float rstd = A.rstd[i * A.hs + h], nh = (A.attn[i * A.as + j] - A.mean[i * A.hs + h]) * rstd;
            A.dattn[i * A.das + j] = dca[jt][rt][r] + rstd * ((Ts[rr * ldt + j] - m1[rr * A.hs + h]) - nh * m2[rr * A.hs + h]);
          }
        }
      }
    }
  }
  // the workgroup's row of partial sums [dgamma | dbeta]: per column (layer norm), per head with its columns added (group norm)
  const int pw = A.group ? A.hs : W;
  float* pr = A.parts + (size_t)blockIdx.x * 2 * pw;
  if (!A.group) {
    for (int c = tid; c < 2 * W; c += SO_THREADS) pr[c] = cp[c];
  } else {
    for (int h = wv; h < A.hs; h += SO_THREADS / TZR_WAVE) {
      float s1 = 0.f, s2 = 0.f;
      for (int c = lane; c < A.nw; c += TZR_WAVE) s1 += cp[h * A.nw + c], s2 += cp[W + h * A.nw + c];
      s1 = tzr_wave_sum(s1), s2 = tzr_wave_sum(s2);
      if (lane == 0) pr[h] = s1, pr[pw + h] = s2;
    }
  }
}

// grid (pw / 64 rounded up, 2): vector v (0: dgamma, 1: dbeta) over the G rows of partial sums, interleaved order
__global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_stu_out_finish_kernel(const float* __restrict__ parts, int G, int pw,
                                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[TZR_FIN_THREADS];
  const int v = blockIdx.y, c = blockIdx.x * TZR_WAVE + (threadIdx.x & (TZR_WAVE - 1));
  const float tot = tzr_parts_sum_interleaved(c < pw ? parts + (size_t)v * pw + c : nullptr, G, 2 * (size_t)pw, red);
  if (threadIdx.x < TZR_WAVE && c < pw) (v == 0 ? dgamma : dbeta)[c] = tot;
}

// ---- backward, weight pass -------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(SO_THREADS) void tzr_stu_out_bwd_w_kernel(SoArgs A) {
  __shared__ float Ct[2][SO_STEP][17];
  const int W = A.W, E = A.E;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int c0 = 16 * (int)blockIdx.x;
  // thread (tr, tc) recomputes C[i0 + tr + 16 q][c0 + tc], q = 0..3
  const int tr = tid >> 4, tc = tid & 15, c = c0 + tc;
  const bool cok = c < 3 * W;
  const int cc = cok ? c : 0, s = cc / W, j = cc - s * W;
  const float gam = A.gamma[so_gidx(A, j)], bet = A.beta[so_gidx(A, j)];
  const int sj = so_stat(A, j);
  const uint64_t seed = A.drop ? (uint64_t)*A.seed : 0ull;
  int col[NT];
  bool nok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    col[t] = 16 * (((int)blockIdx.y * (SO_THREADS / TZR_WAVE) + wv) * NT + t) + li;
    nok[t] = col[t] < E;
  }
  tzr_f32x4 acc[NT], tot[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = tot[t] = tzr_f32x4{0.f, 0.f, 0.f, 0.f};
  float pu[4], pa[4], pm[4], pr[4];
  auto fetch = [&](int64_t i0) {  // (clamped rows: no branch around the loads)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = i0 + tr + 16 * q, ic = i < A.L ? i : A.L - 1;
      pu[q] = A.u[ic * A.us + j], pa[q] = A.attn[ic * A.as + j];
      pm[q] = A.mean[ic * A.hs + sj], pr[q] = A.rstd[ic * A.hs + sj];
    }
  };
  fetch(0);
  int buf = 0, run = 0;
  for (int64_t i0 = 0; i0 < A.L; i0 += SO_STEP, buf ^= 1) {
    float b[4][NT][4];  // g[i0 + 16 q + 4 g + e][col]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = i0 + 16 * q + 4 * g + e;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bool ok = nok[t] && i < A.L;
          const float v = tzr_ldg(A.g + (ok ? i * A.gs + col[t] : 0));
          b[q][t][e] = ok ? v : 0.f;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t i = i0 + tr + 16 * q;
      const float usv = pu[q] * tzr_sigmoid(pu[q]);
      float v = s == 0 ? usv : (s == 1 ? pa[q] : usv * fmaf((pa[q] - pm[q]) * pr[q], gam, bet));
      if (A.drop) v *= so_keep(A, seed, i, cc);
      Ct[buf][tr + 16 * q][tc] = cok && i < A.L ? v : 0.f;
    }
    if (i0 + SO_STEP < A.L) fetch(i0 + SO_STEP);
    __syncthreads();  // (one a step: the step after the next writes this buffer again, behind the next step's barrier)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = Ct[buf][16 * q + 4 * g + e][li];  // (concat column li, row 4 g + e): the transposed operand
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[q][t][e], acc[t], 0, 0, 0);
      }
    }
    if (++run == SO_RUN || i0 + SO_STEP >= A.L) {
      run = 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) tot[t] += acc[t], acc[t] = tzr_f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = c0 + 4 * g + r;
      if (nok[t] && row < 3 * W) A.dwo[(int64_t)row * E + col[t]] = tot[t][r];
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// sizes and limits, then -- with rows -- the operands both directions read
static int so_check(const TzrStuOutput* m, SoArgs* A) {
  if (m->L < 0 || m->H < 1 || m->Dv < 1 || !(m->p >= 0.f) || !(m->p < 1.f)) return TZR_ERR_INVALID;
  const int64_t W = (int64_t)m->H * m->Dv;
  if (!tzr_dim4_ok(m->E, TZR_STU_OUT_MAX_DIM) || W > TZR_STU_OUT_MAX_DIM || !tzr_dim4_ok((int)W, TZR_STU_OUT_MAX_DIM) || (m->group_norm && (m->Dv & 3)) || m->L >= (1ll << 31))
    return TZR_ERR_UNSUPPORTED;
  if (m->L == 0) return TZR_OK;
  A->L = m->L, A->E = m->E, A->W = (int)W, A->group = m->group_norm ? 1 : 0;
  A->hs = A->group ? m->H : 1, A->nw = A->W / A->hs, A->eps = m->eps;
  A->drop = m->training && m->p > 0.f;
  A->thr = (uint32_t)((double)m->p * 16777216.0), A->scale = 1.0f / (1.0f - m->p);
  TZR_TRY(tzr_rows_operand(m->u, m->u_stride, A->W));
  TZR_TRY(tzr_rows_operand(m->attn, m->attn_stride, A->W));
  for (uint64_t p : {m->gamma, m->beta, m->wo, m->mean, m->rstd})
    if (!p || (p & 15)) return TZR_ERR_INVALID;
  if (A->drop && (!m->seed || (m->seed & 7))) return TZR_ERR_INVALID;
  A->u = reinterpret_cast<const float*>(m->u), A->us = m->u_stride;
  A->attn = reinterpret_cast<const float*>(m->attn), A->as = m->attn_stride;
  A->gamma = reinterpret_cast<const float*>(m->gamma), A->beta = reinterpret_cast<const float*>(m->beta);
  A->wo = reinterpret_cast<const float*>(m->wo), A->seed = reinterpret_cast<const int64_t*>(m->seed);
  A->mean = reinterpret_cast<float*>(m->mean), A->rstd = reinterpret_cast<float*>(m->rstd);
  return TZR_OK;
}

static int so_pow2(int n) {  // the unroll class of n tiles a wave: 1, 2, 4, 8
  return n <= 1 ? 1 : (n <= 2 ? 2 : (n <= 4 ? 4 : 8));
}

#define SO_BY_NT(KERNEL, nt, P, grid, s, A)                                                              \
  do {                                                                                                   \
    if ((nt) == 1) hipLaunchKernelGGL((KERNEL<1, P>), grid, dim3(SO_THREADS), 0, s, A);                  \
    else if ((nt) == 2) hipLaunchKernelGGL((KERNEL<2, P>), grid, dim3(SO_THREADS), 0, s, A);             \
    else if ((nt) == 4) hipLaunchKernelGGL((KERNEL<4, P>), grid, dim3(SO_THREADS), 0, s, A);             \
    else hipLaunchKernelGGL((KERNEL<8, P>), grid, dim3(SO_THREADS), 0, s, A);                            \
  } while (0)
// the LDS class of a width: 64, 256 or 512 columns
#define SO_LAUNCH(KERNEL, nt, wide, grid, s, A)                \
  do {                                                         \
    if ((wide) <= 64) SO_BY_NT(KERNEL, nt, 64, grid, s, A);    \
    else if ((wide) <= 256) SO_BY_NT(KERNEL, nt, 256, grid, s, A); \
    else SO_BY_NT(KERNEL, nt, 512, grid, s, A);                \
  } while (0)

extern "C" int tzr_stu_output_fwd(const TzrStuOutput* h_so, void* stream) {
  if (!h_so) return TZR_ERR_INVALID;
  SoArgs A = {};
  TZR_TRY(so_check(h_so, &A));
  if (h_so->L == 0) return TZR_OK;
  TZR_TRY(tzr_rows_operand(h_so->x, h_so->x_stride, A.E));
  TZR_TRY(tzr_rows_operand(h_so->out, h_so->out_stride, A.E));
  A.x = reinterpret_cast<const float*>(h_so->x), A.xs = h_so->x_stride;
  A.out = reinterpret_cast<float*>(h_so->out), A.os = h_so->out_stride;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((A.L + SO_BLOCK - 1) / SO_BLOCK));
  const int nt = so_pow2((((A.E + 15) >> 4) + 3) >> 2);
  SO_LAUNCH(tzr_stu_out_fwd_kernel, nt, A.W, grid, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// one row [dgamma | dbeta] a workgroup of the row pass
extern "C" size_t tzr_stu_output_bwd_workspace(const TzrStuOutput* h_so) {
  SoArgs A = {};
  if (!h_so || so_check(h_so, &A) != TZR_OK || h_so->L == 0) return 256;
  const size_t pw = h_so->group_norm ? (size_t)h_so->H : (size_t)h_so->H * h_so->Dv;
  return (size_t)((h_so->L + SO_BLOCK - 1) / SO_BLOCK) * 2 * pw * sizeof(float) + 256;
}

extern "C" int tzr_stu_output_bwd(const TzrStuOutput* h_so, void* stream) {
  if (!h_so) return TZR_ERR_INVALID;
  SoArgs A = {};
  TZR_TRY(so_check(h_so, &A));
  if (h_so->L == 0) return TZR_OK;
  TZR_TRY(tzr_rows_operand(h_so->grad_out, h_so->grad_out_stride, A.E));
  TZR_TRY(tzr_rows_operand(h_so->du, h_so->du_stride, A.W));
  TZR_TRY(tzr_rows_operand(h_so->dattn, h_so->dattn_stride, A.W));
  for (uint64_t p : {h_so->dwo, h_so->dgamma, h_so->dbeta})
    if (!p || (p & 15)) return TZR_ERR_INVALID;
  if (!h_so->ws || (h_so->ws & 255)) return TZR_ERR_WORKSPACE;
  if (h_so->ws_bytes < tzr_stu_output_bwd_workspace(h_so) - 256) return TZR_ERR_WORKSPACE;
  A.g = reinterpret_cast<const float*>(h_so->grad_out), A.gs = h_so->grad_out_stride;
  A.du = reinterpret_cast<float*>(h_so->du), A.dus = h_so->du_stride;
  A.dattn = reinterpret_cast<float*>(h_so->dattn), A.das = h_so->dattn_stride;
  A.dwo = reinterpret_cast<float*>(h_so->dwo), A.parts = reinterpret_cast<float*>(h_so->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned G = (unsigned)((A.L + SO_BLOCK - 1) / SO_BLOCK);
  const int nj = so_pow2((((A.W + 15) >> 4) + 3) >> 2), wide = A.E > A.W ? A.E : A.W;
  SO_LAUNCH(tzr_stu_out_bwd_rows_kernel, nj, wide, dim3(G), s, A);
  TZR_CHECK_LAUNCH();
  const int ntiles = (A.E + 15) >> 4, nt = ntiles <= 4 ? 1 : (ntiles <= 8 ? 2 : 4), per_wg = 4 * nt;
  const dim3 wgrid((unsigned)((3 * A.W + 15) >> 4), (unsigned)((ntiles + per_wg - 1) / per_wg));
  if (nt == 1) hipLaunchKernelGGL((tzr_stu_out_bwd_w_kernel<1>), wgrid, dim3(SO_THREADS), 0, s, A);
  else if (nt == 2) hipLaunchKernelGGL((tzr_stu_out_bwd_w_kernel<2>), wgrid, dim3(SO_THREADS), 0, s, A);
  else hipLaunchKernelGGL((tzr_stu_out_bwd_w_kernel<4>), wgrid, dim3(SO_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  const int pw = A.group ? A.hs : A.W;
  hipLaunchKernelGGL(tzr_stu_out_finish_kernel, dim3((unsigned)((pw + TZR_WAVE - 1) / TZR_WAVE), 2u), dim3(TZR_FIN_THREADS), 0, s,
                     A.parts, (int)G, pw, reinterpret_cast<float*>(h_so->dgamma), reinterpret_cast<float*>(h_so->dbeta));
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
