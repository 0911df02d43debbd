// The multi-window DIN encoder of TDM (tzrec/modules/sequence.py:288-367) on the jagged rows: per position the attention MLP over
// [k, q * k, q], a one-unit score layer, PReLU, and per window the mean of score * row.  The score is NOT soft-maxed, so a position
// depends on no other: assemble -> layers -> score -> PReLU -> window means is ONE launch forward and one (plus the finishing launch
// of the parameter gradients) backward; no padding position is computed, no [N, H] activation and no [N, 3 C] input is ever in
// memory, and the backward recomputes the pre-activations with the forward's own code (mw_chain): the same bits.
//
// A sample belongs to a WORKGROUP of 256 threads (4 waves).  Its S = min(len, max_len, Sw) rows are loaded once into the LDS tile Ks
// [ceil16(S)][C + 4] (rows behind S as zeros; the row stride C + 4 keeps the float4 reads of sixteen rows off one bank group), the
// query into Qs, and hq = Wc q + b1 -- the query's block of the first layer [Wa | Wb | Wc], one row a SAMPLE -- into Hq.  Wave v
// then takes the 16-row blocks v, v + 4, ..: every layer of a block is a row of 16 x 16 tiles on v_mfma_f32_16x16x4_f32 (exact fp32).
// First layer: contraction length 2 C, lane (li, g) loads the float4 at columns k0 + 4 g of Ks row li and of Qs, the A operand of the
// second half, k * q, is formed in registers and never stored; B is the float4 at W1[col][k0 + 4 g] (nn.Linear's rows are contiguous
// in k: the weights come from L2 as float4s).  A layer writes its PRE-activations to the wave's LDS tile of that layer, [16][HW + 4];
// the next layer applies the activation as it loads its A operand: one code path for ReLU and PReLU, a leaky slope read from
// device memory (ReLU: slope 0).  Score: lane (li, g) takes the units g, g + 4, .. of row li, two xor steps add the four parts.
// Window sums: thread (w, c) walks its window's positions ascending out of Ks.  No atomics, every order fixed: two runs are bit-equal.
//
// Backward.  Workgroup g of min(B, TZR_MWDIN_BWD_MAX_GRID) walks the samples g, g + grid, ..; a sample in chunks of 4 blocks (one a
// wave).  Per chunk: the forward chain; da_n = PReLU'(a_n) <gout[b, w(n)], k_n> / div_w; from the top layer down the gradient g_l
// replaces the pre-activation z_l IN PLACE in the wave's tile (dW_{l+1} = g_{l+1}^T act(z_l) is taken first), g_{l-1} = (g_l W_l)
// act'(z_{l-1}) with B operands W_l[k][col] from L2; the weight gradients are 16 x 16 tiles spread over the four waves, contraction
// over the chunk's rows out of all four waves' tiles, four accumulator chains (one a block) added pairwise; dk_n = s_n / div_w gout +
// g1_n Wa + (g1_n Wb) * q on MFMA, stored from the accumulators; dq's parts in LDS, a row a wave, added in order at the sample's end.
// The partial of the parameter gradients (TZR_MWDIN_MAX_PARAMS = 32768 floats at most) is row g of the workspace, NOT LDS: the
// three in-place tiles of four waves take the LDS (below).  A row of 128 KB is one CU's share of its XCD's 4 MB L2 (32 CUs), which is
// why the cap is set there; that the row stays in L2 between a workgroup's samples is the intent and has NOT been measured.  After the
// row is zeroed (by thread e mod 256), element e is read, added to and written by ONE owner thread for the rest of the launch (tile
// t is wave t mod 4's, a bias or w3 element thread h's), so there is no atomic and the order is the samples' order.  The zeroing
// thread is in general NOT the owner: the __syncthreads() at the top of the sample loop (and those of mw_load behind it), which
// fence global memory at workgroup scope, are what make the owner's first read see the zero -- they are load-bearing, not only LDS
// barriers.  The slopes', alpha's and b3's sums are long signed sums over every position a workgroup sees: per-lane fp64 registers
// (fp32 products), reduced once at the end.  tzr_parts_sum_finish_kernel adds the rows (interleaved order).
//
// Workgroups a CU, by class <HW = 32 | 64 | 128 covering the widest layer, NL layers>.  LDS: Ks 8704 floats (34 KB) + 4 NL tiles of
// 16 (HW + 4) floats + 2 KB (forward) / 6 KB (backward) of rows' scalars, of 160 KB a CU.  Registers (ROCm 7.2, clang 22): the forward
// takes 70 .. 72 VGPRs + 16 AGPRs and is bound by LDS alone; the backward takes 206 .. 249 VGPRs + 32 AGPRs, and a workgroup is one
// wave a SIMD, so the compiler's waves a SIMD is the backward's workgroups a CU whatever LDS would allow:
//   class      example            forward: LDS, workgroups     backward: LDS, VGPRs, workgroups
//   <64, 1>    [36] at C = 96     53 KB, 3                     57 KB, 206, 2
//   <32, 2>    [8, 4] at C = 8    54 KB, 2                     58 KB, 228, 1 (registers; LDS would allow 2)
//   <64, 2>    [64, 32] at C = 64 70 KB, 2                     74 KB, 242, 1 (registers; LDS would allow 2)
//   <128, 3>   the largest        135 KB, 1                    139 KB, 234, 1
// Only the one-layer backward classes reach two workgroups a CU; every two- and three-layer backward class is at one, and the
// three-layer ones spill 80 bytes a lane to scratch.
//
// MW_NOPK: both kernels are compiled with the target feature packed-fp32-ops off, so the compiler does not pair the accumulator
// adds ((acc0 + acc1) + (acc2 + acc3) and the like) into v_pk_add_f32; the inlined helpers take the kernels' setting.  The register,
// LDS and occupancy figures above, the tests and profiles/mwdin are all of that code.  The attribute means nothing to a host pass.
#include "parts_sum.h"
#include "tzr_common.h"

#define MW_THREADS 256
#define MW_WAVES (MW_THREADS / TZR_WAVE)
#define MW_MAXC TZR_MWDIN_MAX_DIM
#define MW_MAXS TZR_MWDIN_MAX_S
#define MW_MAXW TZR_MWDIN_MAX_WINDOWS
#define MW_MAXL TZR_MWDIN_MAX_LAYERS
#define MW_KS_FLOATS (TZR_MWDIN_MAX_SH + 4 * MW_MAXS)  // ceil16(S) rows of C + 4 floats

static_assert(sizeof(TzrMwdin) == 400, "TzrMwdin: the layout _lib.py mirrors");
static_assert(MW_MAXS <= MW_THREADS && MW_MAXC <= MW_THREADS, "one thread a position / a column");

#if defined(__HIP_DEVICE_COMPILE__)
#define MW_NOPK __attribute__((target("no-packed-fp32-ops")))
#else
#define MW_NOPK
#endif

struct MwArgs {
  const float* K;
  const float* Q;
  const int64_t* off;
  const float* Wl[MW_MAXL];
  const float* bl[MW_MAXL];
  const float* sl[MW_MAXL];
  const float* w3;
  const float* b3;
  const float* alpha;
  int64_t ks, qs, B, N;
  int C, W, S, nl;
  int H[MW_MAXL];
  int cum[MW_MAXW + 1];  // cum[w] = wl[0] + .. + wl[w - 1]; cum[W] = Sw
  float* out;
  int64_t os;
  const float* gout;
  int64_t gs;
  float* dK;
  int64_t dks;
  float* dQ;
  int64_t dqs;
  float* parts;
  int P, oW[MW_MAXL], ob[MW_MAXL], ow3, ob3, osl, oal;  // the layout of a partial row (= of dparams)
};

// sample b: its first row, its length (the clamped span: no access leaves the buffers), the rows that take part
__device__ __forceinline__ void mw_sample(const MwArgs& A, int64_t b, int64_t* start, int64_t* len, int* s) {
  tzr_jagged_span(A.off, b, b + 1, A.N, start, len);
  *s = (int)(*len < (int64_t)A.S ? *len : (int64_t)A.S);
}

__device__ __forceinline__ float mw_act(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float mw_dact(float z, float slope) { return z > 0.f ? 1.0f : slope; }
__device__ __forceinline__ float4 mw_act4(float4 z, float slope) {
  return make_float4(mw_act(z.x, slope), mw_act(z.y, slope), mw_act(z.z, slope), mw_act(z.w, slope));
}
// the four parts of a row (lanes li, li + 16, li + 32, li + 48) added in a fixed tree; every lane of the row ends with the sum
__device__ __forceinline__ float mw_row_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// what both kernels load of a sample: the query, the rows, hq = Wc q + b1.  Every thread calls it (barriers inside).
__device__ __forceinline__ void mw_load(const MwArgs& A, int64_t b, int64_t start, int s, float* Ks, float* Qs, float* Hq) {
  const int tid = threadIdx.x, C = A.C, CS = C + 4, C4 = C >> 2, rows = (s + 15) & ~15;
  if (tid < C) Qs[tid] = A.Q[b * A.qs + tid];
  for (int i = tid; i < rows * C4; i += MW_THREADS) {
    const int n = i / C4, j = i - n * C4;
    tzr_st4(Ks + n * CS + 4 * j, n < s ? tzr_ld4(A.K + (start + n) * A.ks + 4 * j) : tzr_zero4());
  }
  __syncthreads();
  if (tid < A.H[0]) {
    const float* wc = A.Wl[0] + (int64_t)tid * 3 * C + 2 * C;
    float a = A.bl[0][tid];
    for (int c = 0; c < C; c += 4) {
      const float4 w = tzr_ld4(wc + c);
      a = fmaf(w.x, Qs[c], a), a = fmaf(w.y, Qs[c + 1], a), a = fmaf(w.z, Qs[c + 2], a), a = fmaf(w.w, Qs[c + 3], a);
    }
    Hq[tid] = a;
  }
  __syncthreads();
}

// The forward of block rb on the calling wave: pre-activations of layer l into tile Tw + l * 16 * TS, the score a_n and
// s_n = PReLU(a_n) into As / Ss (zeros for the rows behind s).  Every thread calls it (barriers inside); `active`: the wave has a block.
template <int HW, int NL>
__device__ __forceinline__ void mw_chain(const MwArgs& A, const float* Ks, const float* Qs, const float* Hq, float* Tw, int rb, bool active, int s,
                                         const float* slp, float alpha, float* As, float* Ss) {
  constexpr int TS = HW + 4;
  const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
  const int C = A.C, CS = C + 4;
  if (active) {  // z1 = [k | k * q] [Wa | Wb]^T + hq
    const int H1 = A.H[0];
    const float* kr = Ks + (16 * rb + li) * CS;
    for (int ct = 0; 16 * ct < H1; ++ct) {
      const int col = 16 * ct + li;
      const bool cok = col < H1;
      const float* wr = A.Wl[0] + (int64_t)(cok ? col : 0) * 3 * C;
      tzr_f32x4 acc[4], z;
      tzr_acc_zero(acc, 4);
      for (int k0 = 0; k0 < C; k0 += 16) {
        const int k = k0 + 4 * g;
        const bool kok = k < C;
        const float4 a = kok ? tzr_ld4(kr + k) : tzr_zero4(), qq = kok ? tzr_ld4(Qs + k) : tzr_zero4();
        const float4 wa = cok && kok ? tzr_ld4(wr + k) : tzr_zero4(), wb = cok && kok ? tzr_ld4(wr + C + k) : tzr_zero4();
        tzr_mfma4(a, wa, acc);
        tzr_mfma4(make_float4(a.x * qq.x, a.y * qq.y, a.z * qq.z, a.w * qq.w), wb, acc);
        // (here and below the join is written inside the k loop, only the last one is used: written behind the loop the
        // backward's register counts move, <32, 2> across an occupancy step -- the class table above is of this form)
        z = tzr_join4(acc);
      }
      if (cok) {
        const float hq = Hq[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) Tw[(4 * g + r) * TS + col] = z[r] + hq;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int l = 1; l < NL; ++l) {  // z_l = act(z_{l-1}) W_l^T + b_l
    if (active) {
      const int Hp = A.H[l - 1], Hc = A.H[l];
      const float* tr = Tw + (l - 1) * 16 * TS + li * TS;
      float* to = Tw + l * 16 * TS;
      for (int ct = 0; 16 * ct < Hc; ++ct) {
        const int col = 16 * ct + li;
        const bool cok = col < Hc;
        const float* wr = A.Wl[l] + (int64_t)(cok ? col : 0) * Hp;
        tzr_f32x4 acc[4], z;
        tzr_acc_zero(acc, 4);
        for (int k0 = 0; k0 < Hp; k0 += 16) {
          const int k = k0 + 4 * g;
          const bool kok = k < Hp;
          tzr_mfma4(kok ? mw_act4(tzr_ld4(tr + k), slp[l - 1]) : tzr_zero4(), cok && kok ? tzr_ld4(wr + k) : tzr_zero4(), acc);
          z = tzr_join4(acc);
        }
        if (cok) {
          const float bias = A.bl[l][col];
#pragma unroll
          for (int r = 0; r < 4; ++r) to[(4 * g + r) * TS + col] = z[r] + bias;
        }
      }
    }
    __syncthreads();
  }
  if (active) {  // a_n = <w3, act(z_L)> + b3, s_n = PReLU(a_n)
    const int HL = A.H[NL - 1];
    const float* tr = Tw + (NL - 1) * 16 * TS + li * TS;
    float p = 0.f;
    for (int h = g; h < HL; h += 4) p = fmaf(A.w3[h], mw_act(tr[h], slp[NL - 1]), p);
    p = mw_row_sum(p);
    const int n = 16 * rb + li;
    const float a = n < s ? p + A.b3[0] : 0.f;
    if (g == 0) As[n] = a, Ss[n] = mw_act(a, alpha);
  }
  __syncthreads();
}

#define MW_SHARED(HW, NL)                                   \
  __shared__ float Ks[MW_KS_FLOATS];                        \
  __shared__ float Ts[MW_WAVES * NL * 16 * (HW + 4)];       \
  __shared__ float Qs[MW_MAXC], Hq[TZR_MWDIN_MAX_DIM];      \
  __shared__ float As[MW_MAXS], Ss[MW_MAXS]

// grid B
template <int HW, int NL>
MW_NOPK __global__ __launch_bounds__(MW_THREADS) void tzr_mwdin_fwd_kernel(MwArgs A) {
  MW_SHARED(HW, NL);
  const int tid = threadIdx.x, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const int C = A.C, CS = C + 4;
  int64_t start, len;
  int s;
  mw_sample(A, b, &start, &len, &s);
  float slp[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) slp[l] = A.sl[l] ? A.sl[l][0] : 0.f;
  const float alpha = A.alpha[0];
  mw_load(A, b, start, s, Ks, Qs, Hq);
  const int nrb = (s + 15) >> 4;
  for (int rb0 = 0; rb0 < nrb; rb0 += MW_WAVES)
    mw_chain<HW, NL>(A, Ks, Qs, Hq, Ts + wv * NL * 16 * (HW + 4), rb0 + wv, rb0 + wv < nrb, s, slp, alpha, As, Ss);
  float* op = A.out + b * A.os;
  for (int o = tid; o < A.W * C; o += MW_THREADS) {  // the window means, positions ascending; a window not reached: a zero row
    const int w = o / C, c = o - w * C;
    const int n1 = A.cum[w + 1] < s ? A.cum[w + 1] : s;
    float a = 0.f;
    for (int n = A.cum[w]; n < n1; ++n) a = fmaf(Ss[n], Ks[n * CS + c], a);
    int64_t d = len - A.cum[w];
    d = d < A.cum[w + 1] - A.cum[w] ? d : A.cum[w + 1] - A.cum[w];
    op[o] = a / (float)(d < 1 ? 1 : d);
  }
  if (tid < C) op[A.W * C + tid] = Qs[tid];
}

// grid min(B, TZR_MWDIN_BWD_MAX_GRID)
template <int HW, int NL>
MW_NOPK __global__ __launch_bounds__(MW_THREADS) void tzr_mwdin_bwd_kernel(MwArgs A) {
  MW_SHARED(HW, NL);
  __shared__ float Da[MW_MAXS];              // the gradient at a_n
  __shared__ float Gsum[TZR_MWDIN_MAX_DIM];  // sum_n g1_n of the sample
  __shared__ float Dv[MW_MAXW];              // the windows' divisors
  __shared__ float Red[MW_WAVES * MW_MAXC];
  __shared__ int Wn[MW_MAXS];                // the window of a position
  constexpr int TS = HW + 4, TW = NL * 16 * TS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int C = A.C, CS = C + 4, C4 = C >> 2, H1 = A.H[0], HL = A.H[NL - 1];
  float* part = A.parts + (int64_t)blockIdx.x * A.P;
  float* Tw = Ts + wv * TW;
  for (int e = tid; e < A.P; e += MW_THREADS) part[e] = 0.f;
  if (tid < MW_MAXS) {
    int w = 0;
    while (w + 1 < A.W && tid >= A.cum[w + 1]) ++w;
    Wn[tid] = w;
  }
  float slp[NL];
  double gsl[NL], gal = 0.0, gb3 = 0.0;  // (sums of signed terms over every position the workgroup sees: fp32 products, added in fp64)
#pragma unroll
  for (int l = 0; l < NL; ++l) slp[l] = A.sl[l] ? A.sl[l][0] : 0.f, gsl[l] = 0.0;
  const float alpha = A.alpha[0];
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    int64_t start, len;
    int s;
    mw_sample(A, b, &start, &len, &s);
    __syncthreads();  // (the sample before is read to its end)
    if (tid < A.W) {
      int64_t d = len - A.cum[tid];
      d = d < A.cum[tid + 1] - A.cum[tid] ? d : A.cum[tid + 1] - A.cum[tid];
      Dv[tid] = (float)(d < 1 ? 1 : d);
    }
    if (tid < H1) Gsum[tid] = 0.f;
    for (int i = tid; i < MW_WAVES * MW_MAXC; i += MW_THREADS) Red[i] = 0.f;  // dq's parts, a row a wave
    mw_load(A, b, start, s, Ks, Qs, Hq);
    const float* gp = A.gout + b * A.gs;
    const int nrb = (s + 15) >> 4;
    for (int rb0 = 0; rb0 < nrb; rb0 += MW_WAVES) {
      const int rb = rb0 + wv, nb = nrb - rb0 < MW_WAVES ? nrb - rb0 : MW_WAVES;  // nb: the chunk's blocks, one a wave
      const bool active = rb < nrb;
      mw_chain<HW, NL>(A, Ks, Qs, Hq, Tw, rb, active, s, slp, alpha, As, Ss);
      if (active) {  // da_n = PReLU'(a_n) <gout[b, w(n)], k_n> / div_w; 0 behind s
        const int n = 16 * rb + li;
        const float* gw = gp + Wn[n] * C;
        const float* kr = Ks + n * CS;
        float p = 0.f;
        for (int c = 4 * g; c < C; c += 16) {
          const float4 x = tzr_ld4(gw + c), k = tzr_ld4(kr + c);
          p = fmaf(x.x, k.x, p), p = fmaf(x.y, k.y, p), p = fmaf(x.z, k.z, p), p = fmaf(x.w, k.w, p);
        }
        p = mw_row_sum(p);
        p = n < s ? p / Dv[Wn[n]] : 0.f;
        const float a = As[n], da = p * mw_dact(a, alpha);
        if (g == 0) Da[n] = da, gb3 += da, gal += a < 0.f ? a * p : 0.f;
      }
      __syncthreads();
      if (tid < HL) {  // dw3 += sum_n da_n act(z_L[n]), the chunk's rows ascending
        float a = 0.f;
        for (int r = 0; r < 16 * nb; ++r)
          a = fmaf(Da[16 * rb0 + r], mw_act(Ts[(r >> 4) * TW + (NL - 1) * 16 * TS + (r & 15) * TS + tid], slp[NL - 1]), a);
        part[A.ow3 + tid] += a;
      }
      __syncthreads();
      if (active) {  // g_L = da_n w3 act'(z_L), in place
        float* t = Tw + (NL - 1) * 16 * TS;
        for (int r = 0; r < 16; ++r) {
          const float da = Da[16 * rb + r];
          for (int h = lane; h < HL; h += TZR_WAVE) {
            const float z = t[r * TS + h], u = da * A.w3[h];
            gsl[NL - 1] += z < 0.f ? z * u : 0.f;
            t[r * TS + h] = u * mw_dact(z, slp[NL - 1]);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int l = NL - 1; l >= 1; --l) {
        const int Hc = A.H[l], Hp = A.H[l - 1];
        const int nit = (Hc + 15) >> 4, njt = (Hp + 15) >> 4;
        for (int t = wv; t < nit * njt; t += MW_WAVES) {  // dW_l += g_l^T act(z_{l-1}): tile t on wave t mod 4, a chain a block
          const int it = t / njt, jt = t - it * njt;
          const int ci = 16 * it + li, cj = 16 * jt + li;
          tzr_f32x4 acc[4];
          tzr_acc_zero(acc, 4);
#pragma unroll
          for (int wb = 0; wb < MW_WAVES; ++wb) {
            if (wb < nb) {
              const float* tg = Ts + wb * TW + l * 16 * TS;
              const float* th = tg - 16 * TS;
#pragma unroll
              for (int r0 = 0; r0 < 16; r0 += 4) {
                const float a = ci < Hc ? tg[(r0 + g) * TS + ci] : 0.f;
                const float x = cj < Hp ? mw_act(th[(r0 + g) * TS + cj], slp[l - 1]) : 0.f;
                acc[wb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x, acc[wb], 0, 0, 0);
              }
            }
          }
          const tzr_f32x4 d = tzr_join4(acc);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (16 * it + 4 * g + r < Hc && cj < Hp) part[A.oW[l] + (16 * it + 4 * g + r) * Hp + cj] += d[r];
        }
        if (tid < Hc) {  // db_l += sum_n g_l[n]
          float a = 0.f;
          for (int r = 0; r < 16 * nb; ++r) a += Ts[(r >> 4) * TW + l * 16 * TS + (r & 15) * TS + tid];
          part[A.ob[l] + tid] += a;
        }
        __syncthreads();
        if (active) {  // g_{l-1} = (g_l W_l) act'(z_{l-1}), in place
          const float* tr = Tw + l * 16 * TS + li * TS;
          float* to = Tw + (l - 1) * 16 * TS;
          for (int ct = 0; 16 * ct < Hp; ++ct) {
            const int col = 16 * ct + li;
            const bool cok = col < Hp;
            tzr_f32x4 acc[4], u;
            tzr_acc_zero(acc, 4);
            for (int k0 = 0; k0 < Hc; k0 += 16) {
              const int k = k0 + 4 * g;
              const bool kok = k < Hc;
              const float* wp = A.Wl[l] + (int64_t)k * Hp + col;
              const bool ok = cok && kok;
              tzr_mfma4(kok ? tzr_ld4(tr + k) : tzr_zero4(), ok ? make_float4(wp[0], wp[Hp], wp[2 * Hp], wp[3 * Hp]) : tzr_zero4(), acc);
              u = tzr_join4(acc);
            }
            if (cok) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float z = to[(4 * g + r) * TS + col];
                gsl[l - 1] += z < 0.f ? z * u[r] : 0.f;
                to[(4 * g + r) * TS + col] = u[r] * mw_dact(z, slp[l - 1]);
              }
            }
          }
        }
        __syncthreads();
      }
      {  // [dWa | dWb] += g1^T [k | k * q]: tile t on wave t mod 4
        const int nit = (H1 + 15) >> 4, njt = (C + 15) >> 4;
        for (int t = wv; t < 2 * nit * njt; t += MW_WAVES) {
          const int half = t / (nit * njt), u = t - half * nit * njt, it = u / njt, jt = u - it * njt;
          const int ci = 16 * it + li, cj = 16 * jt + li;
          const float qf = half ? (cj < C ? Qs[cj] : 0.f) : 1.0f;
          tzr_f32x4 acc[4];
          tzr_acc_zero(acc, 4);
#pragma unroll
          for (int wb = 0; wb < MW_WAVES; ++wb) {
            if (wb < nb) {
              const float* tg = Ts + wb * TW;
              const float* kr = Ks + 16 * (rb0 + wb) * CS;
#pragma unroll
              for (int r0 = 0; r0 < 16; r0 += 4) {
                const float a = ci < H1 ? tg[(r0 + g) * TS + ci] : 0.f;
                const float x = cj < C ? kr[(r0 + g) * CS + cj] * qf : 0.f;
                acc[wb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x, acc[wb], 0, 0, 0);
              }
            }
          }
          const tzr_f32x4 d = tzr_join4(acc);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (16 * it + 4 * g + r < H1 && cj < C) part[A.oW[0] + (16 * it + 4 * g + r) * 3 * C + half * C + cj] += d[r];
        }
        if (tid < H1) {  // db1 += sum_n g1[n]; the sample's sum for dWc and dq
          float a = 0.f;
          for (int r = 0; r < 16 * nb; ++r) a += Ts[(r >> 4) * TW + (r & 15) * TS + tid];
          part[A.ob[0] + tid] += a;
          Gsum[tid] += a;
        }
      }
      if (active) {  // dk_n = s_n / div_w gout[b, w(n)] + g1_n Wa + (g1_n Wb) * q; dq += (g1_n Wb) * k_n
        const float* tr = Tw + li * TS;
        for (int ct = 0; 16 * ct < C; ++ct) {
          {
            const int col = 16 * ct + li;
            const bool cok = col < C;
            tzr_f32x4 acca[4], accb[4], ua, ub;
            tzr_acc_zero(acca, 4), tzr_acc_zero(accb, 4);
            for (int k0 = 0; k0 < H1; k0 += 16) {
              const int k = k0 + 4 * g;
              const bool kok = k < H1, ok = cok && kok;
              const float* wp = A.Wl[0] + (int64_t)k * 3 * C + col;
              const float4 a = kok ? tzr_ld4(tr + k) : tzr_zero4();
              tzr_mfma4(a, ok ? make_float4(wp[0], wp[3 * C], wp[6 * C], wp[9 * C]) : tzr_zero4(), acca);
              tzr_mfma4(a, ok ? make_float4(wp[C], wp[4 * C], wp[7 * C], wp[10 * C]) : tzr_zero4(), accb);
              ua = tzr_join4(acca), ub = tzr_join4(accb);
            }
            float dqp = 0.f;
            if (cok) {
              const float qc = Qs[col];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int n = 16 * rb + 4 * g + r;
                if (n < s) {
                  const int w = Wn[n];
                  A.dK[(start + n) * A.dks + col] = fmaf(ub[r], qc, fmaf(Ss[n] / Dv[w], gp[w * C + col], ua[r]));
                  dqp = fmaf(ub[r], Ks[n * CS + col], dqp);
                }
              }
            }
            dqp = mw_row_sum(dqp);
            if (g == 0 && cok) Red[wv * MW_MAXC + col] += dqp;
          }
        }
      }
      __syncthreads();
    }
    for (int64_t i = (int64_t)s * C4 + tid; i < len * C4; i += MW_THREADS) {  // rows behind S: zero gradient rows
      const int64_t n = i / C4;
      tzr_st4(A.dK + (start + n) * A.dks + 4 * (i - n * C4), tzr_zero4());
    }
    if (tid < C) {  // dq = sum_n (g1_n Wb) * k_n (a wave's blocks in order, then the four waves) + Wc^T sum_n g1_n + gout[b, W]
      float a = 0.f;
      for (int i = 0; i < H1; ++i) a = fmaf(A.Wl[0][(int64_t)i * 3 * C + 2 * C + tid], Gsum[i], a);
      const float v = (Red[tid] + Red[MW_MAXC + tid]) + (Red[2 * MW_MAXC + tid] + Red[3 * MW_MAXC + tid]);
      A.dQ[b * A.dqs + tid] = (v + a) + gp[A.W * C + tid];
    }
    for (int e = tid; e < H1 * C; e += MW_THREADS) {  // dWc += (sum_n g1_n) q^T
      const int i = e / C, c = e - i * C;
      part[A.oW[0] + i * 3 * C + 2 * C + c] += Gsum[i] * Qs[c];
    }
  }
  if (blockIdx.x == 0) {  // rows in front of offsets[0] and behind offsets[B] belong to no sample: zero gradient rows, by workgroup 0
    int64_t lo, n;
    tzr_jagged_span(A.off, 0, A.B, A.N, &lo, &n);
    const int64_t hi = lo + n;
    for (int64_t i = tid; i < (lo + A.N - hi) * C4; i += MW_THREADS) {
      const int64_t n = i / C4;
      tzr_st4(A.dK + (n < lo ? n : hi + (n - lo)) * A.dks + 4 * (i - n * C4), tzr_zero4());
    }
  }
  __syncthreads();
  // the slopes', alpha's and b3's sums: lanes by the xor tree, the four waves in order
  __shared__ double Rd[MW_WAVES * 8];
  double v[NL + 2];
#pragma unroll
  for (int l = 0; l < NL; ++l) v[l] = tzr_wave_sum(gsl[l]);
  v[NL] = tzr_wave_sum(gal), v[NL + 1] = tzr_wave_sum(gb3);
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < NL + 2; ++l) Rd[wv * 8 + l] = v[l];
  }
  __syncthreads();
  if (tid < NL + 2) {
    const double t = (Rd[tid] + Rd[8 + tid]) + (Rd[16 + tid] + Rd[24 + tid]);
    // (a ReLU layer -- no slope pointer -- has no slope gradient: its slot is 0, as the header says)
    part[tid < NL ? A.osl + tid : (tid == NL ? A.oal : A.ob3)] = tid < NL && !A.sl[tid] ? 0.f : (float)t;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// the floats of dparams: per layer [W_l | b_l], w3, b3, a slope a layer, alpha; 0: a shape outside the limits
static int64_t mw_params(const TzrMwdin* m) {
  if (m->layers < 1 || m->layers > MW_MAXL || m->C < 4 || (m->C & 3) || m->C > MW_MAXC) return 0;
  int64_t P = 0, in = 3 * (int64_t)m->C;
  for (int l = 0; l < m->layers; ++l) {
    const int H = m->H[l];
    if (H < 4 || (H & 3) || H > TZR_MWDIN_MAX_DIM) return 0;
    P += (in + 1) * H;
    in = H;
  }
  return P + in + 1 + m->layers + 1;
}

static bool mw_limits(const TzrMwdin* m, int* S) {
  const int64_t P = mw_params(m);
  if (P == 0 || P > TZR_MWDIN_MAX_PARAMS || m->W < 1 || m->W > MW_MAXW || m->max_len < 1) return false;
  int64_t sw = 0;
  for (int w = 0; w < m->W; ++w) {
    if (m->windows_len[w] < 1) return false;
    sw += m->windows_len[w];
  }
  const int64_t s = sw < m->max_len ? sw : m->max_len;
  if (s > MW_MAXS) return false;
  int wide = m->C;
  for (int l = 0; l < m->layers; ++l) wide = m->H[l] > wide ? m->H[l] : wide;
  if ((s + 15) / 16 * 16 * wide > TZR_MWDIN_MAX_SH || m->B >= (1ll << 31) || m->N >= (1ll << 31)) return false;
  *S = (int)s;
  return true;
}

static inline size_t mw_ws_bytes(const TzrMwdin* m) { return tzr_align_up((size_t)tzr_capped_grid(m->B, TZR_MWDIN_BWD_MAX_GRID) * mw_params(m) * sizeof(float)); }

// sizes, limits (nothing else is looked at for a shape this build has no kernel for), then the pointers both directions read
static int mw_check(const TzrMwdin* m, MwArgs* A) {
  if (m->B < 0 || m->N < 0) return TZR_ERR_INVALID;
  int S = 0;
  if (!mw_limits(m, &S)) return TZR_ERR_UNSUPPORTED;
  if (m->N > 0) TZR_TRY(tzr_rows_operand(m->k, m->k_stride, m->C));
  TZR_TRY(tzr_rows_operand(m->q, m->q_stride, m->C));
  if (!m->offsets || (m->offsets & 7) || !m->w3 || (m->w3 & 3) || !m->b3 || (m->b3 & 3) || !m->alpha || (m->alpha & 3)) return TZR_ERR_INVALID;
  int P = 0, in = 3 * m->C;
  for (int l = 0; l < m->layers; ++l) {
    if (!m->w[l] || (m->w[l] & 15) || !m->b[l] || (m->b[l] & 3) || (m->slope[l] & 3)) return TZR_ERR_INVALID;
    A->Wl[l] = reinterpret_cast<const float*>(m->w[l]);
    A->bl[l] = reinterpret_cast<const float*>(m->b[l]);
    A->sl[l] = reinterpret_cast<const float*>(m->slope[l]);
    A->H[l] = m->H[l];
    A->oW[l] = P, A->ob[l] = P + in * m->H[l];
    P += (in + 1) * m->H[l];
    in = m->H[l];
  }
  A->ow3 = P, A->ob3 = P + in, A->osl = P + in + 1, A->oal = P + in + 1 + m->layers;
  A->P = A->oal + 1;
  A->K = reinterpret_cast<const float*>(m->k);
  A->Q = reinterpret_cast<const float*>(m->q);
  A->off = reinterpret_cast<const int64_t*>(m->offsets);
  A->w3 = reinterpret_cast<const float*>(m->w3);
  A->b3 = reinterpret_cast<const float*>(m->b3);
  A->alpha = reinterpret_cast<const float*>(m->alpha);
  A->ks = m->k_stride, A->qs = m->q_stride, A->B = m->B, A->N = m->N;
  A->C = m->C, A->W = m->W, A->S = S, A->nl = m->layers;
  A->cum[0] = 0;
  for (int w = 0; w < m->W; ++w) A->cum[w + 1] = A->cum[w] + m->windows_len[w];
  return TZR_OK;
}

// the class of a shape: HW covers the widest layer, NL = the layers
#define MW_LAUNCH_NL(KERNEL, NL, grid, s, A)                                                                                 \
  do {                                                                                                                        \
    int wide_ = 0;                                                                                                            \
    for (int l_ = 0; l_ < NL; ++l_) wide_ = (A).H[l_] > wide_ ? (A).H[l_] : wide_;                                            \
    if (wide_ <= 32) hipLaunchKernelGGL((KERNEL<32, NL>), dim3((unsigned)(grid)), dim3(MW_THREADS), 0, s, A);                 \
    else if (wide_ <= 64) hipLaunchKernelGGL((KERNEL<64, NL>), dim3((unsigned)(grid)), dim3(MW_THREADS), 0, s, A);            \
    else hipLaunchKernelGGL((KERNEL<128, NL>), dim3((unsigned)(grid)), dim3(MW_THREADS), 0, s, A);                            \
  } while (0)
#define MW_LAUNCH(KERNEL, grid, s, A)                            \
  do {                                                           \
    if ((A).nl == 1) MW_LAUNCH_NL(KERNEL, 1, grid, s, A);        \
    else if ((A).nl == 2) MW_LAUNCH_NL(KERNEL, 2, grid, s, A);   \
    else MW_LAUNCH_NL(KERNEL, 3, grid, s, A);                    \
  } while (0)

extern "C" size_t tzr_mwdin_workspace(const TzrMwdin* h_mw) {
  int S;
  if (!h_mw || h_mw->B < 1 || !mw_limits(h_mw, &S)) return 256;
  return mw_ws_bytes(h_mw) + 256;
}

extern "C" int tzr_mwdin_fwd(const TzrMwdin* h_mw, void* stream) {
  if (!h_mw) return TZR_ERR_INVALID;
  MwArgs A = {};
  TZR_TRY(mw_check(h_mw, &A));
  TZR_TRY(tzr_rows_operand(h_mw->out, h_mw->out_stride, (h_mw->W + 1) * h_mw->C));
  if (h_mw->B == 0) return TZR_OK;
  A.out = reinterpret_cast<float*>(h_mw->out);
  A.os = h_mw->out_stride;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MW_LAUNCH(tzr_mwdin_fwd_kernel, h_mw->B, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_mwdin_bwd(const TzrMwdin* h_mw, void* stream) {
  if (!h_mw) return TZR_ERR_INVALID;
  MwArgs A = {};
  TZR_TRY(mw_check(h_mw, &A));
  TZR_TRY(tzr_rows_operand(h_mw->grad_out, h_mw->grad_out_stride, (h_mw->W + 1) * h_mw->C));
  if (h_mw->N > 0) TZR_TRY(tzr_rows_operand(h_mw->dk, h_mw->dk_stride, h_mw->C));
  TZR_TRY(tzr_rows_operand(h_mw->dq, h_mw->dq_stride, h_mw->C));
  if (!h_mw->dparams || (h_mw->dparams & 3)) return TZR_ERR_INVALID;
  if (h_mw->B == 0) return TZR_OK;
  if (!h_mw->ws || (h_mw->ws & 255) || h_mw->ws_bytes < mw_ws_bytes(h_mw)) return TZR_ERR_WORKSPACE;
  A.gout = reinterpret_cast<const float*>(h_mw->grad_out);
  A.gs = h_mw->grad_out_stride;
  A.dK = reinterpret_cast<float*>(h_mw->dk);
  A.dks = h_mw->dk_stride;
  A.dQ = reinterpret_cast<float*>(h_mw->dq);
  A.dqs = h_mw->dq_stride;
  A.parts = reinterpret_cast<float*>(h_mw->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int G = (int)tzr_capped_grid(h_mw->B, TZR_MWDIN_BWD_MAX_GRID);
  MW_LAUNCH(tzr_mwdin_bwd_kernel, G, s, A);
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_parts_sum_finish_kernel<>, dim3((unsigned)((A.P + TZR_WAVE - 1) / TZR_WAVE)), dim3(TZR_FIN_THREADS), 0, s, A.parts, G, A.P,
                     reinterpret_cast<float*>(h_mw->dparams));
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
