// The Bayesian relation towers of DBMTL (tzrec/models/dbmtl.py:90-112, 155-167), the whole chain of a model in one launch
// forward and two launches backward.  Tower t (config order, T <= 8) has an input x_t [B, Hx_t], a list deps_t of EARLIER
// towers and L_t in 0..4 layers (W [N, K], b [N]) in nn.Linear layout:
//
//     L_t = 0:   r_t = x_t                                        (nothing computed or copied: consumers read x_t)
//     L_t >= 1:  r_t = relu(W_{L-1} .. relu(W_0 u_t + b_0) .. + b_{L-1}),   u_t = [x_t | r_d for d in deps_t]
//
// As torch ops that is a cat and per layer an addmm and a ReLU forward, and about three times that backward, a serial chain
// of GEMMs a few dozen units wide.  Here u_t is never written: the K loop of the first layer walks the segments.
//
// Rows.  A workgroup of 256 threads takes a block of 16 rows (one MFMA M-tile) at a time in a grid-stride loop; every product
// is on v_mfma_f32_16x16x4_f32 (exact fp32).  The N / 16 column tiles of a layer go round-robin over the four waves (N <= 128:
// at most two tiles a wave), each tile on RC_CH = 8 interleaved accumulator chains over K (the 4-column steps c, c + 8, ..
// form chain c; added pairwise), so a chain is K / 32 additions long, eight independent MFMAs cover a dependent one's latency
// and eight weight loads of a tile are in flight together.  The first layer's A operand is staged into LDS RC_KC columns of u_t at a time, from x_t in memory, from x_d in
// memory (L_d = 0) or from r_d of THIS row block in LDS (Rs, L_d >= 1); the later layers read the previous h from LDS.
// Weights are the B operand, read from memory (L2).  Every layer's post-ReLU output goes to memory (h, all the backward
// keeps) and to LDS.  Rows past B are zeros going in and are not stored.
//
// Backward, rows.  Gs[t] starts as g_t = dL/dr_t (zeros for a null pointer); the towers are walked in reverse, and tower t
// adds the slices of du_t = dz_{t,0} W_{t,0} to Gs[d] of its deps, so the gradient of r_d is g_d plus its consumers' slices in
// descending consumer index.  dz_l = (dz_{l+1} W_{l+1}) * [h_l > 0] goes to LDS as the next product's A operand and to the
// workspace.  Slice 0 of du_t is dx_t; the slice of an L_d = 0 dep goes to dx_d in memory, stored by its highest consumer and
// added to by the others (separated by workgroup barriers; a block's rows belong to one workgroup).  An L = 0 tower nobody
// reads gets zeros.
//
// Backward, weights.  Workgroup (tile, (t, l)) of 512 threads owns a 16 x 16 tile of dW_{t,l} = dz_{t,l}^T u over the WHOLE
// batch: its eight waves take the 4-row steps w, w + 8, .., a wave's steps going round-robin onto eight accumulator chains
// (at B = 8192 a chain is 32 MFMAs long; 16 loads of a lane in flight); chains and then waves are added pairwise, the waves through LDS.  The first layer's
// operand column is resolved to its segment once; the workgroups of k-tile 0 also add the columns of dz for db (a lane its
// rows on eight chains; chains, waves and the four row residues added pairwise).
//
// LDS.  The r_t / gradient buffers are sized by a template class over the number NR of towers WITH layers (2, 4, 8):
// forward Us 16.1 KB + Hs 16.3 KB + Rs 8.1 KB x NR = 48.6 / 64.9 / 97.4 KB (3 / 2 / 1 workgroups a CU); backward rows
// Ds 16.3 KB + Gs 8.1 KB x NR = 32.5 / 48.8 / 81.3 KB; weights 10 KB.
// No atomics; every sum has a fixed order, a function of the shapes alone: two runs are bit-equal.
#include "tzr_common.h"

#define RC_THREADS 256
#define RC_WAVES (RC_THREADS / TZR_WAVE)
#define RC_ROWS 16
#define RC_T TZR_RELATION_CHAIN_MAX_TOWERS
#define RC_L TZR_RELATION_CHAIN_MAX_LAYERS
#define RC_MAXW TZR_RELATION_CHAIN_MAX_WIDTH
#define RC_MAXX TZR_RELATION_CHAIN_MAX_X
#define RC_WS (RC_MAXW + 2)  // LDS row strides of 2 mod 32 floats: the 16 rows x 4 columns of an A operand read hit 32 banks per half
#define RC_KC 256
#define RC_US (RC_KC + 2)
#define RC_TPW (RC_MAXW / 16 / RC_WAVES)  // column tiles a wave owns at a time
#define RC_CH 8
#define RC_MAXGRID 512  // workgroups of a row pass
#define RC_WG_THREADS 512
#define RC_WG_WAVES (RC_WG_THREADS / TZR_WAVE)
#define RC_WG_UN 8  // accumulator chains of a wave over its steps (sixteen measured slower: 86 against 46 us a launch)
static_assert(RC_WG_WAVES == 8 && RC_WG_UN == 8, "the pairwise joins below are written out for eight");

static_assert(sizeof(TzrRelationChain) == 2176, "TzrRelationChain: the layout _lib.py mirrors");

typedef float rc_f4 __attribute__((ext_vector_type(4)));

struct RcTower {
  const float* x;
  int64_t xs;
  const float* g;  // backward: dL/dr_t, null: none
  int64_t gs;
  float* dx;
  int64_t dxs;
  const float* w[RC_L];
  const float* b[RC_L];
  float* h[RC_L];   // [B, n[l]] contiguous: the forward writes, the backward reads
  float* dz[RC_L];  // [B, n[l]] contiguous: workspace
  float* dw[RC_L];
  float* db[RC_L];
  int hx, L, nd, K0;  // K0: width of u_t
  int rw;             // width of r_t
  int zero_dx;        // L = 0 and no consumer
  int slot;           // L >= 1: which of the NR rows-in-LDS buffers holds r_t (forward) / its gradient (backward)
  int dep[RC_T];
  int off[RC_T + 2];  // segment s of u_t is [off[s], off[s + 1]): s = 0 is x_t, s >= 1 is r of dep[s - 1]
  int n[RC_L];
  int first[RC_T + 1];  // segment s is an L = 0 dep whose dx this tower stores (1) or adds to (0)
};
struct RcArgs {
  int T;
  RcTower t[RC_T];
};

__device__ __forceinline__ rc_f4 rc_zero() {
  rc_f4 z = {0.f, 0.f, 0.f, 0.f};
  return z;
}

// acc[u][c] += As[16, kc] W for the wave's tiles t0 + wv + RC_WAVES u: A(i, k) = As[i AS + k] (LDS), W(k, j) = W[k wks + j wjs], j < N
__device__ __forceinline__ void rc_mma(const float* As, int AS, int kc, const float* __restrict__ W, size_t wks, size_t wjs, int N, int t0, int wv,
                                       int q, int li, rc_f4 (*acc)[RC_CH]) {
  const int NT = (N + 15) >> 4;
  for (int k0 = 0; k0 < kc; k0 += 4 * RC_CH) {
#pragma unroll
    for (int c = 0; c < RC_CH; ++c) {
      const int k = k0 + 4 * c + q;
      const bool kok = k < kc;
      const int kk = kok ? k : 0;
      const float a = kok ? As[li * AS + kk] : 0.f;
#pragma unroll
      for (int u = 0; u < RC_TPW; ++u) {
        const int tile = t0 + wv + RC_WAVES * u;
        if (tile < NT) {  // (uniform)
          const int j = 16 * tile + li;
          const bool ok = kok && j < N;
          const float b = W[ok ? (size_t)kk * wks + (size_t)j * wjs : 0];
          acc[u][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok ? b : 0.f, acc[u][c], 0, 0, 0);
        }
      }
    }
  }
}
__device__ __forceinline__ rc_f4 rc_join(const rc_f4* a) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }
static_assert(RC_CH == 8, "rc_join is written out for eight chains");
__device__ __forceinline__ void rc_clear(rc_f4 (*acc)[RC_CH]) {
#pragma unroll
  for (int u = 0; u < RC_TPW; ++u)
#pragma unroll
    for (int c = 0; c < RC_CH; ++c) acc[u][c] = rc_zero();
}

// grid min(B / 16 rounded up, RC_MAXGRID).  NR: the class's bound on the towers with layers (the emulator's __shared__ is a
// function-local static, so the arrays are static and sized by a template class, as in cross_v2.hip).
template <int NR>
__global__ __launch_bounds__(RC_THREADS) void tzr_relation_chain_fwd_kernel(RcArgs A, int64_t B) {
  __shared__ float Us[RC_ROWS * RC_US];
  __shared__ float Hs[2 * RC_ROWS * RC_WS];
  __shared__ float Rs[NR * RC_ROWS * RC_WS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int64_t nblk = (B + RC_ROWS - 1) / RC_ROWS;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t b0 = blk * RC_ROWS;
#pragma unroll 1
    for (int t = 0; t < A.T; ++t) {
      const RcTower& tw = A.t[t];
#pragma unroll 1
      for (int l = 0; l < tw.L; ++l) {
        const int N = tw.n[l], NT = (N + 15) >> 4;
        rc_f4 acc[RC_TPW][RC_CH];
        rc_clear(acc);
        if (l == 0) {
          for (int c0 = 0; c0 < tw.K0; c0 += RC_KC) {
            const int kc = min(RC_KC, tw.K0 - c0);
            __syncthreads();  // (the previous reads of Us; Rs of the towers before)
            for (int s = 0; s <= tw.nd; ++s) {
              const int lo = max(tw.off[s], c0), hi = min(tw.off[s + 1], c0 + kc);
              if (lo >= hi) continue;  // (uniform)
              const int w4 = (hi - lo) >> 2;
              const RcTower& src = s == 0 ? tw : A.t[tw.dep[s - 1]];
              const bool lds = s > 0 && src.L > 0;
              const float* rs = Rs + (lds ? src.slot : 0) * RC_ROWS * RC_WS;
              for (int e = threadIdx.x; e < RC_ROWS * w4; e += RC_THREADS) {
                const int row = e / w4, col = lo + 4 * (e - row * w4), sc = col - tw.off[s];
                float4 v = tzr_zero4();
                if (lds) {
                  const float* p = rs + row * RC_WS + sc;
                  v = make_float4(p[0], p[1], p[2], p[3]);
                } else if (b0 + row < B) {
                  v = tzr_ld4(src.x + (b0 + row) * src.xs + sc);
                }
                float* d = Us + row * RC_US + (col - c0);
                d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
              }
            }
            __syncthreads();
            rc_mma(Us, RC_US, kc, tw.w[0] + c0, 1, tw.K0, N, 0, wv, q, li, acc);
          }
        } else {
          const int K = tw.n[l - 1];
          rc_mma(Hs + ((l - 1) & 1) * RC_ROWS * RC_WS, RC_WS, K, tw.w[l], 1, K, N, 0, wv, q, li, acc);
        }
        float* dst = l == tw.L - 1 ? Rs + tw.slot * RC_ROWS * RC_WS : Hs + (l & 1) * RC_ROWS * RC_WS;
        float* hl = tw.h[l];
#pragma unroll
        for (int u = 0; u < RC_TPW; ++u) {
          const int tile = wv + RC_WAVES * u, col = 16 * tile + li;
          if (tile < NT && col < N) {
            const rc_f4 sum = rc_join(acc[u]);
            const float bias = tw.b[l][col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 4 * q + r;
              const float v = fmaxf(sum[r] + bias, 0.f);
              dst[row * RC_WS + col] = v;
              if (b0 + row < B) hl[(b0 + row) * N + col] = v;
            }
          }
        }
        __syncthreads();
      }
    }
  }
}

// The backward's row pass.
template <int NR>
__global__ __launch_bounds__(RC_THREADS) void tzr_relation_chain_bwd_rows_kernel(RcArgs A, int64_t B) {
  __shared__ float Gs[NR * RC_ROWS * RC_WS];
  __shared__ float Ds[2 * RC_ROWS * RC_WS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int64_t nblk = (B + RC_ROWS - 1) / RC_ROWS;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t b0 = blk * RC_ROWS;
    __syncthreads();  // (the previous block's reads of Gs)
#pragma unroll 1
    for (int t = 0; t < A.T; ++t) {
      const RcTower& tw = A.t[t];
      const int w4 = tw.rw >> 2;
      if (tw.L > 0) {
        float* gt = Gs + tw.slot * RC_ROWS * RC_WS;
        for (int e = threadIdx.x; e < RC_ROWS * w4; e += RC_THREADS) {
          const int row = e / w4, col = 4 * (e - row * w4);
          const float4 v = tw.g && b0 + row < B ? tzr_ld4(tw.g + (b0 + row) * tw.gs + col) : tzr_zero4();
          float* d = gt + row * RC_WS + col;
          d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
      } else if (tw.zero_dx) {
        for (int e = threadIdx.x; e < RC_ROWS * w4; e += RC_THREADS) {
          const int row = e / w4, col = 4 * (e - row * w4);
          if (b0 + row < B) tzr_st4(tw.dx + (b0 + row) * tw.dxs + col, tzr_zero4());
        }
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = A.T - 1; t >= 0; --t) {
      const RcTower& tw = A.t[t];
      if (tw.L == 0) continue;  // (uniform)
      {
        const int l = tw.L - 1, N = tw.n[l];
        const float* gt = Gs + tw.slot * RC_ROWS * RC_WS;
        float* ds = Ds + (l & 1) * RC_ROWS * RC_WS;
        for (int e = threadIdx.x; e < RC_ROWS * N; e += RC_THREADS) {
          const int row = e / N, col = e - row * N;
          const bool ok = b0 + row < B;
          const float hv = ok ? tw.h[l][(b0 + row) * N + col] : 0.f;
          const float v = hv > 0.f ? gt[row * RC_WS + col] : 0.f;
          ds[row * RC_WS + col] = v;
          if (ok) tw.dz[l][(b0 + row) * N + col] = v;
        }
      }
      __syncthreads();
#pragma unroll 1
      for (int l = tw.L - 1; l >= 1; --l) {
        const int Nk = tw.n[l], No = tw.n[l - 1], NT = (No + 15) >> 4;
        rc_f4 acc[RC_TPW][RC_CH];
        rc_clear(acc);
        rc_mma(Ds + (l & 1) * RC_ROWS * RC_WS, RC_WS, Nk, tw.w[l], No, 1, No, 0, wv, q, li, acc);
        float* ds = Ds + ((l - 1) & 1) * RC_ROWS * RC_WS;
#pragma unroll
        for (int u = 0; u < RC_TPW; ++u) {
          const int tile = wv + RC_WAVES * u, col = 16 * tile + li;
          if (tile < NT && col < No) {
            const rc_f4 sum = rc_join(acc[u]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 4 * q + r;
              const bool ok = b0 + row < B;
              const float hv = ok ? tw.h[l - 1][(b0 + row) * No + col] : 0.f;
              const float v = hv > 0.f ? sum[r] : 0.f;
              ds[row * RC_WS + col] = v;
              if (ok) tw.dz[l - 1][(b0 + row) * No + col] = v;
            }
          }
        }
        __syncthreads();
      }
      const int N0 = tw.n[0], KT = (tw.K0 + 15) >> 4;
#pragma unroll 1
      for (int c0 = 0; c0 < KT; c0 += RC_WAVES * RC_TPW) {
        rc_f4 acc[RC_TPW][RC_CH];
        rc_clear(acc);
        rc_mma(Ds, RC_WS, N0, tw.w[0], tw.K0, 1, tw.K0, c0, wv, q, li, acc);
#pragma unroll
        for (int u = 0; u < RC_TPW; ++u) {
          const int tile = c0 + wv + RC_WAVES * u, col = 16 * tile + li;
          if (tile < KT && col < tw.K0) {
            const rc_f4 sum = rc_join(acc[u]);
            int s = 0;
            while (col >= tw.off[s + 1]) ++s;
            const int sc = col - tw.off[s];
            const int d = tw.dep[s > 0 ? s - 1 : 0];
            const bool lds = s > 0 && A.t[d].L > 0;
            float* dxp = s == 0 ? tw.dx : A.t[d].dx;
            const int64_t dxs = s == 0 ? tw.dxs : A.t[d].dxs;
            const bool store = s == 0 || tw.first[s];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 4 * q + r;
              if (lds) {
                Gs[(A.t[d].slot * RC_ROWS + row) * RC_WS + sc] += sum[r];
              } else if (b0 + row < B) {
                float* p = dxp + (b0 + row) * dxs + sc;
                *p = store ? sum[r] : *p + sum[r];
              }
            }
          }
        }
      }
      __syncthreads();  // (Gs and the dx of L = 0 deps before the next tower reads or adds)
    }
  }
}

// grid (max over (t, l) of n-tiles x k-tiles, T x RC_L), RC_WG_THREADS threads
__global__ __launch_bounds__(RC_WG_THREADS) void tzr_relation_chain_wgrad_kernel(RcArgs A, int64_t B) {
  __shared__ float red[RC_WG_WAVES * 256];
  __shared__ float redc[RC_WG_WAVES * TZR_WAVE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int t = blockIdx.y / RC_L, l = blockIdx.y % RC_L;
  if (t >= A.T) return;
  const RcTower& tw = A.t[t];
  if (l >= tw.L) return;
  const int N = tw.n[l], K = l ? tw.n[l - 1] : tw.K0;
  const int NT = (N + 15) >> 4, KT = (K + 15) >> 4;
  if ((int)blockIdx.x >= NT * KT) return;
  const int nt = blockIdx.x / KT, kt = blockIdx.x - nt * KT;
  const int n = 16 * nt + li, kcol = 16 * kt + li;
  const bool nok = n < N, kok = kcol < K;
  const float* pu = tw.x;  // the operand column kcol of u (first layer) or of h_{l-1}
  int64_t su = tw.xs;
  if (l > 0) {
    pu = tw.h[l - 1] + (kok ? kcol : 0);
    su = K;
  } else if (kok) {
    int s = 0;
    while (kcol >= tw.off[s + 1]) ++s;
    if (s > 0) {
      const RcTower& src = A.t[tw.dep[s - 1]];
      pu = src.L > 0 ? src.h[src.L - 1] : src.x;
      su = src.L > 0 ? (int64_t)src.rw : src.xs;
    }
    pu += kcol - tw.off[s];
  }
  const float* pz = tw.dz[l] + (nok ? n : 0);
  rc_f4 acc[RC_WG_UN];
  float cs[RC_WG_UN];
#pragma unroll
  for (int u = 0; u < RC_WG_UN; ++u) acc[u] = rc_zero(), cs[u] = 0.f;
  const int64_t steps = (B + 3) >> 2;
  for (int64_t s0 = wv; s0 < steps; s0 += RC_WG_UN * RC_WG_WAVES) {  // RC_WG_UN of the wave's steps at a time, each on its own chain
    float va[RC_WG_UN], vb[RC_WG_UN];
#pragma unroll
    for (int u = 0; u < RC_WG_UN; ++u) {
      const int64_t b = 4 * (s0 + RC_WG_WAVES * u) + q;
      const bool bok = b < B;
      const float a0 = pz[bok && nok ? b * N : 0];
      const float b1 = pu[bok && kok ? b * su : 0];
      va[u] = bok && nok ? a0 : 0.f;
      vb[u] = bok && kok ? b1 : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RC_WG_UN; ++u) {
      cs[u] += va[u];  // (a step past the batch adds +0)
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[u], vb[u], acc[u], 0, 0, 0);
    }
  }
  const rc_f4 sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wv * 256 + r * 64 + lane] = sum[r];
  redc[wv * TZR_WAVE + lane] = ((cs[0] + cs[1]) + (cs[2] + cs[3])) + ((cs[4] + cs[5]) + (cs[6] + cs[7]));
  __syncthreads();
  if (threadIdx.x < 256) {
    const int e = threadIdx.x;
    const float* p = red + e;
    const float v = ((p[0] + p[256]) + (p[512] + p[768])) + ((p[1024] + p[1280]) + (p[1536] + p[1792]));
    const int r = e >> 6, ln = e & 63;
    const int i = 16 * nt + 4 * (ln >> 4) + r, j = 16 * kt + (ln & 15);  // the tile's row (output unit) and column (input)
    if (i < N && j < K) tw.dw[l][(size_t)i * K + j] = v;
  }
  if (kt == 0 && threadIdx.x < 16 && 16 * nt + (int)threadIdx.x < N) {
    float qs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* p = redc + 16 * k + threadIdx.x;
      qs[k] = ((p[0] + p[64]) + (p[128] + p[192])) + ((p[256] + p[320]) + (p[384] + p[448]));
    }
    tw.db[l][16 * nt + threadIdx.x] = (qs[0] + qs[1]) + (qs[2] + qs[3]);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// sizes, limits, graph, x / W / b / h: what both directions need.  Errors first, limits second.
static int rc_check(const TzrRelationChain* m, RcArgs* A, int* n_slots) {
  if (m->B <= 0 || m->n_towers <= 0) return TZR_ERR_INVALID;
  if (m->n_towers > RC_T) return TZR_ERR_UNSUPPORTED;
  const int T = m->n_towers;
  for (int t = 0; t < T; ++t) {
    if (m->x_width[t] <= 0 || m->n_layers[t] < 0 || m->n_deps[t] < 0) return TZR_ERR_INVALID;
    if (m->n_layers[t] > RC_L || m->n_deps[t] > RC_T) return TZR_ERR_UNSUPPORTED;
    for (int j = 0; j < m->n_deps[t]; ++j) {
      const int d = m->deps[t][j];
      if (d < 0 || d >= t) return TZR_ERR_INVALID;  // an earlier tower
      for (int i = 0; i < j; ++i)
        if (m->deps[t][i] == d) return TZR_ERR_INVALID;  // once
    }
    for (int l = 0; l < m->n_layers[t]; ++l)
      if (m->width[t][l] <= 0) return TZR_ERR_INVALID;
  }
  for (int t = 0; t < T; ++t) {
    if ((m->x_width[t] & 3) || m->x_width[t] > RC_MAXX) return TZR_ERR_UNSUPPORTED;
    for (int l = 0; l < m->n_layers[t]; ++l)
      if ((m->width[t][l] & 3) || m->width[t][l] > RC_MAXW) return TZR_ERR_UNSUPPORTED;
  }
  A->T = T;
  bool read[RC_T] = {};
  for (int t = T - 1; t >= 0; --t) {  // (descending: `first` marks the highest consumer of an L = 0 tower)
    RcTower& w = A->t[t];
    const int L = m->n_layers[t];
    TZR_TRY(tzr_rows_operand(m->x[t], m->x_stride[t], m->x_width[t]));
    w.x = reinterpret_cast<const float*>(m->x[t]);
    w.xs = m->x_stride[t];
    w.hx = m->x_width[t];
    w.L = L;
    w.nd = L > 0 ? m->n_deps[t] : 0;  // (deps without layers: ignored)
    w.rw = L > 0 ? m->width[t][L - 1] : w.hx;
    w.off[0] = 0;
    w.off[1] = w.hx;
    for (int j = 0; j < w.nd; ++j) {
      const int d = m->deps[t][j];
      const int dl = m->n_layers[d];
      w.dep[j] = d;
      w.off[j + 2] = w.off[j + 1] + (dl > 0 ? m->width[d][dl - 1] : m->x_width[d]);
      w.first[j + 1] = dl == 0 && !read[d];
      read[d] = true;
    }
    w.K0 = w.off[w.nd + 1];
    for (int l = 0; l < L; ++l) {
      if (!m->w[t][l] || (m->w[t][l] & 15) || !m->b[t][l] || (m->b[t][l] & 15) || !m->h[t][l] || (m->h[t][l] & 15)) return TZR_ERR_INVALID;
      w.n[l] = m->width[t][l];
      w.w[l] = reinterpret_cast<const float*>(m->w[t][l]);
      w.b[l] = reinterpret_cast<const float*>(m->b[t][l]);
      w.h[l] = reinterpret_cast<float*>(m->h[t][l]);
    }
  }
  int slots = 0;
  for (int t = 0; t < T; ++t) {
    A->t[t].zero_dx = A->t[t].L == 0 && !read[t];
    A->t[t].slot = A->t[t].L > 0 ? slots++ : 0;
  }
  *n_slots = slots;
  return TZR_OK;
}

// the class of a model by its towers with layers: 2 (48.6 KB of LDS forward: three workgroups a CU), 4 (64.9 KB: two) or 8 (97.4 KB: one)
#define RC_BY_CLASS(LAUNCH)      \
  do {                           \
    if (slots <= 2) LAUNCH(2);   \
    else if (slots <= 4) LAUNCH(4); \
    else LAUNCH(8);              \
  } while (0)

static inline unsigned rc_grid(int64_t B) { return (unsigned)std::min<int64_t>((B + RC_ROWS - 1) / RC_ROWS, RC_MAXGRID); }

extern "C" int tzr_relation_chain_fwd(const TzrRelationChain* h_rc, void* stream) {
  if (!h_rc) return TZR_ERR_INVALID;
  RcArgs A = {};
  int slots = 0;
  TZR_TRY(rc_check(h_rc, &A, &slots));
#define RC_FWD(NR_) \
  hipLaunchKernelGGL((tzr_relation_chain_fwd_kernel<NR_>), dim3(rc_grid(h_rc->B)), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream), A, h_rc->B)
  RC_BY_CLASS(RC_FWD);
#undef RC_FWD
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// the pre-activation gradients dz_{t,l} [B, N], each 256-byte aligned
static size_t rc_workspace(const TzrRelationChain* m) {
  size_t off = 0;
  for (int t = 0; t < m->n_towers; ++t)
    for (int l = 0; l < m->n_layers[t]; ++l) off = tzr_align_up(off + (size_t)m->B * (size_t)m->width[t][l] * sizeof(float));
  return off;
}

extern "C" size_t tzr_relation_chain_bwd_workspace(const TzrRelationChain* h_rc) {
  if (!h_rc || h_rc->B <= 0 || h_rc->n_towers <= 0 || h_rc->n_towers > RC_T) return 256;
  for (int t = 0; t < h_rc->n_towers; ++t) {
    if (h_rc->n_layers[t] < 0 || h_rc->n_layers[t] > RC_L) return 256;
    for (int l = 0; l < h_rc->n_layers[t]; ++l)
      if (h_rc->width[t][l] <= 0 || h_rc->width[t][l] > RC_MAXW) return 256;
  }
  return rc_workspace(h_rc) + 256;
}

extern "C" int tzr_relation_chain_bwd(const TzrRelationChain* h_rc, void* stream) {
  if (!h_rc) return TZR_ERR_INVALID;
  RcArgs A = {};
  int slots = 0;
  TZR_TRY(rc_check(h_rc, &A, &slots));
  const int T = h_rc->n_towers;
  int tiles = 0;
  for (int t = 0; t < T; ++t) {
    RcTower& w = A.t[t];
    TZR_TRY(tzr_rows_operand(h_rc->dx[t], h_rc->dx_stride[t], w.hx));
    w.dx = reinterpret_cast<float*>(h_rc->dx[t]);
    w.dxs = h_rc->dx_stride[t];
    if (w.L > 0 && h_rc->grad_r[t]) {
      TZR_TRY(tzr_rows_operand(h_rc->grad_r[t], h_rc->grad_r_stride[t], w.rw));
      w.g = reinterpret_cast<const float*>(h_rc->grad_r[t]);
      w.gs = h_rc->grad_r_stride[t];
    }
    for (int l = 0; l < w.L; ++l) {
      if (!h_rc->dw[t][l] || (h_rc->dw[t][l] & 15) || !h_rc->db[t][l] || (h_rc->db[t][l] & 15)) return TZR_ERR_INVALID;
      w.dw[l] = reinterpret_cast<float*>(h_rc->dw[t][l]);
      w.db[l] = reinterpret_cast<float*>(h_rc->db[t][l]);
      const int K = l ? w.n[l - 1] : w.K0;
      tiles = std::max(tiles, ((w.n[l] + 15) / 16) * ((K + 15) / 16));
    }
  }
  if (!h_rc->ws || (h_rc->ws & 255) || h_rc->ws_bytes < rc_workspace(h_rc)) return TZR_ERR_WORKSPACE;
  TzrCarver carve(reinterpret_cast<void*>(h_rc->ws));
  for (int t = 0; t < T; ++t)
    for (int l = 0; l < A.t[t].L; ++l) A.t[t].dz[l] = carve.take<float>((size_t)h_rc->B * (size_t)A.t[t].n[l]);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define RC_BWD(NR_) hipLaunchKernelGGL((tzr_relation_chain_bwd_rows_kernel<NR_>), dim3(rc_grid(h_rc->B)), dim3(RC_THREADS), 0, s, A, h_rc->B)
  RC_BY_CLASS(RC_BWD);
#undef RC_BWD
  TZR_CHECK_LAUNCH();
  if (tiles > 0) {
    hipLaunchKernelGGL(tzr_relation_chain_wgrad_kernel, dim3((unsigned)tiles, (unsigned)(T * RC_L)), dim3(RC_WG_THREADS), 0, s, A, h_rc->B);
    TZR_CHECK_LAUNCH();
  }
  return TZR_OK;
}
