// HSTU's pointwise-SiLU attention over jagged sequences (tzrec/ops/hstu_attention.py::hstu_mha, the op under the STU layer of
// hstu_match / dlrm_hstu / ultra_hstu), causal, fp32:
//   out[i, h, :] = sum_j valid(i, j) silu(alpha <q[i, h], k[j, h]>) / scale v[j, h, :]        (i, j rows of one sample)
// with the reference's mask (_get_valid_attn_mask: targets, a local window, a contextual prefix) evaluated per element from the
// index rule of include/tzrec_hip.h.  There is no softmax, so no running maximum and no rescale: a score tile is used and dropped.
// A sample has thousands of rows: unlike mwdin / capsule_routing nothing of a sample is resident, every kernel WALKS tiles.
//
// Forward (grid blocks x H x B, 256 threads).  A workgroup owns (sample, head, HS_BLOCK = 64 query rows), wave v the rows 16 v ..
// 16 v + 15.  The wave's Q block stays in registers as the B operand fragments of v_mfma_f32_16x16x4_f32 (lane (li, g) holds the
// float4s at columns 16 ch + 4 g of row li: D / 16 float4s).  K and V tiles of HS_TILE = 16 keys go through LDS once for all four
// waves: every thread fetches its float4s of the NEXT tile into registers before it multiplies the current one and stores them
// into the other LDS buffer behind the multiply: one barrier a tile, rows [16][Da + 4] / [16][Dv + 4] (the + 4 keeps the float4
// reads of sixteen rows off one bank group).  The score tile is computed TRANSPOSED, S^T = K Q^T: accumulator register e of lane
// (li, g) is (key 4 g + e, query li).  After mask, SiLU and scale that register is already the A operand of P V for contraction
// step e, IF step e takes V's row 4 g + e as its B operand (the contraction index may be permuted freely): P never goes through
// LDS.  The 16 x Dv output accumulates in registers (D / 16 accumulators) and is stored once.
//
// Backward, row pass (the forward's grid and walk): dP^T = V dO^T with dO as a second set of register fragments, dS^T = dP^T
// silu'(s) alpha / scale under the mask, dq = dS K with K's rows 4 g + e out of the same LDS tile; dq stored once.
// Backward, column pass: a workgroup owns 64 KEYS (wave v: 16 of them, K and V as register fragments) and walks tiles of 16
// query rows (Q and dO through LDS, the same loader): the score tile UN-transposed, S = Q K^T, register e of lane (li, g) =
// (query 4 g + e, key li), so that the same register trick feeds dv = P^T dO and dk = dS^T Q.  dk, dv stored once.
// Every output element has one owner and one fixed order of additions: no atomics, two runs are bit-equal.  Every score tile
// is recomputed in the backward; nothing of size N x N or [B, H, max_seq_len, .] exists.
//
// Tiles with no valid pair are not visited (hs_row_walk / hs_col_walk: at most two runs of tiles, uniform in the workgroup):
// keys behind the block's last row, keys in front of the window (max_attn_len), target keys in front of the block (a target is
// seen by itself alone); a block with a contextual row walks every non-target key.  Inside a walked tile a wave whose sixteen rows
// all lie in front of the tile's first key (diagonal blocks) skips the multiply.  The walk is a superset: validity is the
// per-element rule.  A workgroup whose block starts at or behind n exits at once; the late (long) blocks are issued first.
// Rows at or behind max_seq_len, and rows outside offsets[0] .. offsets[B], get zeros from the kernels (block 0 of a sample).
//
// HS_NOPK: compiled with packed-fp32-ops off, as mwdin.hip (the accumulator adds stay scalar instructions).
#include "tzr_common.h"

#define HS_THREADS 256
#define HS_BLOCK TZR_HSTU_BLOCK
#define HS_TILE TZR_HSTU_TILE

static_assert(sizeof(TzrHstuAttn) == 264, "TzrHstuAttn: the layout _lib.py mirrors");
static_assert(HS_BLOCK == 64 && HS_TILE == 16, "four waves of one 16 x 16 MFMA tile each");

#if defined(__HIP_DEVICE_COMPILE__)
#define HS_NOPK __attribute__((target("no-packed-fp32-ops")))
#else
#define HS_NOPK
#endif

struct HsOperand {
  float* p;
  int64_t rs, hs;  // floats between rows / between heads
};

struct HsArgs {
  HsOperand q, k, v, out, dout, dq, dk, dv;
  const int64_t* off;
  const int64_t* nt;  // nullable
  int64_t N;
  int B, H, Da, Dv, max_len, L, c, nblk;
  float alpha, inv_scale;
};

struct HsSample {
  int64_t start, len;
  int n, max_id, nts, has_t;  // nts: keys at or behind it are targets (n without targets)
};

__device__ __forceinline__ HsSample hs_sample(const HsArgs& A, int b) {
  HsSample S;
  tzr_jagged_span(A.off, b, b + 1, A.N, &S.start, &S.len);
  S.n = (int)(S.len < (int64_t)A.max_len ? S.len : (int64_t)A.max_len);
  int64_t t = A.nt ? A.nt[b] : 0;
  t = t < -(int64_t)TZR_HSTU_MAX_SEQ_LEN ? -(int64_t)TZR_HSTU_MAX_SEQ_LEN : (t > TZR_HSTU_MAX_SEQ_LEN ? TZR_HSTU_MAX_SEQ_LEN : t);  // (int arithmetic below)
  S.has_t = A.nt != nullptr;
  S.max_id = (A.c > 0 ? S.n - A.c + 1 : S.n) - (int)t;
  const int nts = S.n - (int)t;
  S.nts = nts < 0 ? 0 : (nts > S.n ? S.n : nts);
  return S;
}

__device__ __forceinline__ int hs_id(const HsArgs& A, const HsSample& S, int i) {
  int v = i;
  if (A.c > 0) v = i - A.c + 1 > 0 ? i - A.c + 1 : 0;
  if (S.has_t) v = v < S.max_id ? v : S.max_id;
  return v;
}

// the index rule, row i with id ii against key j with id jj (both inside the sample)
__device__ __forceinline__ bool hs_valid(const HsArgs& A, const HsSample& S, int i, int ii, int j, int jj) {
  const int d = ii - jj;
  bool ok = i == j || d > 0;
  if (A.L > 0) ok = ok && d <= A.L;
  if (A.c > 0) ok = ok || (ii == 0 && jj < S.max_id);
  return ok && i < S.n && j < S.n;
}

// two runs of tiles: a0 .. a0 + na - 1, then b0 .. b0 + nb - 1
struct HsWalk {
  int a0, na, b0, nb;
  bool ctx;  // the block holds a contextual row (forward / row pass); the first run is the contextual rows (column pass)
  __device__ __forceinline__ int tile(int s) const { return s < na ? a0 + s : b0 + (s - na); }
};

// the key tiles of the query rows [r0, r1)
__device__ __forceinline__ HsWalk hs_row_walk(const HsArgs& A, const HsSample& S, int r0, int r1) {
  HsWalk W;
  W.ctx = A.c > 0 && r0 < A.c && S.max_id > 0;
  const int hi = W.ctx ? (r1 > S.nts ? r1 : S.nts) : r1;
  int lo = 0;
  if (A.L > 0 && !W.ctx) {  // the first key whose id reaches id(r0) - L
    const int target = hs_id(A, S, r0) - A.L;
    lo = target <= 0 ? 0 : target + (A.c > 0 ? A.c - 1 : 0);
  }
  const int hit = (hi + HS_TILE - 1) / HS_TILE;
  W.a0 = lo / HS_TILE;
  int a1 = hit;
  if (S.has_t) {  // tiles of targets alone in front of the block's own rows: nothing valid
    a1 = (S.nts + HS_TILE - 1) / HS_TILE;
    a1 = a1 < W.a0 ? W.a0 : (a1 > hit ? hit : a1);
  }
  int b0 = r0 / HS_TILE;
  b0 = b0 < a1 ? a1 : (b0 > hit ? hit : b0);
  W.na = a1 - W.a0, W.b0 = b0, W.nb = hit - b0;
  return W;
}

// the query-row tiles of the keys [c0, c1); c0 a multiple of HS_BLOCK
__device__ __forceinline__ HsWalk hs_col_walk(const HsArgs& A, const HsSample& S, int c0, int c1) {
  HsWalk W;
  W.ctx = A.c > 0 && S.max_id > 0 && c0 < S.nts;  // contextual rows in front of the block see its non-target keys
  const int ct = (A.c + HS_TILE - 1) / HS_TILE, c0t = c0 / HS_TILE;
  W.a0 = 0, W.na = W.ctx ? (ct < c0t ? ct : c0t) : 0;
  int hi = S.n;
  if (S.has_t && c0 >= S.nts) {
    hi = c1;  // targets alone: each seen by itself
  } else if (A.L > 0) {  // the last row whose id stays within id(c1 - 1) + L
    const int target = hs_id(A, S, c1 - 1) + A.L;
    if (!(S.has_t && target >= S.max_id)) {
      const int64_t last = (int64_t)target + (A.c > 0 ? A.c - 1 : 0) + 1;
      hi = last < (int64_t)S.n ? (int)last : S.n;
      hi = hi < c1 ? c1 : hi;
    }
  }
  W.b0 = c0t, W.nb = (hi + HS_TILE - 1) / HS_TILE - c0t;
  return W;
}

// A tile of 16 rows of two operands (X: width wx, Y: width wy) of one (sample, head): global -> registers -> LDS rows
// [16][wx + 4] at 0 and [16][wy + 4] at HS_YB.  Thread t owns the float4s t, t + 256, ..: where they come from and go to is
// worked out once.  Rows at or behind n are zeros; the load itself is unconditional, from a clamped row (no branch around it).
template <int D>
struct HsLoader {
  static constexpr int NP = D / 32;  // 16 rows x 2 D / 4 float4s over 256 threads
  static constexpr int YB = 16 * (D + 4);
  const float* src[NP];
  int64_t rs[NP];
  int row[NP], dst[NP];
  float4 pre[NP];

  __device__ __forceinline__ void setup(const float* x, int64_t xrs, int wx, const float* y, int64_t yrs, int wy) {
    const int x4 = wx >> 2, w4 = x4 + (wy >> 2);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int i = threadIdx.x + p * HS_THREADS;
      const int r = i / w4, cc = i - r * w4;
      const bool isy = cc >= x4;
      row[p] = r < 16 ? r : -1;
      src[p] = r < 16 ? (isy ? y + 4 * (cc - x4) : x + 4 * cc) : x;
      rs[p] = isy && r < 16 ? yrs : xrs;
      dst[p] = isy ? YB + r * (wy + 4) + 4 * (cc - x4) : r * (wx + 4) + 4 * cc;
    }
  }
  __device__ __forceinline__ void fetch(int t0, int n) {  // n >= 1
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = t0 + (row[p] < 0 ? 0 : row[p]);
      const float4 v = tzr_ld4(src[p] + (int64_t)(r < n ? r : n - 1) * rs[p]);
      pre[p] = r < n ? v : tzr_zero4();
    }
  }
  __device__ __forceinline__ void stash(float* buf) const {
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (row[p] >= 0) tzr_st4(buf + dst[p], pre[p]);
  }
};

// the float4 fragments of row `rowp` (null: zeros) at columns 16 ch + 4 g, zeros behind width w
template <int D>
__device__ __forceinline__ void hs_frags(float4* f, const float* rowp, int w, int g) {
#pragma unroll
  for (int ch = 0; ch < D / 16; ++ch) {
    const int a = 16 * ch + 4 * g;
    f[ch] = rowp && a < w ? tzr_ld4(rowp + a) : tzr_zero4();
  }
}

// acc (four chains) += T[li][0 .. w) (an LDS tile, row stride w + 4) against the fragments f: A operand the tile, B the fragments
template <int D>
__device__ __forceinline__ tzr_f32x4 hs_tile_dot(const float* T, int w, const float4* f, int li, int g) {
  tzr_f32x4 acc[4];
  tzr_acc_zero(acc, 4);
  const float* tr = T + li * (w + 4);
#pragma unroll
  for (int ch = 0; ch < D / 16; ++ch) {
    if (16 * ch < w) {
      const int a = 16 * ch + 4 * g;
      const float4 t = tzr_ld4(tr + (a < w ? a : 0));  // (unconditional, from a clamped column: no branch around the read)
      tzr_mfma4(a < w ? t : tzr_zero4(), f[ch], acc);
    }
  }
  return tzr_join4(acc);
}

// o[ct] += p^T-trick: step e takes p[e] as the A operand and T's row 4 g + e as the B operand
template <int D>
__device__ __forceinline__ void hs_tile_acc(tzr_f32x4* o, const tzr_f32x4 p, const float* T, int w, int li, int g) {
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct) {
    if (16 * ct < w) {
      const int col = 16 * ct + li;
      const float* tc = T + 4 * g * (w + 4) + (col < w ? col : 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = tc[e * (w + 4)];
        o[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[e], col < w ? t : 0.f, o[ct], 0, 0, 0);
      }
    }
  }
}

// accumulator register r of lane (li, g) is (row r0 + 4 g + r, column 16 ct + li): rows below n, columns below w
template <int D>
__device__ __forceinline__ void hs_store(const HsOperand& O, const tzr_f32x4* o, int64_t start, int h, int r0, int n, int w, int li, int g) {
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct) {
    const int col = 16 * ct + li;
    if (col < w) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r0 + 4 * g + r < n) O.p[(start + r0 + 4 * g + r) * O.rs + h * O.hs + col] = o[ct][r];
    }
  }
}

// zeros for head h of the rows [lo, hi) of O (width w)
__device__ __forceinline__ void hs_zero_rows(const HsOperand& O, int64_t lo, int64_t hi, int h, int w) {
  const int w4 = w >> 2;
  for (int64_t i = threadIdx.x; i < (hi - lo) * w4; i += HS_THREADS) {
    const int64_t r = i / w4;
    tzr_st4(O.p + (lo + r) * O.rs + h * O.hs + 4 * (i - r * w4), tzr_zero4());
  }
}
// block 0 of a sample: the rows behind max_seq_len; of sample 0 also the rows in front of offsets[0], of sample B - 1 those behind offsets[B]
__device__ __forceinline__ void hs_zero_outside(const HsArgs& A, const HsSample& S, const HsOperand& O, int b, int h, int w) {
  hs_zero_rows(O, S.start + S.n, S.start + S.len, h, w);
  if (b == 0) hs_zero_rows(O, 0, S.start, h, w);
  if (b == A.B - 1) hs_zero_rows(O, S.start + S.len, A.N, h, w);
}

// blockIdx.x -> block (late blocks first), sample, head
__device__ __forceinline__ void hs_decode(const HsArgs& A, int* blk, int* b, int* h) {
  const unsigned x = blockIdx.x, bh = (unsigned)A.B * (unsigned)A.H, u = x / bh, v = x - u * bh;
  *blk = A.nblk - 1 - (int)u;
  *b = (int)(v / (unsigned)A.H);
  *h = (int)(v - (unsigned)*b * (unsigned)A.H);
}

// BWD false: out = P V.  BWD true: dq = dS K.
template <int D, bool BWD>
HS_NOPK __global__ __launch_bounds__(HS_THREADS) void tzr_hstu_rows_kernel(HsArgs A) {
  __shared__ float Sm[2][2 * 16 * (D + 4)];
  constexpr int YB = HsLoader<D>::YB;
  int blk, b, h;
  hs_decode(A, &blk, &b, &h);
  const HsSample S = hs_sample(A, b);
  const HsOperand& O = BWD ? A.dq : A.out;
  const int ow = BWD ? A.Da : A.Dv;
  if (blk == 0) hs_zero_outside(A, S, O, b, h, ow);
  const int r0 = blk * HS_BLOCK;
  if (r0 >= S.n) return;
  const int r1 = r0 + HS_BLOCK < S.n ? r0 + HS_BLOCK : S.n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int w0 = r0 + 16 * wv, i = w0 + li, ii = hs_id(A, S, i);
  float4 qf[D / 16], gf[BWD ? D / 16 : 1];
  hs_frags<D>(qf, i < S.n ? A.q.p + (S.start + i) * A.q.rs + h * A.q.hs : nullptr, A.Da, g);
  if (BWD) hs_frags<D>(gf, i < S.n ? A.dout.p + (S.start + i) * A.dout.rs + h * A.dout.hs : nullptr, A.Dv, g);
  tzr_f32x4 o[D / 16];
  tzr_acc_zero(o, D / 16);
  const HsWalk W = hs_row_walk(A, S, r0, r1);
  const int total = W.na + W.nb;
  HsLoader<D> ld;
  ld.setup(A.k.p + S.start * A.k.rs + h * A.k.hs, A.k.rs, A.Da, A.v.p + S.start * A.v.rs + h * A.v.hs, A.v.rs, A.Dv);
  ld.fetch(W.tile(0) * HS_TILE, S.n);  // (total >= 1: the block's own diagonal tile)
  ld.stash(Sm[0]);
  __syncthreads();
  const float ds_scale = A.alpha * A.inv_scale;
  for (int s = 0; s < total; ++s) {
    const int k0 = W.tile(s) * HS_TILE;
    const float* Ks = Sm[s & 1];
    const float* Vs = Ks + YB;
    if (s + 1 < total) ld.fetch(W.tile(s + 1) * HS_TILE, S.n);
    if (w0 < S.n && (W.ctx || k0 <= w0 + 15)) {  // (uniform in the wave)
      const tzr_f32x4 st = hs_tile_dot<D>(Ks, A.Da, qf, li, g);  // (key 4 g + e, query li)
      tzr_f32x4 p;
      if (!BWD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = k0 + 4 * g + e;
          const float x = A.alpha * st[e];
          p[e] = hs_valid(A, S, i, ii, j, hs_id(A, S, j)) ? x * tzr_sigmoid(x) * A.inv_scale : 0.f;
        }
        hs_tile_acc<D>(o, p, Vs, A.Dv, li, g);
      } else {
        const tzr_f32x4 dp = hs_tile_dot<D>(Vs, A.Dv, gf, li, g);  // dP^T = V dO^T
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = k0 + 4 * g + e;
          const float x = A.alpha * st[e], sg = tzr_sigmoid(x);
          p[e] = hs_valid(A, S, i, ii, j, hs_id(A, S, j)) ? dp[e] * (sg * (1.0f + x * (1.0f - sg))) * ds_scale : 0.f;
        }
        hs_tile_acc<D>(o, p, Ks, A.Da, li, g);
      }
    }
    if (s + 1 < total) ld.stash(Sm[(s + 1) & 1]);
    __syncthreads();
  }
  if (w0 < S.n) hs_store<D>(O, o, S.start, h, w0, S.n, ow, li, g);
}

// dk = dS^T Q, dv = P^T dO for the keys [c0, c0 + 64)
template <int D>
HS_NOPK __global__ __launch_bounds__(HS_THREADS) void tzr_hstu_cols_kernel(HsArgs A) {
  __shared__ float Sm[2][2 * 16 * (D + 4)];
  constexpr int YB = HsLoader<D>::YB;
  int blk, b, h;
  hs_decode(A, &blk, &b, &h);
  blk = A.nblk - 1 - blk;  // (a key block's walk is long when it is EARLY)
  const HsSample S = hs_sample(A, b);
  if (blk == 0) hs_zero_outside(A, S, A.dk, b, h, A.Da), hs_zero_outside(A, S, A.dv, b, h, A.Dv);
  const int c0 = blk * HS_BLOCK;
  if (c0 >= S.n) return;
  const int c1 = c0 + HS_BLOCK < S.n ? c0 + HS_BLOCK : S.n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int w0 = c0 + 16 * wv, j = w0 + li, jj = hs_id(A, S, j);
  float4 kf[D / 16], vf[D / 16];
  hs_frags<D>(kf, j < S.n ? A.k.p + (S.start + j) * A.k.rs + h * A.k.hs : nullptr, A.Da, g);
  hs_frags<D>(vf, j < S.n ? A.v.p + (S.start + j) * A.v.rs + h * A.v.hs : nullptr, A.Dv, g);
  tzr_f32x4 ok_[D / 16], ov[D / 16];
  tzr_acc_zero(ok_, D / 16), tzr_acc_zero(ov, D / 16);
  const HsWalk W = hs_col_walk(A, S, c0, c1);
  const int total = W.na + W.nb;
  HsLoader<D> ld;
  ld.setup(A.q.p + S.start * A.q.rs + h * A.q.hs, A.q.rs, A.Da, A.dout.p + S.start * A.dout.rs + h * A.dout.hs, A.dout.rs, A.Dv);
  ld.fetch(W.tile(0) * HS_TILE, S.n);  // (total >= 1: the block's own diagonal tile)
  ld.stash(Sm[0]);
  __syncthreads();
  const float ds_scale = A.alpha * A.inv_scale;
  for (int s = 0; s < total; ++s) {
    const int q0 = W.tile(s) * HS_TILE;
    const float* Qs = Sm[s & 1];
    const float* Gs = Qs + YB;
    if (s + 1 < total) ld.fetch(W.tile(s + 1) * HS_TILE, S.n);
    if (w0 < S.n && (s < W.na || q0 + 15 >= w0 || (W.ctx && q0 < A.c))) {  // (uniform in the wave)
      const tzr_f32x4 sc = hs_tile_dot<D>(Qs, A.Da, kf, li, g);  // (query 4 g + e, key li)
      const tzr_f32x4 dp = hs_tile_dot<D>(Gs, A.Dv, vf, li, g);  // dP = dO V^T
      tzr_f32x4 p, ds;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = q0 + 4 * g + e;
        const float x = A.alpha * sc[e], sg = tzr_sigmoid(x);
        const bool ok = hs_valid(A, S, i, hs_id(A, S, i), j, jj);
        p[e] = ok ? x * sg * A.inv_scale : 0.f;
        ds[e] = ok ? dp[e] * (sg * (1.0f + x * (1.0f - sg))) * ds_scale : 0.f;
      }
      hs_tile_acc<D>(ov, p, Gs, A.Dv, li, g);
      hs_tile_acc<D>(ok_, ds, Qs, A.Da, li, g);
    }
    if (s + 1 < total) ld.stash(Sm[(s + 1) & 1]);
    __syncthreads();
  }
  if (w0 < S.n) {
    hs_store<D>(A.dk, ok_, S.start, h, w0, S.n, A.Da, li, g);
    hs_store<D>(A.dv, ov, S.start, h, w0, S.n, A.Dv, li, g);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// an [N, H, D] operand by row and head stride: null or misaligned is an error, strides the float4 accesses cannot take (or that
// let two heads or two rows share a float) unsupported
static int hs_operand(uint64_t ptr, int64_t rs, int64_t hs, int H, int D, HsOperand* o) {
  if (!ptr || (ptr & 15)) return TZR_ERR_INVALID;
  if ((rs & 3) || (hs & 3) || hs < D || rs < (int64_t)(H - 1) * hs + D) return TZR_ERR_UNSUPPORTED;
  o->p = reinterpret_cast<float*>(ptr), o->rs = rs, o->hs = hs;
  return TZR_OK;
}

// sizes, limits, then the operands both directions read
static int hs_check(const TzrHstuAttn* m, HsArgs* A) {
  if (m->B < 0 || m->N < 0 || m->max_attn_len < 0 || m->contextual_seq_len < 0) return TZR_ERR_INVALID;
  if (!tzr_dim4_ok(m->Da, TZR_HSTU_MAX_DIM) || !tzr_dim4_ok(m->Dv, TZR_HSTU_MAX_DIM) || m->H < 1 || m->max_seq_len < 1 || m->max_seq_len > TZR_HSTU_MAX_SEQ_LEN ||
      m->max_attn_len > TZR_HSTU_MAX_SEQ_LEN || m->contextual_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->N >= (1ll << 31))
    return TZR_ERR_UNSUPPORTED;
  const int64_t nblk = ((int64_t)m->max_seq_len + HS_BLOCK - 1) / HS_BLOCK;
  if (m->B > 0 && (m->B >= (1ll << 31) / m->H || nblk >= (1ll << 31) / (m->B * m->H))) return TZR_ERR_UNSUPPORTED;  // the grid
  if (m->B == 0 || m->N == 0) return TZR_OK;
  TZR_TRY(hs_operand(m->q, m->q_stride, m->q_head_stride, m->H, m->Da, &A->q));
  TZR_TRY(hs_operand(m->k, m->k_stride, m->k_head_stride, m->H, m->Da, &A->k));
  TZR_TRY(hs_operand(m->v, m->v_stride, m->v_head_stride, m->H, m->Dv, &A->v));
  if (!m->offsets || (m->offsets & 7) || (m->num_targets & 7)) return TZR_ERR_INVALID;
  A->off = reinterpret_cast<const int64_t*>(m->offsets);
  A->nt = reinterpret_cast<const int64_t*>(m->num_targets);
  A->N = m->N, A->B = (int)m->B, A->H = m->H, A->Da = m->Da, A->Dv = m->Dv, A->max_len = m->max_seq_len;
  A->L = m->max_attn_len, A->c = m->contextual_seq_len, A->nblk = (int)nblk;
  A->alpha = m->alpha;
  A->inv_scale = 1.0f / (float)(m->scaling_seqlen > 0 ? m->scaling_seqlen : m->max_seq_len);
  return TZR_OK;
}

// the class of a shape: D covers both widths
#define HS_ROWS_FWD(D) tzr_hstu_rows_kernel<D, false>
#define HS_ROWS_BWD(D) tzr_hstu_rows_kernel<D, true>
#define HS_COLS(D) tzr_hstu_cols_kernel<D>
#define HS_LAUNCH(KERNEL, s, A)                                                                       \
  do {                                                                                                \
    const int wide_ = (A).Da > (A).Dv ? (A).Da : (A).Dv;                                              \
    const dim3 grid_((unsigned)((int64_t)(A).nblk * (A).B * (A).H));                                  \
    if (wide_ <= 32) hipLaunchKernelGGL((KERNEL(32)), grid_, dim3(HS_THREADS), 0, s, A);              \
    else if (wide_ <= 64) hipLaunchKernelGGL((KERNEL(64)), grid_, dim3(HS_THREADS), 0, s, A);         \
    else hipLaunchKernelGGL((KERNEL(128)), grid_, dim3(HS_THREADS), 0, s, A);                         \
  } while (0)

extern "C" int tzr_hstu_attn_fwd(const TzrHstuAttn* h_at, void* stream) {
  if (!h_at) return TZR_ERR_INVALID;
  HsArgs A = {};
  TZR_TRY(hs_check(h_at, &A));
  if (h_at->B == 0 || h_at->N == 0) return TZR_OK;
  TZR_TRY(hs_operand(h_at->out, h_at->out_stride, h_at->out_head_stride, h_at->H, h_at->Dv, &A.out));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HS_LAUNCH(HS_ROWS_FWD, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_hstu_attn_bwd(const TzrHstuAttn* h_at, void* stream) {
  if (!h_at) return TZR_ERR_INVALID;
  HsArgs A = {};
  TZR_TRY(hs_check(h_at, &A));
  if (h_at->B == 0 || h_at->N == 0) return TZR_OK;
  TZR_TRY(hs_operand(h_at->grad_out, h_at->grad_out_stride, h_at->grad_out_head_stride, h_at->H, h_at->Dv, &A.dout));
  TZR_TRY(hs_operand(h_at->dq, h_at->dq_stride, h_at->dq_head_stride, h_at->H, h_at->Da, &A.dq));
  TZR_TRY(hs_operand(h_at->dk, h_at->dk_stride, h_at->dk_head_stride, h_at->H, h_at->Da, &A.dk));
  TZR_TRY(hs_operand(h_at->dv, h_at->dv_stride, h_at->dv_head_stride, h_at->H, h_at->Dv, &A.dv));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HS_LAUNCH(HS_ROWS_BWD, s, A);
  TZR_CHECK_LAUNCH();
  HS_LAUNCH(HS_COLS, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
