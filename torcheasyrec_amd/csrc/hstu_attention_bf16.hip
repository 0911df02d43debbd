// HSTU's jagged pointwise-SiLU attention (csrc/hstu_attention.hip has the operation, the mask and the walk) in bf16 on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulators: bf16 operands and outputs, one launch forward, two backward, no workspace,
// no atomics.  The numeric contract is in include/tzrec_hip.h: fp32 scores, fp32 sigmoid / silu' / mask / scale, P and dS
// rounded ONCE to bf16 as the second product's operand, every output accumulated in fp32 and rounded once at its single store.
//
// One MFMA contracts over 32: lane (li, g) = (lane & 15, lane >> 4) supplies eight consecutive contraction slots 8 g .. 8 g + 7
// of row li (A) or column li (B), and gets D[4 g + r][li] in register r.  A workgroup (256 threads) owns HB_BLOCK = 64 rows,
// wave v sixteen of them, and walks tiles of HB_TILE = 32 rows of the other side.
//
// Forward.  The wave's Q rows are resident as B fragments (lane (li, g): the 16 bytes at columns 32 ch + 8 g of row li, D / 32
// of them; a width that is no multiple of 32 is padded with zero fragments in registers).  A 32-key tile is scored as TWO 16-key
// sub-tiles, each transposed, S^T = K Q^T, and sub-tile t takes the keys 8 (m >> 2) + 4 t + (m & 3) as its rows m = 0 .. 15:
// register r of lane (li, g) is then (key 8 g + 4 t + r, query li), so that the eight registers of the two sub-tiles, after
// mask, SiLU, scale and one pack, ARE the A fragment of P V for the contraction slots 8 g .. 8 g + 7 = the keys 8 g .. 8 g + 7 in
// their natural order.  P never goes through LDS.  The B fragment of P V is eight consecutive KEYS of one V column.
// Backward, row pass: dP^T = V dO^T the same way (dO a second set of resident fragments), dS^T = dP^T silu'(s) alpha / scale
// under the mask, dq = dS K with eight consecutive keys of one K column as the B fragment.
// Backward, column pass: the wave owns 16 keys (K and V resident), walks tiles of 32 query rows, scores UN-transposed,
// S = Q K^T and dP = dO V^T (register r = (query 8 g + 4 t + r, key li)), and the same packed registers feed dv = P^T dO and
// dk = dS^T Q, whose B fragments are eight consecutive QUERY rows of one dO / Q column.
//
// LDS.  The walked side's tile goes through LDS once for all four waves, fetched a tile ahead into registers with 16-byte
// loads (thread -> (row pair, 8-column chunk)) and stored into the other buffer behind the multiply: one barrier a tile.
//   * as score operand (A, contracted over the columns) a tile lies row-major, [32][D + 8] bf16, with row rho stored at position
//     16 t + m (rho = 8 (m >> 2) + 4 t + (m & 3)): the sixteen rows of sub-tile t are consecutive, and with a row stride of
//     D / 2 + 4 dwords their 16-byte reads fall on sixteen different bank groups (rows 16 apart would share one);
//   * as B fragment of the second product (contracted over the tile's ROWS) it lies TRANSPOSED, [D][32 + 8] bf16: the loader
//     holds two consecutive rows of its chunk and stores eight dwords (row 2 p | row 2 p + 1) down the columns; a fragment is
//     then one 16-byte read, and a column stride of 20 dwords spreads sixteen columns over all banks.
//   A transposed STORE, not the transposing LDS reads of gfx950 (ds_read_b64_tr_b16): the tile is written once and read by four
//   waves, so the transpose is paid once instead of in every wave's inner loop, a fragment stays one 16-byte read instead of
//   two 8-byte ones, and the lane emulator of the tests needs no new instruction.  Its price is eight 4-byte LDS stores where
//   one 16-byte store would do; NOTES.md has the reading.
//   Forward: K row-major, V transposed.  Row pass: K both, V row-major.  Column pass: Q and dO both.
// The walk (which tiles, which waves skip a tile), the zeros for rows behind max_seq_len and outside the offsets, and the
// launch order (long blocks first) are the fp32 file's, restated here for 32-row tiles; the fp32 file itself is untouched.
#include "tzr_common.h"
#include "tzr_bf16.h"

#define HB_THREADS 256
#define HB_BLOCK TZR_HSTU_BF16_BLOCK
#define HB_TILE TZR_HSTU_BF16_TILE

static_assert(sizeof(TzrHstuAttn) == 264, "TzrHstuAttn: the layout _lib.py mirrors");
static_assert(HB_BLOCK == 64 && HB_TILE == 32, "four waves of sixteen rows; one bf16 MFMA contracts over a tile");

struct HbOperand {
  uint16_t* p;
  int64_t rs, hs;  // bf16 elements between rows / between heads
};

struct HbArgs {
  HbOperand q, k, v, out, dout, dq, dk, dv;
  const int64_t* off;
  const int64_t* nt;  // nullable
  int64_t N;
  int B, H, Da, Dv, max_len, L, c, nblk;
  float alpha, inv_scale;
};

struct HbSample {
  int64_t start, len;
  int n, max_id, nts, has_t;  // nts: keys at or behind it are targets (n without targets)
};

__device__ __forceinline__ HbSample hb_sample(const HbArgs& A, int b) {
  HbSample S;
  tzr_jagged_span(A.off, b, b + 1, A.N, &S.start, &S.len);
  S.n = (int)(S.len < (int64_t)A.max_len ? S.len : (int64_t)A.max_len);
  int64_t t = A.nt ? A.nt[b] : 0;
  t = t < -(int64_t)TZR_HSTU_MAX_SEQ_LEN ? -(int64_t)TZR_HSTU_MAX_SEQ_LEN : (t > TZR_HSTU_MAX_SEQ_LEN ? TZR_HSTU_MAX_SEQ_LEN : t);
  S.has_t = A.nt != nullptr;
  S.max_id = (A.c > 0 ? S.n - A.c + 1 : S.n) - (int)t;
  const int nts = S.n - (int)t;
  S.nts = nts < 0 ? 0 : (nts > S.n ? S.n : nts);
  return S;
}

__device__ __forceinline__ int hb_id(const HbArgs& A, const HbSample& S, int i) {
  int v = i;
  if (A.c > 0) v = i - A.c + 1 > 0 ? i - A.c + 1 : 0;
  if (S.has_t) v = v < S.max_id ? v : S.max_id;
  return v;
}

// the index rule, row i with id ii against key j with id jj
__device__ __forceinline__ bool hb_valid(const HbArgs& A, const HbSample& S, int i, int ii, int j, int jj) {
  const int d = ii - jj;
  bool ok = i == j || d > 0;
  if (A.L > 0) ok = ok && d <= A.L;
  if (A.c > 0) ok = ok || (ii == 0 && jj < S.max_id);
  return ok && i < S.n && j < S.n;
}

// two runs of tiles: a0 .. a0 + na - 1, then b0 .. b0 + nb - 1
struct HbWalk {
  int a0, na, b0, nb;
  bool ctx;  // the block holds a contextual row (forward / row pass); the first run is the contextual rows (column pass)
  __device__ __forceinline__ int tile(int s) const { return s < na ? a0 + s : b0 + (s - na); }
};

// the key tiles of the query rows [r0, r1)
__device__ __forceinline__ HbWalk hb_row_walk(const HbArgs& A, const HbSample& S, int r0, int r1) {
  HbWalk W;
  W.ctx = A.c > 0 && r0 < A.c && S.max_id > 0;
  const int hi = W.ctx ? (r1 > S.nts ? r1 : S.nts) : r1;
  int lo = 0;
  if (A.L > 0 && !W.ctx) {  // the first key whose id reaches id(r0) - L
    const int target = hb_id(A, S, r0) - A.L;
    lo = target <= 0 ? 0 : target + (A.c > 0 ? A.c - 1 : 0);
  }
  const int hit = (hi + HB_TILE - 1) / HB_TILE;
  W.a0 = lo / HB_TILE;
  int a1 = hit;
  if (S.has_t) {  // tiles of targets alone in front of the block's own rows: nothing valid
    a1 = (S.nts + HB_TILE - 1) / HB_TILE;
    a1 = a1 < W.a0 ? W.a0 : (a1 > hit ? hit : a1);
  }
  int b0 = r0 / HB_TILE;
  b0 = b0 < a1 ? a1 : (b0 > hit ? hit : b0);
  W.na = a1 - W.a0, W.b0 = b0, W.nb = hit - b0;
  return W;
}

// the query-row tiles of the keys [c0, c1); c0 a multiple of HB_BLOCK
__device__ __forceinline__ HbWalk hb_col_walk(const HbArgs& A, const HbSample& S, int c0, int c1) {
  HbWalk W;
  W.ctx = A.c > 0 && S.max_id > 0 && c0 < S.nts;  // contextual rows in front of the block see its non-target keys
  const int ct = (A.c + HB_TILE - 1) / HB_TILE, c0t = c0 / HB_TILE;
  W.a0 = 0, W.na = W.ctx ? (ct < c0t ? ct : c0t) : 0;
  int hi = S.n;
  if (S.has_t && c0 >= S.nts) {
    hi = c1;  // targets alone: each seen by itself
  } else if (A.L > 0) {  // the last row whose id stays within id(c1 - 1) + L
    const int target = hb_id(A, S, c1 - 1) + A.L;
    if (!(S.has_t && target >= S.max_id)) {
      const int64_t last = (int64_t)target + (A.c > 0 ? A.c - 1 : 0) + 1;
      hi = last < (int64_t)S.n ? (int)last : S.n;
      hi = hi < c1 ? c1 : hi;
    }
  }
  W.b0 = c0t, W.nb = (hi + HB_TILE - 1) / HB_TILE - c0t;
  return W;
}

// the LDS position of tile row rho (even rho: rho + 1 follows it)
__device__ __forceinline__ int hb_pos(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }

// A tile of 32 rows of two operands (X: width wx, Y: width wy) of one (sample, head): global -> registers -> LDS, X row-major
// always, X transposed / Y row-major / Y transposed as asked.  An item is (8-column chunk, row pair): thread t owns the items
// t, t + 256, ..; sixteen consecutive threads hold the sixteen row pairs of one chunk, so that their transposed dword stores
// are consecutive.  Rows at or behind n are zeros; the loads themselves are unconditional, from a clamped row.
template <int D, bool XT, bool YR, bool YT>
struct HbLoader {
  static constexpr int RS = D + 8, TS = HB_TILE + 8;
  static constexpr int NP = D >= 64 ? D / 64 : 1;  // 16 row pairs x 2 D / 8 chunks over 256 threads
  static constexpr int XR_AT = 0, XT_AT = HB_TILE * RS, YR_AT = XT_AT + (XT ? D * TS : 0), YT_AT = YR_AT + (YR ? HB_TILE * RS : 0);
  static constexpr int SIZE = YT_AT + (YT ? D * TS : 0);
  const uint16_t* src[NP];
  int64_t rs[NP];
  int row[NP], rat[NP], tat[NP];  // the pair's first row (-1: no item), where it goes row-major / transposed (-1: nowhere)
  tzr_u32x4 pre[NP][2];

  __device__ __forceinline__ void setup(const uint16_t* x, int64_t xrs, int wx, const uint16_t* y, int64_t yrs, int wy) {
    const int x8 = wx >> 3, n8 = x8 + (wy >> 3);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int i = threadIdx.x + p * HB_THREADS;
      const int c = i >> 4, r2 = 2 * (i & 15);
      const bool act = c < n8, isy = c >= x8;
      const int col = 8 * (isy ? c - x8 : c);
      row[p] = act ? r2 : -1;
      src[p] = act ? (isy ? y + col : x + col) : x;
      rs[p] = act && isy ? yrs : xrs;
      const int ra = hb_pos(r2) * RS + col, ta = col * TS + r2;
      rat[p] = isy ? (YR ? YR_AT + ra : -1) : XR_AT + ra;
      tat[p] = isy ? (YT ? YT_AT + ta : -1) : (XT ? XT_AT + ta : -1);
    }
  }
  __device__ __forceinline__ void fetch(int t0, int n) {  // n >= 1
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = t0 + (row[p] < 0 ? 0 : row[p]);
      const tzr_u32x4 a = tzr_ldg16(src[p] + (int64_t)(r < n ? r : n - 1) * rs[p]);
      const tzr_u32x4 b = tzr_ldg16(src[p] + (int64_t)(r + 1 < n ? r + 1 : n - 1) * rs[p]);
      pre[p][0] = r < n ? a : tzr_zero16();
      pre[p][1] = r + 1 < n ? b : tzr_zero16();
    }
  }
  __device__ __forceinline__ void stash(uint16_t* buf) const {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (row[p] < 0) continue;
      const tzr_u32x4 a = pre[p][0], b = pre[p][1];
      if (rat[p] >= 0) {
        tzr_st16(buf + rat[p], a);
        tzr_st16(buf + rat[p] + RS, b);
      }
      if ((XT || YT) && tat[p] >= 0) {
        uint32_t* t = reinterpret_cast<uint32_t*>(buf + tat[p]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // columns 2 j and 2 j + 1 of the chunk: (row 2 p | row 2 p + 1)
          t[(2 * j) * (TS / 2)] = (a[j] & 0xffffu) | (b[j] << 16);
          t[(2 * j + 1) * (TS / 2)] = (a[j] >> 16) | (b[j] & 0xffff0000u);
        }
      }
    }
  }
};

// the resident fragments of row `rowp` (null: zeros): the 16 bytes at columns 32 ch + 8 g, zeros behind width w
template <int D>
__device__ __forceinline__ void hb_frags(tzr_u32x4* f, const uint16_t* rowp, int w, int g) {
#pragma unroll
  for (int ch = 0; ch < D / 32; ++ch) {
    const int a = 32 * ch + 8 * g;
    f[ch] = rowp && a < w ? tzr_ldg16(rowp + a) : tzr_zero16();
  }
}

// s[t] = the 16 x 16 product of sub-tile t of the row-major LDS tile T (A operand: the row at position 16 t + li, width w)
// and the fragments f (B operand): register r of lane (li, g) is (tile row 8 g + 4 t + r, resident row li)
template <int D>
__device__ __forceinline__ void hb_scores(tzr_f32x4* s, const uint16_t* T, int w, const tzr_u32x4* f, int li, int g) {
  s[0] = tzr_acc_zero(), s[1] = tzr_acc_zero();
  const uint16_t* tr = T + li * (D + 8);
#pragma unroll
  for (int ch = 0; ch < D / 32; ++ch) {
    if (32 * ch < w) {
      const int a = 32 * ch + 8 * g;
      const bool in = a < w;
      const tzr_u32x4 t0 = tzr_ld16(tr + (in ? a : 0)), t1 = tzr_ld16(tr + 16 * (D + 8) + (in ? a : 0));  // (unconditional, from a clamped column)
      s[0] = tzr_mfma_bf16(in ? t0 : tzr_zero16(), f[ch], s[0]);
      s[1] = tzr_mfma_bf16(in ? t1 : tzr_zero16(), f[ch], s[1]);
    }
  }
}

// o[ct] += p (A fragment: resident row li against the tile rows 8 g .. 8 g + 7) times the transposed LDS tile TT (B fragment:
// those rows of column 16 ct + li)
template <int D>
__device__ __forceinline__ void hb_acc(tzr_f32x4* o, const tzr_u32x4 p, const uint16_t* TT, int w, int li, int g) {
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct) {
    if (16 * ct < w) {
      const int col = 16 * ct + li;
      const tzr_u32x4 t = tzr_ld16(TT + (col < w ? col : 0) * (HB_TILE + 8) + 8 * g);
      o[ct] = tzr_mfma_bf16(p, col < w ? t : tzr_zero16(), o[ct]);
    }
  }
}

// accumulator register r of lane (li, g) is (row r0 + 4 g + r, column 16 ct + li): rows below n, columns below w; the one rounding
template <int D>
__device__ __forceinline__ void hb_store(const HbOperand& O, const tzr_f32x4* o, int64_t start, int h, int r0, int n, int w, int li, int g) {
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct) {
    const int col = 16 * ct + li;
    if (col < w) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r0 + 4 * g + r < n) tzr_stg2(O.p + (start + r0 + 4 * g + r) * O.rs + h * O.hs + col, tzr_bf16_rne(o[ct][r]));
    }
  }
}

// zeros for head h of the rows [lo, hi) of O (width w)
__device__ __forceinline__ void hb_zero_rows(const HbOperand& O, int64_t lo, int64_t hi, int h, int w) {
  const int w8 = w >> 3;
  for (int64_t i = threadIdx.x; i < (hi - lo) * w8; i += HB_THREADS) {
    const int64_t r = i / w8;
    tzr_stg16(O.p + (lo + r) * O.rs + h * O.hs + 8 * (i - r * w8), tzr_zero16());
  }
}
// block 0 of a sample: the rows behind max_seq_len; of sample 0 also the rows in front of offsets[0], of sample B - 1 those behind offsets[B]
__device__ __forceinline__ void hb_zero_outside(const HbArgs& A, const HbSample& S, const HbOperand& O, int b, int h, int w) {
  hb_zero_rows(O, S.start + S.n, S.start + S.len, h, w);
  if (b == 0) hb_zero_rows(O, 0, S.start, h, w);
  if (b == A.B - 1) hb_zero_rows(O, S.start + S.len, A.N, h, w);
}

// blockIdx.x -> block (late blocks first), sample, head
__device__ __forceinline__ void hb_decode(const HbArgs& A, int* blk, int* b, int* h) {
  const unsigned x = blockIdx.x, bh = (unsigned)A.B * (unsigned)A.H, u = x / bh, v = x - u * bh;
  *blk = A.nblk - 1 - (int)u;
  *b = (int)(v / (unsigned)A.H);
  *h = (int)(v - (unsigned)*b * (unsigned)A.H);
}

// BWD false: out = P V.  BWD true: dq = dS K.
template <int D, bool BWD>
__global__ __launch_bounds__(HB_THREADS) void tzr_hstu_bf16_rows_kernel(HbArgs A) {
  typedef HbLoader<D, BWD, BWD, !BWD> Ld;  // K row-major (+ transposed), V transposed (row-major)
  __shared__ uint16_t Sm[2][Ld::SIZE] __attribute__((aligned(16)));
  int blk, b, h;
  hb_decode(A, &blk, &b, &h);
  const HbSample S = hb_sample(A, b);
  const HbOperand& O = BWD ? A.dq : A.out;
  const int ow = BWD ? A.Da : A.Dv;
  if (blk == 0) hb_zero_outside(A, S, O, b, h, ow);
  const int r0 = blk * HB_BLOCK;
  if (r0 >= S.n) return;
  const int r1 = r0 + HB_BLOCK < S.n ? r0 + HB_BLOCK : S.n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int w0 = r0 + 16 * wv, i = w0 + li, ii = hb_id(A, S, i);
  tzr_u32x4 qf[D / 32], gf[BWD ? D / 32 : 1];
  hb_frags<D>(qf, i < S.n ? A.q.p + (S.start + i) * A.q.rs + h * A.q.hs : nullptr, A.Da, g);
  if (BWD) hb_frags<D>(gf, i < S.n ? A.dout.p + (S.start + i) * A.dout.rs + h * A.dout.hs : nullptr, A.Dv, g);
  tzr_f32x4 o[D / 16];
  tzr_acc_zero(o, D / 16);
  const HbWalk W = hb_row_walk(A, S, r0, r1);
  const int total = W.na + W.nb;
  Ld ld;
  ld.setup(A.k.p + S.start * A.k.rs + h * A.k.hs, A.k.rs, A.Da, A.v.p + S.start * A.v.rs + h * A.v.hs, A.v.rs, A.Dv);
  ld.fetch(W.tile(0) * HB_TILE, S.n);  // (total >= 1: the block's own diagonal tile)
  ld.stash(Sm[0]);
  __syncthreads();
  const float ds_scale = A.alpha * A.inv_scale;
  for (int s = 0; s < total; ++s) {
    const int k0 = W.tile(s) * HB_TILE;
    const uint16_t* T = Sm[s & 1];
    if (s + 1 < total) ld.fetch(W.tile(s + 1) * HB_TILE, S.n);
    if (w0 < S.n && (W.ctx || k0 <= w0 + 15)) {  // (uniform in the wave)
      tzr_f32x4 st[2], p[2];
      hb_scores<D>(st, T + Ld::XR_AT, A.Da, qf, li, g);  // (key 8 g + 4 t + r, query li)
      if (!BWD) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int j = k0 + 8 * g + e;
          const float x = A.alpha * st[e >> 2][e & 3];
          p[e >> 2][e & 3] = hb_valid(A, S, i, ii, j, hb_id(A, S, j)) ? x * tzr_sigmoid(x) * A.inv_scale : 0.f;
        }
        hb_acc<D>(o, tzr_pack_bf16x8(p[0], p[1]), T + Ld::YT_AT, A.Dv, li, g);
      } else {
        tzr_f32x4 dp[2];
        hb_scores<D>(dp, T + Ld::YR_AT, A.Dv, gf, li, g);  // dP^T = V dO^T
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int j = k0 + 8 * g + e;
          const float x = A.alpha * st[e >> 2][e & 3], sg = tzr_sigmoid(x);
          p[e >> 2][e & 3] = hb_valid(A, S, i, ii, j, hb_id(A, S, j)) ? dp[e >> 2][e & 3] * (sg * (1.0f + x * (1.0f - sg))) * ds_scale : 0.f;
        }
        hb_acc<D>(o, tzr_pack_bf16x8(p[0], p[1]), T + Ld::XT_AT, A.Da, li, g);
      }
    }
    if (s + 1 < total) ld.stash(Sm[(s + 1) & 1]);
    __syncthreads();
  }
  if (w0 < S.n) hb_store<D>(O, o, S.start, h, w0, S.n, ow, li, g);
}

// dk = dS^T Q, dv = P^T dO for the keys [c0, c0 + 64)
template <int D>
__global__ __launch_bounds__(HB_THREADS, 2) void tzr_hstu_bf16_cols_kernel(HbArgs A) {
  typedef HbLoader<D, true, true, true> Ld;  // Q and dO, each row-major and transposed
  __shared__ uint16_t Sm[2][Ld::SIZE] __attribute__((aligned(16)));
  int blk, b, h;
  hb_decode(A, &blk, &b, &h);
  blk = A.nblk - 1 - blk;  // (a key block's walk is long when it is EARLY)
  const HbSample S = hb_sample(A, b);
  if (blk == 0) hb_zero_outside(A, S, A.dk, b, h, A.Da), hb_zero_outside(A, S, A.dv, b, h, A.Dv);
  const int c0 = blk * HB_BLOCK;
  if (c0 >= S.n) return;
  const int c1 = c0 + HB_BLOCK < S.n ? c0 + HB_BLOCK : S.n;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int w0 = c0 + 16 * wv, j = w0 + li, jj = hb_id(A, S, j);
  tzr_u32x4 kf[D / 32], vf[D / 32];
  hb_frags<D>(kf, j < S.n ? A.k.p + (S.start + j) * A.k.rs + h * A.k.hs : nullptr, A.Da, g);
  hb_frags<D>(vf, j < S.n ? A.v.p + (S.start + j) * A.v.rs + h * A.v.hs : nullptr, A.Dv, g);
  tzr_f32x4 ok_[D / 16], ov[D / 16];
  tzr_acc_zero(ok_, D / 16), tzr_acc_zero(ov, D / 16);
  const HbWalk W = hb_col_walk(A, S, c0, c1);
  const int total = W.na + W.nb;
  Ld ld;
  ld.setup(A.q.p + S.start * A.q.rs + h * A.q.hs, A.q.rs, A.Da, A.dout.p + S.start * A.dout.rs + h * A.dout.hs, A.dout.rs, A.Dv);
  ld.fetch(W.tile(0) * HB_TILE, S.n);  // (total >= 1: the block's own diagonal tile)
  ld.stash(Sm[0]);
  __syncthreads();
  const float ds_scale = A.alpha * A.inv_scale;
  for (int s = 0; s < total; ++s) {
    const int q0 = W.tile(s) * HB_TILE;
    const uint16_t* T = Sm[s & 1];
    if (s + 1 < total) ld.fetch(W.tile(s + 1) * HB_TILE, S.n);
    if (w0 < S.n && (s < W.na || q0 + HB_TILE - 1 >= w0 || (W.ctx && q0 < A.c))) {  // (uniform in the wave)
      tzr_f32x4 sc[2], dp[2], p[2], ds[2];
      hb_scores<D>(sc, T + Ld::XR_AT, A.Da, kf, li, g);  // (query 8 g + 4 t + r, key li)
      hb_scores<D>(dp, T + Ld::YR_AT, A.Dv, vf, li, g);  // dP = dO V^T
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = q0 + 8 * g + e;
        const float x = A.alpha * sc[e >> 2][e & 3], sg = tzr_sigmoid(x);
        const bool ok = hb_valid(A, S, i, hb_id(A, S, i), j, jj);
        p[e >> 2][e & 3] = ok ? x * sg * A.inv_scale : 0.f;
        ds[e >> 2][e & 3] = ok ? dp[e >> 2][e & 3] * (sg * (1.0f + x * (1.0f - sg))) * ds_scale : 0.f;
      }
      hb_acc<D>(ov, tzr_pack_bf16x8(p[0], p[1]), T + Ld::YT_AT, A.Dv, li, g);
      hb_acc<D>(ok_, tzr_pack_bf16x8(ds[0], ds[1]), T + Ld::XT_AT, A.Da, li, g);
    }
    if (s + 1 < total) ld.stash(Sm[(s + 1) & 1]);
    __syncthreads();
  }
  if (w0 < S.n) {
    hb_store<D>(A.dk, ok_, S.start, h, w0, S.n, A.Da, li, g);
    hb_store<D>(A.dv, ov, S.start, h, w0, S.n, A.Dv, li, g);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// an [N, H, D] bf16 operand by row and head stride: null or misaligned is an error, strides the 16-byte accesses cannot take
// (or that let two heads or two rows share an element) unsupported
static int hb_operand(uint64_t ptr, int64_t rs, int64_t hs, int H, int D, HbOperand* o) {
  if (!ptr || (ptr & 15)) return TZR_ERR_INVALID;
  if ((rs & 7) || (hs & 7) || hs < D || rs < (int64_t)(H - 1) * hs + D) return TZR_ERR_UNSUPPORTED;
  o->p = reinterpret_cast<uint16_t*>(ptr), o->rs = rs, o->hs = hs;
  return TZR_OK;
}

// sizes, limits, then the operands both directions read (the order of hstu_attention.hip's hs_check)
static int hb_check(const TzrHstuAttn* m, HbArgs* A) {
  if (m->B < 0 || m->N < 0 || m->max_attn_len < 0 || m->contextual_seq_len < 0) return TZR_ERR_INVALID;
  if (!tzr_dim8_ok(m->Da, TZR_HSTU_MAX_DIM) || !tzr_dim8_ok(m->Dv, TZR_HSTU_MAX_DIM) || m->H < 1 || m->max_seq_len < 1 || m->max_seq_len > TZR_HSTU_MAX_SEQ_LEN ||
      m->max_attn_len > TZR_HSTU_MAX_SEQ_LEN || m->contextual_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->N >= (1ll << 31))
    return TZR_ERR_UNSUPPORTED;
  const int64_t nblk = ((int64_t)m->max_seq_len + HB_BLOCK - 1) / HB_BLOCK;
  if (m->B > 0 && (m->B >= (1ll << 31) / m->H || nblk >= (1ll << 31) / (m->B * m->H))) return TZR_ERR_UNSUPPORTED;  // the grid
  if (m->B == 0 || m->N == 0) return TZR_OK;
  TZR_TRY(hb_operand(m->q, m->q_stride, m->q_head_stride, m->H, m->Da, &A->q));
  TZR_TRY(hb_operand(m->k, m->k_stride, m->k_head_stride, m->H, m->Da, &A->k));
  TZR_TRY(hb_operand(m->v, m->v_stride, m->v_head_stride, m->H, m->Dv, &A->v));
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
#define HB_ROWS_FWD(D) tzr_hstu_bf16_rows_kernel<D, false>
#define HB_ROWS_BWD(D) tzr_hstu_bf16_rows_kernel<D, true>
#define HB_COLS(D) tzr_hstu_bf16_cols_kernel<D>
#define HB_LAUNCH(KERNEL, s, A)                                                                       \
  do {                                                                                                \
    const int wide_ = (A).Da > (A).Dv ? (A).Da : (A).Dv;                                              \
    const dim3 grid_((unsigned)((int64_t)(A).nblk * (A).B * (A).H));                                  \
    if (wide_ <= 32) hipLaunchKernelGGL((KERNEL(32)), grid_, dim3(HB_THREADS), 0, s, A);              \
    else if (wide_ <= 64) hipLaunchKernelGGL((KERNEL(64)), grid_, dim3(HB_THREADS), 0, s, A);         \
    else hipLaunchKernelGGL((KERNEL(128)), grid_, dim3(HB_THREADS), 0, s, A);                         \
  } while (0)

extern "C" int tzr_hstu_attn_bf16_fwd(const TzrHstuAttn* h_at, void* stream) {
  if (!h_at) return TZR_ERR_INVALID;
  HbArgs A = {};
  TZR_TRY(hb_check(h_at, &A));
  if (h_at->B == 0 || h_at->N == 0) return TZR_OK;
  TZR_TRY(hb_operand(h_at->out, h_at->out_stride, h_at->out_head_stride, h_at->H, h_at->Dv, &A.out));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HB_LAUNCH(HB_ROWS_FWD, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_hstu_attn_bf16_bwd(const TzrHstuAttn* h_at, void* stream) {
  if (!h_at) return TZR_ERR_INVALID;
  HbArgs A = {};
  TZR_TRY(hb_check(h_at, &A));
  if (h_at->B == 0 || h_at->N == 0) return TZR_OK;
  TZR_TRY(hb_operand(h_at->grad_out, h_at->grad_out_stride, h_at->grad_out_head_stride, h_at->H, h_at->Dv, &A.dout));
  TZR_TRY(hb_operand(h_at->dq, h_at->dq_stride, h_at->dq_head_stride, h_at->H, h_at->Da, &A.dq));
  TZR_TRY(hb_operand(h_at->dk, h_at->dk_stride, h_at->dk_head_stride, h_at->H, h_at->Da, &A.dk));
  TZR_TRY(hb_operand(h_at->dv, h_at->dv_stride, h_at->dv_head_stride, h_at->H, h_at->Dv, &A.dv));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HB_LAUNCH(HB_ROWS_BWD, s, A);
  TZR_CHECK_LAUNCH();
  HB_LAUNCH(HB_COLS, s, A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
