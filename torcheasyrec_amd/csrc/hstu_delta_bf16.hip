// HSTU's delta attention (csrc/hstu_delta.hip has the operation, the two segments, the mask and the walk) in bf16 on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulators, forward only: delta_q, k, v, k_delta, v_delta and out are bf16, strides count
// bf16 elements, the struct and the workspace are the fp32 entry's.  The numeric contract is the one include/tzrec_hip.h states
// for tzr_hstu_attn_bf16_*: fp32 scores, fp32 sigmoid / mask / scale, P rounded ONCE to bf16 as the second product's operand, the
// output accumulated in fp32 over all its keys -- across waves, and across chunks in the workspace -- and rounded once at its
// single store.  A serving step reads every cached K and V row once for 1 .. 32 query rows: its cost is the bytes of the cache,
// which bf16 halves.
//
// The work split is the fp32 file's.  Grid chunks x ceil(delta / 16) x B x H, 256 threads; a workgroup owns (sample, head, 16
// delta rows, HDB_CHUNK keys); the Q tile is resident as B fragments (lane (li, g) = (lane & 15, lane >> 4): the 16 bytes at
// columns 32 ch + 8 g of query li, a width that is no multiple of 32 padded with zero fragments in registers).  Wave w takes the
// 32-key tiles w, w + 4, .. of the chunk: no two waves share a tile.  A tile is scored as two transposed 16-key sub-tiles with the
// row permutation of hstu_attention_bf16.hip (sub-tile t takes the keys 8 (m >> 2) + 4 t + (m & 3) as its rows m): register r of
// lane (li, g) is (key 8 g + 4 t + r, query li), so after mask, SiLU, scale and one pack the lane's eight registers ARE the A
// fragment of P V for the keys 8 g .. 8 g + 7.  P never leaves registers, and K needs no LDS: lane (li, g) of sub-tile t loads the
// 16 bytes at columns 32 ch + 8 g of its key row straight from global memory as the A fragment of the scores.
//
// The B fragment of P V is eight consecutive KEYS of one V column, and V's rows lie along the columns: whatever the instruction,
// a contraction over keys wants a transpose of the V tile.  The tiles are wave-private here, so -- unlike the full attention,
// whose tile is transposed once for four waves -- every wave pays for its own.  It is paid as a TRANSPOSED STORE into a
// wave-private stash in LDS, Vt[wave][Dv][32 + 8] bf16 with the column stride of hstu_attention_bf16.hip (20 dwords: sixteen
// columns fall on all banks): lane (li, g) fetches the 16 bytes at columns 8 (g + 4 p) of the two rows 2 li, 2 li + 1 of the NEXT
// tile from global memory before the current tile's multiplies, and stores eight dwords (row 2 li | row 2 li + 1) down the
// columns behind them; a fragment is then ONE 16-byte LDS read per (column, g).  Why this way: the alternatives were (1) the
// transposing LDS reads of gfx950 (ds_read_b64_tr_b16) on a row-major stash -- two 8-byte reads a fragment in the inner loop and an
// instruction the lane emulator of tests/ has no body for; (2) a transpose in registers by cross-lane moves -- a lane needs
// values of eight other lanes per fragment, 4 bytes a move, and the moves run on the LDS hardware anyway; (3) a stash shared by
// the workgroup -- one transpose for four waves, but then the four waves walk the SAME tile and the keys are split over workgroups
// alone: a quarter of the loads in flight per workgroup on a path whose cost is the bytes.  The price of the stash is 32 dword
// stores a lane and tile at D = 128, against 64 MFMAs and 4 KB of global loads a lane group; NOTES.md has the reading.
// The stash's store and its reads are ordered by __syncthreads() (what the emulator's fibers honour); the tile loop therefore has
// ONE trip count for all four waves (HDB_CT / 4) and each wave's work is predicated on its tile lying in the walk.
//
// Each wave's 16 x Dv fp32 partial goes to LDS once; the four are added in wave order 0 .. 3.  With one chunk the sum is rounded
// and stored to `out`; with more it goes, in fp32, into ws[chunk][B delta][H][Dv] (tzr_hstu_delta_workspace: the fp32 entry's
// layout and size) and tzr_hstu_delta_bf16_finish_kernel adds the chunks a sample has in order 0, 1, .. in fp32, rounds once and
// stores.  No atomics: two runs are bit-equal, and so are the two forms on the same rows.  Key tiles with no valid pair are skipped
// by hdb_row_walk (hd_row_walk restated for 32-key tiles): a superset, validity is the per-element rule.  A sample with n >
// max_seq_len or n < delta gets zeros: no key row of it is read.
#include "tzr_common.h"
#include "tzr_bf16.h"

#define HDB_THREADS 256
#define HDB_ROWS 16  // delta rows a workgroup
#define HDB_TILE 32  // keys a tile: the contraction depth of one bf16 MFMA
#define HDB_CHUNK TZR_HSTU_DELTA_CHUNK
#define HDB_CT (HDB_CHUNK / HDB_TILE)  // tiles a chunk
#define HDB_TS (HDB_TILE + 8)          // bf16 between the columns of the transposed stash

static_assert(sizeof(TzrHstuDelta) == 232, "TzrHstuDelta: the layout _lib.py mirrors");
static_assert(HDB_CHUNK % (4 * HDB_TILE) == 0, "a chunk is whole tiles, the same number for each of the four waves");

struct HdbOperand {
  uint16_t* p;
  int64_t rs, hs;  // bf16 elements between rows / between heads
};

struct HdbArgs {
  HdbOperand q, k, v, kd, vd, out;  // kd.p null: one segment
  const int64_t* off;
  const int64_t* nt;  // nullable
  float* ws;
  int64_t Nc;
  int B, H, Da, Dv, delta, max_len, L, c, ntile, nchunk;
  float alpha, inv_scale;
};

// The sample, mask and walk helpers of hstu_delta.hip, restated on this file's argument struct.
struct HdbSample {
  int64_t start;
  int n, n1, max_id, nts, has_t;  // n1: cached rows (n in the one-segment form); nts: keys at or behind it are targets
  bool ok;                        // delta <= n <= max_seq_len
};

// the rows of sample b: first cached row, cached rows, and n (-1: refused)
__device__ __forceinline__ int hdb_rows(const HdbArgs& A, int b, int64_t* start, int64_t* len) {
  tzr_jagged_span(A.off, b, b + 1, A.Nc, start, len);
  const int64_t n = *len + (A.kd.p ? A.delta : 0);
  return n <= (int64_t)A.max_len && n >= (int64_t)A.delta ? (int)n : -1;
}

__device__ __forceinline__ HdbSample hdb_sample(const HdbArgs& A, int b) {
  HdbSample S;
  int64_t len;
  const int n = hdb_rows(A, b, &S.start, &len);
  S.ok = n >= 0;
  S.n = S.ok ? n : 0;
  S.n1 = A.kd.p && S.ok ? (int)len : S.n;
  int64_t t = A.nt ? A.nt[b] : 0;
  t = t < -(int64_t)TZR_HSTU_MAX_SEQ_LEN ? -(int64_t)TZR_HSTU_MAX_SEQ_LEN : (t > TZR_HSTU_MAX_SEQ_LEN ? TZR_HSTU_MAX_SEQ_LEN : t);  // (int arithmetic below)
  S.has_t = A.nt != nullptr;
  S.max_id = (A.c > 0 ? S.n - A.c + 1 : S.n) - (int)t;
  const int nts = S.n - (int)t;
  S.nts = nts < 0 ? 0 : (nts > S.n ? S.n : nts);
  return S;
}

__device__ __forceinline__ int hdb_id(const HdbArgs& A, const HdbSample& S, int i) {
  int v = i;
  if (A.c > 0) v = i - A.c + 1 > 0 ? i - A.c + 1 : 0;
  if (S.has_t) v = v < S.max_id ? v : S.max_id;
  return v;
}

// the index rule, row i with id ii against key j with id jj
__device__ __forceinline__ bool hdb_valid(const HdbArgs& A, const HdbSample& S, int i, int ii, int j, int jj) {
  const int d = ii - jj;
  bool ok = i == j || d > 0;
  if (A.L > 0) ok = ok && d <= A.L;
  if (A.c > 0) ok = ok || (ii == 0 && jj < S.max_id);
  return ok && i < S.n && j < S.n;
}

// the 32-key tiles of the query rows [r0, r1): two runs, [a0, a1) and [b0, b1), the second at or behind the first
struct HdbWalk {
  int a0, a1, b0, b1;
  __device__ __forceinline__ bool has(int t) const { return (t >= a0 && t < a1) || (t >= b0 && t < b1); }
};

__device__ __forceinline__ HdbWalk hdb_row_walk(const HdbArgs& A, const HdbSample& S, int r0, int r1) {
  HdbWalk W;
  const bool ctx = A.c > 0 && r0 < A.c && S.max_id > 0;  // a contextual row walks every non-target key
  const int hi = ctx ? (r1 > S.nts ? r1 : S.nts) : r1;
  int lo = 0;
  if (A.L > 0 && !ctx) {  // the first key whose id reaches id(r0) - L
    const int target = hdb_id(A, S, r0) - A.L;
    lo = target <= 0 ? 0 : target + (A.c > 0 ? A.c - 1 : 0);
  }
  const int hit = (hi + HDB_TILE - 1) / HDB_TILE;
  W.a0 = lo / HDB_TILE;
  int a1 = hit;
  if (S.has_t) {  // tiles of targets alone in front of the rows' own: nothing valid
    a1 = (S.nts + HDB_TILE - 1) / HDB_TILE;
    a1 = a1 < W.a0 ? W.a0 : (a1 > hit ? hit : a1);
  }
  int b0 = r0 / HDB_TILE;
  b0 = b0 < a1 ? a1 : (b0 > hit ? hit : b0);
  W.a1 = a1, W.b0 = b0, W.b1 = hit;
  return W;
}

// key row j of head h, clamped below n (>= 1): a cached row or, behind them, a delta row
__device__ __forceinline__ const uint16_t* hdb_row(const HdbOperand& c, const HdbOperand& d, const HdbSample& S, int b, int h, int delta, int j) {
  j = j < S.n ? j : S.n - 1;
  return j < S.n1 ? c.p + (S.start + j) * c.rs + h * c.hs : d.p + ((int64_t)b * delta + (j - S.n1)) * d.rs + h * d.hs;
}

// A wave's V tile on its way into the wave's transposed stash: lane (li, g) holds, of the rows k0 + 2 li and k0 + 2 li + 1, the 16
// bytes at columns 8 (g + 4 p), p < D / 32 -- sixteen consecutive lanes hold the sixteen row pairs of one 8-column chunk, so their
// transposed dword stores are consecutive.  Rows at or behind n are zeros; the loads are unconditional, from a clamped row and column.
template <int D>
struct HdbStash {
  static constexpr int NP = D / 32;
  tzr_u32x4 pre[NP][2];

  __device__ __forceinline__ void fetch(const HdbArgs& A, const HdbSample& S, int b, int h, int k0, int li, int g) {
    const int r = k0 + 2 * li;
    const uint16_t* p0 = hdb_row(A.v, A.vd, S, b, h, A.delta, r);
    const uint16_t* p1 = hdb_row(A.v, A.vd, S, b, h, A.delta, r + 1);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int col = 8 * (g + 4 * p);
      if (32 * p < A.Dv) {
        const tzr_u32x4 x = tzr_ldg16(p0 + (col < A.Dv ? col : 0)), y = tzr_ldg16(p1 + (col < A.Dv ? col : 0));
        pre[p][0] = r < S.n ? x : tzr_zero16();
        pre[p][1] = r + 1 < S.n ? y : tzr_zero16();
      }
    }
  }
  __device__ __forceinline__ void store(uint16_t* Vt, int Dv, int li, int g) const {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int col = 8 * (g + 4 * p);
      if (col < Dv) {
        const tzr_u32x4 x = pre[p][0], y = pre[p][1];
        uint32_t* t = reinterpret_cast<uint32_t*>(Vt + col * HDB_TS + 2 * li);
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // columns 2 j and 2 j + 1 of the chunk: (row 2 li | row 2 li + 1)
          t[(2 * j) * (HDB_TS / 2)] = (x[j] & 0xffffu) | (y[j] << 16);
          t[(2 * j + 1) * (HDB_TS / 2)] = (x[j] >> 16) | (y[j] & 0xffff0000u);
        }
      }
    }
  }
};

// the A fragments of the scores: lane (li, g) of sub-tile t holds the 16 bytes at columns 32 ch + 8 g of key k0 + 8 (li >> 2) + 4 t +
// (li & 3), straight from global memory; zeros at or behind n and behind the width
template <int D>
__device__ __forceinline__ void hdb_keys(tzr_u32x4 (*kf)[D / 32], const HdbArgs& A, const HdbSample& S, int b, int h, int k0, int li, int g) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int jk = k0 + 8 * (li >> 2) + 4 * t + (li & 3);
    const uint16_t* kp = hdb_row(A.k, A.kd, S, b, h, A.delta, jk);
#pragma unroll
    for (int ch = 0; ch < D / 32; ++ch) {
      const int a = 32 * ch + 8 * g;
      if (32 * ch < A.Da) {
        const tzr_u32x4 x = tzr_ldg16(kp + (a < A.Da ? a : 0));
        kf[t][ch] = a < A.Da && jk < S.n ? x : tzr_zero16();
      }
    }
  }
}

// one tile of 32 keys from k0 on: o += (masked silu(alpha K Q^T) / scale)^T V, K in kf, V in the wave's stash Vt
template <int D>
__device__ __forceinline__ void hdb_tile(const HdbArgs& A, const HdbSample& S, int k0, const tzr_u32x4 (*kf)[D / 32], const tzr_u32x4* qf, int i, int ii,
                                         const uint16_t* Vt, tzr_f32x4* o, int li, int g) {
  tzr_f32x4 st[2], p[2];
  st[0] = tzr_acc_zero(), st[1] = tzr_acc_zero();
#pragma unroll
  for (int ch = 0; ch < D / 32; ++ch) {
    if (32 * ch < A.Da) {
      st[0] = tzr_mfma_bf16(kf[0][ch], qf[ch], st[0]);
      st[1] = tzr_mfma_bf16(kf[1][ch], qf[ch], st[1]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {  // register e & 3 of sub-tile e >> 2: (key 8 g + e, query li)
    const int j = k0 + 8 * g + e;
    const float x = A.alpha * st[e >> 2][e & 3];
    p[e >> 2][e & 3] = hdb_valid(A, S, i, ii, j, hdb_id(A, S, j)) ? x * tzr_sigmoid(x) * A.inv_scale : 0.f;
  }
  const tzr_u32x4 pk = tzr_pack_bf16x8(p[0], p[1]);  // the one rounding of P
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct) {
    if (16 * ct < A.Dv) {
      const int col = 16 * ct + li;
      const tzr_u32x4 t = tzr_ld16(Vt + (col < A.Dv ? col : 0) * HDB_TS + 8 * g);
      o[ct] = tzr_mfma_bf16(pk, col < A.Dv ? t : tzr_zero16(), o[ct]);
    }
  }
}

__device__ __forceinline__ tzr_f32x4 hdb_f32x4(float4 v) { return tzr_f32x4{v.x, v.y, v.z, v.w}; }

template <int D>
__global__ __launch_bounds__(HDB_THREADS) void tzr_hstu_delta_bf16_kernel(HdbArgs A) {
  __shared__ uint16_t Vt[4][D * HDB_TS] __attribute__((aligned(16)));
  __shared__ float Sm[4][HDB_ROWS][D + 4];
  const unsigned x = blockIdx.x, bh = (unsigned)A.B * (unsigned)A.H, u = x / bh, bhi = x - u * bh;
  const int b = (int)(bhi / (unsigned)A.H), h = (int)(bhi - (unsigned)b * (unsigned)A.H);
  const int ch = (int)(u / (unsigned)A.ntile), r0 = HDB_ROWS * (int)(u - (unsigned)ch * (unsigned)A.ntile);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, li = lane & 15;
  const int rows = A.delta - r0 < HDB_ROWS ? A.delta - r0 : HDB_ROWS, v8 = A.Dv >> 3;
  const int64_t row0 = (int64_t)b * A.delta + r0;
  uint16_t* dst = A.out.p + row0 * A.out.rs + h * A.out.hs;
  const HdbSample S = hdb_sample(A, b);
  if (!S.ok) {  // zeros: here with one chunk, from the finishing launch otherwise
    if (A.nchunk == 1)
      for (int e = tid; e < rows * v8; e += HDB_THREADS) tzr_stg16(dst + (e / v8) * A.out.rs + 8 * (e % v8), tzr_zero16());
    return;
  }
  if (ch * HDB_CHUNK >= S.n) return;  // (never chunk 0: n >= delta >= 1)
  const int rq = r0 + li, i = S.n - A.delta + rq, ii = hdb_id(A, S, i);  // (rq >= delta: i >= n, nothing valid)
  const uint16_t* qp = rq < A.delta ? A.q.p + (row0 + li) * A.q.rs + h * A.q.hs : nullptr;
  tzr_u32x4 qf[D / 32];
#pragma unroll
  for (int c = 0; c < D / 32; ++c) {
    const int a = 32 * c + 8 * g;
    qf[c] = qp && a < A.Da ? tzr_ldg16(qp + a) : tzr_zero16();
  }
  tzr_f32x4 o[D / 16];
  tzr_acc_zero(o, D / 16);
  const int i0 = S.n - A.delta + r0;
  const HdbWalk W = hdb_row_walk(A, S, i0, i0 + rows);
  // wave w: the tiles t0, t0 + 4, .. of the chunk.  One trip count for the four waves (the barriers); a wave whose tile is not in
  // the walk does nothing between them.  The V tile travels a tile ahead: global -> registers under the multiplies, -> stash behind them.
  const int t0 = ch * HDB_CT + wv;
  HdbStash<D> vs;
  tzr_u32x4 kf[2][D / 32];
  if (W.has(t0)) vs.fetch(A, S, b, h, t0 * HDB_TILE, li, g);
  for (int s = 0; s < HDB_CT / 4; ++s) {
    const int t = t0 + 4 * s;
    const bool act = W.has(t), next = s + 1 < HDB_CT / 4 && W.has(t + 4);  // (uniform in the wave)
    if (act) {
      vs.store(Vt[wv], A.Dv, li, g);
      hdb_keys<D>(kf, A, S, b, h, t * HDB_TILE, li, g);
    }
    if (next) vs.fetch(A, S, b, h, (t + 4) * HDB_TILE, li, g);
    __syncthreads();
    if (act) hdb_tile<D>(A, S, t * HDB_TILE, kf, qf, i, ii, Vt[wv], o, li, g);
    __syncthreads();
  }
  // register r of accumulator ct is (query 4 g + r, column 16 ct + li)
#pragma unroll
  for (int ct = 0; ct < D / 16; ++ct)
    if (16 * ct < A.Dv)
#pragma unroll
      for (int r = 0; r < 4; ++r) Sm[wv][4 * g + r][16 * ct + li] = o[ct][r];
  __syncthreads();
  float* wdst = A.nchunk == 1 ? nullptr : A.ws + (((int64_t)ch * A.B * A.delta + row0) * A.H + h) * A.Dv;
  for (int e = tid; e < rows * v8; e += HDB_THREADS) {  // the four partials in wave order, eight columns a thread
    const int r = e / v8, c = 8 * (e - r * v8);
    const float4 lo = tzr_add4(tzr_add4(tzr_add4(tzr_ld4(&Sm[0][r][c]), tzr_ld4(&Sm[1][r][c])), tzr_ld4(&Sm[2][r][c])), tzr_ld4(&Sm[3][r][c]));
    const float4 hi = tzr_add4(tzr_add4(tzr_add4(tzr_ld4(&Sm[0][r][c + 4]), tzr_ld4(&Sm[1][r][c + 4])), tzr_ld4(&Sm[2][r][c + 4])), tzr_ld4(&Sm[3][r][c + 4]));
    if (wdst) {
      tzr_stg4(wdst + (int64_t)r * A.H * A.Dv + c, lo);
      tzr_stg4(wdst + (int64_t)r * A.H * A.Dv + c + 4, hi);
    } else {
      tzr_stg16(dst + r * A.out.rs + c, tzr_pack_bf16x8(hdb_f32x4(lo), hdb_f32x4(hi)));  // the one rounding of out
    }
  }
}

// out = the chunks' fp32 partials in order 0, 1, .. -- only the chunks the sample has --, rounded once; zeros for a refused sample.
// One thread eight columns.
__global__ __launch_bounds__(HDB_THREADS) void tzr_hstu_delta_bf16_finish_kernel(HdbArgs A) {
  const int v8 = A.Dv >> 3;
  const int64_t x = (int64_t)blockIdx.x * HDB_THREADS + threadIdx.x, rows = (int64_t)A.B * A.delta;
  if (x >= rows * A.H * v8) return;
  const int c = 8 * (int)(x % v8);
  const int64_t rh = x / v8, row = rh / A.H;
  const int h = (int)(rh - row * A.H);
  int64_t start, len;
  const int n = hdb_rows(A, (int)(row / A.delta), &start, &len);
  float4 lo = tzr_zero4(), hi = tzr_zero4();
  if (n >= 0) {
    const int nch = (n + HDB_CHUNK - 1) / HDB_CHUNK;  // (>= 1, and <= nchunk: n <= max_seq_len)
    const int64_t slot = rows * A.H * A.Dv;
    const float* p = A.ws + (row * A.H + h) * A.Dv + c;
    lo = tzr_ldg4(p), hi = tzr_ldg4(p + 4);
    for (int k = 1; k < nch; ++k) lo = tzr_add4(lo, tzr_ldg4(p + k * slot)), hi = tzr_add4(hi, tzr_ldg4(p + k * slot + 4));
  }
  tzr_stg16(A.out.p + row * A.out.rs + h * A.out.hs + c, tzr_pack_bf16x8(hdb_f32x4(lo), hdb_f32x4(hi)));
}

// ---- host ------------------------------------------------------------------------------------------------------------

// an [N, H, D] bf16 operand by row and head stride, the rule of hstu_attention_bf16.hip
static int hdb_operand(uint64_t ptr, int64_t rs, int64_t hs, int H, int D, HdbOperand* o) {
  if (!ptr || (ptr & 15)) return TZR_ERR_INVALID;
  if ((rs & 7) || (hs & 7) || hs < D || rs < (int64_t)(H - 1) * hs + D) return TZR_ERR_UNSUPPORTED;
  o->p = reinterpret_cast<uint16_t*>(ptr), o->rs = rs, o->hs = hs;
  return TZR_OK;
}

// sizes, then limits (those of hstu_delta.hip with widths in steps of 8); `A` gets the shape
static int hdb_shape(const TzrHstuDelta* m, HdbArgs* A) {
  if (m->B < 0 || m->Nc < 0 || m->max_attn_len < 0 || m->contextual_seq_len < 0) return TZR_ERR_INVALID;
  if (!tzr_dim8_ok(m->Da, TZR_HSTU_MAX_DIM) || !tzr_dim8_ok(m->Dv, TZR_HSTU_MAX_DIM) || m->H < 1 || m->delta < 1 || m->max_seq_len < 1 ||
      m->max_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->max_attn_len > TZR_HSTU_MAX_SEQ_LEN || m->contextual_seq_len > TZR_HSTU_MAX_SEQ_LEN || m->Nc >= (1ll << 31))
    return TZR_ERR_UNSUPPORTED;
  const int64_t nchunk = ((int64_t)m->max_seq_len + HDB_CHUNK - 1) / HDB_CHUNK, ntile = ((int64_t)m->delta + HDB_ROWS - 1) / HDB_ROWS;
  if (m->B > 0 && (m->B >= (1ll << 31) / m->delta || m->B * m->delta >= (1ll << 31) / m->H || nchunk * ntile >= (1ll << 31) / (m->B * m->H))) return TZR_ERR_UNSUPPORTED;
  A->Nc = m->Nc, A->B = (int)m->B, A->H = m->H, A->Da = m->Da, A->Dv = m->Dv, A->delta = m->delta, A->max_len = m->max_seq_len;
  A->L = m->max_attn_len, A->c = m->contextual_seq_len, A->ntile = (int)ntile, A->nchunk = (int)nchunk;
  A->alpha = m->alpha;
  A->inv_scale = 1.0f / (float)(m->scaling_seqlen > 0 ? m->scaling_seqlen : m->max_seq_len);
  return TZR_OK;
}

extern "C" int tzr_hstu_delta_bf16_fwd(const TzrHstuDelta* h_dl, void* stream) {
  if (!h_dl) return TZR_ERR_INVALID;
  HdbArgs A = {};
  TZR_TRY(hdb_shape(h_dl, &A));
  if (h_dl->B == 0) return TZR_OK;
  TZR_TRY(hdb_operand(h_dl->delta_q, h_dl->delta_q_stride, h_dl->delta_q_head_stride, A.H, A.Da, &A.q));
  if (A.Nc > 0) {
    TZR_TRY(hdb_operand(h_dl->k, h_dl->k_stride, h_dl->k_head_stride, A.H, A.Da, &A.k));
    TZR_TRY(hdb_operand(h_dl->v, h_dl->v_stride, h_dl->v_head_stride, A.H, A.Dv, &A.v));
  }
  if (!h_dl->k_delta != !h_dl->v_delta) return TZR_ERR_INVALID;
  if (h_dl->k_delta) {
    TZR_TRY(hdb_operand(h_dl->k_delta, h_dl->k_delta_stride, h_dl->k_delta_head_stride, A.H, A.Da, &A.kd));
    TZR_TRY(hdb_operand(h_dl->v_delta, h_dl->v_delta_stride, h_dl->v_delta_head_stride, A.H, A.Dv, &A.vd));
  }
  if (!h_dl->offsets || (h_dl->offsets & 7) || (h_dl->num_targets & 7)) return TZR_ERR_INVALID;
  TZR_TRY(hdb_operand(h_dl->out, h_dl->out_stride, h_dl->out_head_stride, A.H, A.Dv, &A.out));
  // the fp32 partials of the chunks: the workspace of the fp32 entry, [chunks][B delta][H][Dv] floats
  if (A.nchunk > 1 && (!h_dl->ws || (h_dl->ws & 255) || h_dl->ws_bytes < tzr_hstu_delta_workspace(h_dl))) return TZR_ERR_WORKSPACE;
  A.off = reinterpret_cast<const int64_t*>(h_dl->offsets);
  A.nt = reinterpret_cast<const int64_t*>(h_dl->num_targets);
  A.ws = reinterpret_cast<float*>(h_dl->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((int64_t)A.nchunk * A.ntile * A.B * A.H));
  if ((A.Da > A.Dv ? A.Da : A.Dv) <= 64) hipLaunchKernelGGL((tzr_hstu_delta_bf16_kernel<64>), grid, dim3(HDB_THREADS), 0, s, A);
  else hipLaunchKernelGGL((tzr_hstu_delta_bf16_kernel<128>), grid, dim3(HDB_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  if (A.nchunk > 1) {
    const int64_t n8 = (int64_t)A.B * A.delta * A.H * (A.Dv >> 3);
    hipLaunchKernelGGL(tzr_hstu_delta_bf16_finish_kernel, dim3((unsigned)((n8 + HDB_THREADS - 1) / HDB_THREADS)), dim3(HDB_THREADS), 0, s, A);
    TZR_CHECK_LAUNCH();
  }
  return TZR_OK;
}
