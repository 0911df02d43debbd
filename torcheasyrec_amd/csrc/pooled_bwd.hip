// K6: backward index plan for gfx950.
//
// Replaces fbgemm transpose_embedding_input (linearize + cub radix sort + run-length), reached from
// autograd of self.ebc(kjt) (/root/reference/tzrec/modules/embedding.py:930) with the optimizer
// fused by apply_optimizer_in_backward (/root/reference/tzrec/main.py:774-781).
//
// The apply (K7, pooled_bwd_apply.hip) wants, per table, the lookups ordered by (row, original
// lookup position): every summation order is then a function of the ids alone => bit-reproducible
// updates, no float atomics anywhere.  Round 1 got there with a 3-pass LSD radix sort = 10 dependent
// launches of latency-bound kernels (95 us at B = 65536 for ~20 us of traffic).  Now:
//
//   hist     one launch: every workgroup derives the table-major geometry itself (no prep launch),
//            counts its chunk's lookups per BUCKET (<= 512 per table, ~rows/512 consecutive row ids
//            each, evenly filled by uniform ids -- bwd_bucket_params);
//   scan     per table: bucket starts, the unit grid of the apply, the list of heavy buckets;
//   scatter  ONE stable partition pass into buckets (lookups regrouped table-major on the way);
//   sort     ONE launch finishes the order, ks[1] -> ks[0]: a workgroup per unit of the apply sorts
//            the unit's light buckets in LDS (< 1280 lookups, 2-3 counting passes on the row-id bits
//            left inside the unit); buckets with more than BWD_TH lookups (hot rows: Zipf heads,
//            default ids) are sorted by extra workgroups of the same launch, tile-parallel when the
//            bucket holds <= 512 row ids (one counting pass), else tile by tile by one workgroup.
//
// 4 launches instead of 10, ~1/2 of the ks traffic; the apply kernels are what they were.
#include <tzr_gfx950.h>

#include "pooled_bwd_sort.h"

#ifdef IT_PROF  // scripts/build_prof_lib.sh: wall-clock (100 MHz) start / end of every workgroup of the plan's four launches
#define PLAN_PROF_WGS 4096
__device__ uint64_t g_plan_prof[4 * PLAN_PROF_WGS * 2];
struct PlanProf {
  int k;
  __device__ PlanProf(int k_) : k(k_) {
    if (threadIdx.x == 0 && blockIdx.x < PLAN_PROF_WGS) g_plan_prof[((size_t)k * PLAN_PROF_WGS + blockIdx.x) * 2] = wall_clock64();
  }
  __device__ ~PlanProf() {
    if (threadIdx.x == 0 && blockIdx.x < PLAN_PROF_WGS) g_plan_prof[((size_t)k * PLAN_PROF_WGS + blockIdx.x) * 2 + 1] = wall_clock64();
  }
};
#define PLAN_PROF(k) PlanProf plan_prof_(k)
extern "C" int tzr_plan_prof_dump(uint64_t* h_out) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_plan_prof), sizeof(uint64_t) * 4 * PLAN_PROF_WGS * 2) == hipSuccess ? 0 : -1;
}
#else
#define PLAN_PROF(k)
#endif

extern "C" size_t tzr_pooled_bwd_workspace(int64_t n_values, int64_t n_positions, int n_feats,
                                           int n_tables, int64_t B, int max_dim) {
  (void)B;
  if (n_values < 0 || n_positions < 0 || n_feats <= 0 || n_tables <= 0 || max_dim <= 0) return 0;
  return bwd_layout(nullptr, nullptr, n_values, n_positions, n_feats, n_tables, max_dim) + 256;
}

// Inspection of a plan (tests, debugging): byte offsets into `ws` of
//   out[0] ks[0]  out[1] ks[1]  (uint2 {row, lookup position} per table-major position)
//   out[2] feat_start (uint32[F+1])  out[3] ucut (uint32[max_chunks+1])  out[4] cdesc (64 B each)
//   out[5] max_chunks  out[6] hcount (uint32)  out[7] hlist (32 B each)
extern "C" int tzr_pooled_bwd_plan_view(int64_t n_values, int64_t n_positions, int n_feats,
                                        int n_tables, int max_dim, int64_t* out8) {
  if (!out8 || n_values < 0 || n_positions < 0 || n_feats <= 0 || n_tables <= 0 || max_dim <= 0)
    return TZR_ERR_INVALID;
  BwdPlan P;
  bwd_layout(&P, nullptr, n_values, n_positions, n_feats, n_tables, max_dim);
  const char* base = nullptr;
  out8[0] = reinterpret_cast<const char*>(P.ks[0]) - base;
  out8[1] = reinterpret_cast<const char*>(P.ks[1]) - base;
  out8[2] = reinterpret_cast<const char*>(P.feat_start) - base;
  out8[3] = reinterpret_cast<const char*>(P.ucut) - base;
  out8[4] = reinterpret_cast<const char*>(P.cdesc) - base;
  out8[5] = P.max_chunks;
  out8[6] = reinterpret_cast<const char*>(P.hcount) - base;
  out8[7] = reinterpret_cast<const char*>(P.hlist) - base;
  return TZR_OK;
}

// ------------------------------------------------------------------------------------------
// geometry
// ------------------------------------------------------------------------------------------

// Fallback for more than BWD_GEO lookups or tables: one workgroup writes the geometry to the
// workspace (serial prefixes), the hist workgroups read it from there.
__global__ __launch_bounds__(BWD_THREADS) void tzr_bwd_prep_kernel(
    const TzrTable* __restrict__ tables, int T, BwdSrcArgs A, int F, BwdPlan P) {
  if (P.nslices > 1)
    for (int o = threadIdx.x; o < T; o += BWD_THREADS) P.scnt[o] = 0;  // arrivals of the scan launch's slices
  for (int f = threadIdx.x; f < F; f += BWD_THREADS) {
    const TzrFeature ft = A.feats[f];
    const int64_t key = ft.key;
    const int64_t n =
        ft.table < 0 ? 0 : (A.uniform ? A.B : A.offsets[(key + 1) * A.B] - A.offsets[key * A.B]);
    P.feat_start[ft.order] = (uint32_t)n;
    P.feat_key[ft.order] = ft.key;
    P.feat_by_order[ft.order] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int o = 0; o < F; ++o) {
      const uint32_t n = P.feat_start[o];
      P.feat_start[o] = run;
      run += n;
    }
    P.feat_start[F] = run;
    P.hcount[0] = 0;
    P.hcount[1] = (uint32_t)P.fuse;
  }
  for (int t = threadIdx.x; t < T; t += BWD_THREADS) P.tab_stitch[t] = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += BWD_THREADS) {
    const TzrTable tb = tables[t];
    const uint32_t s = tb.n_feats > 0 ? P.feat_start[tb.first_order] : 0u;
    const uint32_t e = tb.n_feats > 0 ? P.feat_start[tb.first_order + tb.n_feats] : 0u;
    P.tab_chunk[t] = (int32_t)((e - s + (uint32_t)P.ch - 1) / (uint32_t)P.ch);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t run = 0;
    for (int t = 0; t < T; ++t) {
      const int32_t n = P.tab_chunk[t];
      P.tab_chunk[t] = run;
      run += n;
    }
    P.tab_chunk[T] = run;
  }
}

// ------------------------------------------------------------------------------------------
// hist: chunk descriptors + bucket counts of every chunk
// ------------------------------------------------------------------------------------------
template <bool FUSED>
__global__ __launch_bounds__(BWD_THREADS) void tzr_bwd_hist_kernel(
    const TzrTable* __restrict__ tables, int T, int F, BwdSrcArgs A, BwdPlan P) {
  PLAN_PROF(0);
  __shared__ unsigned h[BWD_NB];
  __shared__ BwdGeoLds GL;
  BwdGeo G;
  if (FUSED) {
    bwd_geometry(tables, T, A, F, (uint32_t)P.ch, GL);
    G.fstart = GL.fstart;
    G.fkey = GL.fkey;
    G.tchunk = reinterpret_cast<const int32_t*>(GL.tchunk);
    if (blockIdx.x == 0) {  // the later kernels of the plan and the apply read it from the workspace
      if (P.nslices > 1)
        for (int o = threadIdx.x; o < T; o += BWD_THREADS) P.scnt[o] = 0;  // arrivals of the scan launch's slices
      for (int o = threadIdx.x; o <= F; o += BWD_THREADS) P.feat_start[o] = GL.fstart[o];
      for (int o = threadIdx.x; o < F; o += BWD_THREADS) P.feat_key[o] = GL.fkey[o];
      for (int f = threadIdx.x; f < F; f += BWD_THREADS) P.feat_by_order[A.feats[f].order] = f;
      for (int t = threadIdx.x; t <= T; t += BWD_THREADS) P.tab_chunk[t] = (int32_t)GL.tchunk[t];
      for (int t = threadIdx.x; t < T; t += BWD_THREADS) P.tab_stitch[t] = 0;
      if (threadIdx.x == 0) {
        P.hcount[0] = 0;
        P.hcount[1] = (uint32_t)P.fuse;  // the apply sorts the units without heavy lookups itself (read by the sort launch and the apply)
      }
    }
  } else {
    G.fstart = P.feat_start;
    G.fkey = P.feat_key;
    G.tchunk = P.tab_chunk;
  }
  const int c = blockIdx.x;
  BwdChunkDesc cd;
  cd.t = -1;
  cd.nb = cd.exact = cd.last_chunk = 0;
  cd.s = cd.e = cd.ts = cd.te = 0;
  cd.mult = 0;
  TzrTable tb;
  if (c < G.tchunk[T]) {
    int lo = 0, hi = T;  // last t with tchunk[t] <= c (the non-empty table holding it)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (G.tchunk[mid] <= c) lo = mid; else hi = mid;
    }
    tb = tables[lo];
    cd.t = lo;
    bwd_bucket_params(tb.rows, &cd.nb, &cd.mult);
    cd.exact = tb.rows <= BWD_NB;
    cd.last_chunk = G.tchunk[lo + 1];
    cd.ts = tb.n_feats > 0 ? (int64_t)G.fstart[tb.first_order] : 0;
    cd.te = tb.n_feats > 0 ? (int64_t)G.fstart[tb.first_order + tb.n_feats] : cd.ts;
    cd.s = cd.ts + (int64_t)(c - G.tchunk[lo]) * P.ch;
    cd.e = min(cd.te, cd.s + (int64_t)P.ch);
  }
  if (threadIdx.x == 0) P.cdesc[c] = cd;
  if (cd.t < 0) return;
  for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) h[i] = 0;
  // all of the chunk's keys are loaded before any is counted: independent loads in flight, one
  // memory latency per workgroup instead of one per element
  constexpr int kRounds = BWD_CH / BWD_THREADS;
  uint32_t kreg[kRounds];
  if (tb.n_feats == 1) {  // (workgroup-uniform) one key reads the table: unconditional loads, see bwd_elem_one
    const BwdOneSeg sg = bwd_one_seg(G, tb, A);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      uint32_t sv;
      bwd_elem_one(sg, tb, A, cd.s + (int64_t)r * BWD_THREADS + threadIdx.x, cd.e, &kreg[r], &sv);
    }
  } else {
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int64_t p = cd.s + (int64_t)r * BWD_THREADS + threadIdx.x;
      uint32_t sv;
      int64_t kk;
      kreg[r] = 0u;
      if (p < cd.e) bwd_elem0(G, tb, A, p, &kreg[r], &sv, &kk);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t p = cd.s + (int64_t)r * BWD_THREADS + threadIdx.x;
    if (p < cd.e) atomicAdd(&h[bwd_bucket(kreg[r], cd.mult)], 1u);
  }
  __syncthreads();
  uint32_t* out = P.hist + (size_t)blockIdx.x * BWD_NB;
  for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) out[i] = h[i];
}

// ------------------------------------------------------------------------------------------
// scan: bucket starts, the unit grid, heavy buckets
// ------------------------------------------------------------------------------------------
// One workgroup per table, one thread per bucket: exclusive scan over the table's chunks (in
// place) and over buckets -> binbase.  Chunk columns are read in batches of independent loads.
//
// Units of the apply.  Cut points = bucket boundaries + the BWD_CH-block boundaries that fall
// INSIDE a heavy bucket; unit j of a table starts at the first cut point at or after block j
// (ts + j * BWD_CH).  So a unit is a whole number of light buckets (which the reduce kernel sorts
// in LDS) and/or block-sized slices of heavy buckets (sorted by the heavy kernel), it holds fewer
// than BWD_CH + BWD_TH lookups, and a run of one row can only cross a unit boundary inside a heavy
// bucket.
#define BWD_SCAN_BATCH 64
__global__ __launch_bounds__(BWD_NB) void tzr_bwd_scan_kernel(const TzrTable* __restrict__ tables,
                                                              int T, int one_wg_heavy, BwdPlan P) {
  PLAN_PROF(1);
  __shared__ unsigned tot[BWD_NB];
  __shared__ int s_last, s_heavy;
  const int nsl = P.nslices;
  const int t = nsl > 1 ? (int)blockIdx.x / nsl : (int)blockIdx.x;
  const int sl = nsl > 1 ? (int)blockIdx.x % nsl : 0;
  const int c0 = P.tab_chunk[t];
  const int C = P.tab_chunk[t + 1] - c0;
  if (C <= 0 && nsl == 1) return;
  const TzrTable tb = tables[t];
  const uint32_t ts = P.feat_start[tb.first_order];
  const uint32_t te = P.feat_start[tb.first_order + tb.n_feats];
  const bool exact = tb.rows <= BWD_NB;
  const int bin = threadIdx.x;
  // this workgroup's slice of the table's chunks (all of them when the launch has one workgroup per table)
  const int SL = (C + nsl - 1) / nsl;
  const int cs = min(C, sl * SL), ce = min(C, cs + SL);
  unsigned run = 0;
  for (int cb = cs; cb < ce; cb += BWD_SCAN_BATCH) {
    unsigned v[BWD_SCAN_BATCH];
#pragma unroll
    for (int j = 0; j < BWD_SCAN_BATCH; ++j)
      v[j] = (cb + j < ce) ? P.hist[(size_t)(c0 + cb + j) * BWD_NB + bin] : 0u;
#pragma unroll
    for (int j = 0; j < BWD_SCAN_BATCH; ++j) {
      if (cb + j < ce) P.hist[(size_t)(c0 + cb + j) * BWD_NB + bin] = run;
      run += v[j];
    }
  }
  if (nsl > 1) {
    // the slice's bucket counts go out write-through; the workgroup that completes the table's arrivals turns them
    // into slice bases (the scatter launch adds them to the chunk-exclusive counts) and finishes the table
    uint32_t* st = P.stot + ((size_t)t * nsl) * BWD_NB;
    tzr_publish_u32(st + (size_t)sl * BWD_NB + bin, run);
    tzr_drain_stores();
    __syncthreads();
    if (threadIdx.x == 0) s_last = tzr_arrive(P.scnt + t) == (uint32_t)(nsl - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    run = 0;
    for (int s2 = 0; s2 < nsl; ++s2) {
      const uint32_t v = tzr_consume_u32(st + (size_t)s2 * BWD_NB + bin);
      st[(size_t)s2 * BWD_NB + bin] = run;
      run += v;
    }
    if (C <= 0) return;
  }
  // A table WITH heavy buckets keeps the sort launch for all of its units (the launch is long anyway -- its heavy buckets -- and
  // the light units sort under them for free: fusing them into the apply measured +6 us on Zipf ids, profiles/r05ao); a table
  // without any leaves every unit to the apply.
  if (bin == 0) s_heavy = 0;  // (a variable of its own: other waves may still be reading s_last above)
  __syncthreads();
  if (!exact && run > BWD_TH) s_heavy = 1;
  __syncthreads();
  const int any_heavy = s_heavy;
  for (int i = bin; i < C; i += BWD_NB) P.umix[c0 + i] = any_heavy ? 1u : 0u;
  tot[bin] = run;
  __syncthreads();
  // Hillis-Steele inclusive scan over the buckets
  for (int d = 1; d < BWD_NB; d <<= 1) {
    const unsigned add = bin >= d ? tot[bin - d] : 0u;
    __syncthreads();
    tot[bin] += add;
    __syncthreads();
  }
  const uint32_t end = ts + tot[bin];
  const uint32_t start = end - run;
  uint32_t* bb = P.binbase + (size_t)t * (BWD_NB + 1);
  bb[bin] = start;
  if (bin == BWD_NB - 1) bb[BWD_NB] = te;
  {  // bitmap of the heavy buckets (read by the unit sort): one ballot per wave = two words
    const unsigned long long hb = __ballot(!exact && run > BWD_TH);
    if ((threadIdx.x & (TZR_WAVE - 1)) == 0) {
      uint32_t* hw = P.hbits + (size_t)t * (BWD_NB / 32) + (threadIdx.x / TZR_WAVE) * 2;
      hw[0] = (uint32_t)hb;
      hw[1] = (uint32_t)(hb >> 32);
      if (hb != 0 || (exact && threadIdx.x == 0)) atomicOr(&P.tab_stitch[t], 1u);
    }
  }
  // Stitch groups of the apply: a run of one row can only cross a unit boundary inside a sorted
  // bucket; the units overlapping such a bucket meet at its counter (reduce kernel)
  {
    uint32_t expect = 0;
    if (run > 0 && (exact || run > BWD_TH)) {
      const uint32_t ch = (uint32_t)P.ch;
      const uint32_t units = (end - 1 - ts) / ch - (start - ts) / ch + 1;
      expect = units > 1 ? units : 0u;
    }
    P.sexp[(size_t)t * BWD_NB + bin] = expect;
    P.sarr[(size_t)t * BWD_NB + bin] = 0;
  }
  if (run == 0) return;
  // an exact table's buckets are single rows: in final order after the partition pass whatever
  // their size, cut at blocks like heavy buckets but never listed for the heavy kernel
  const bool heavy = !exact && run > BWD_TH;
  const bool sorted = exact || heavy;
  // blocks whose first position lies in this bucket
  const uint32_t ch = (uint32_t)P.ch;
  const uint32_t j0 = (start - ts + ch - 1) / ch;
  const uint32_t j1 = (end - 1 - ts) / ch;
  for (uint32_t j = j0; j <= j1; ++j) {
    const uint32_t bs = ts + j * ch;
    P.ucut[c0 + j] = (bs == start || sorted) ? bs : end;
    const uint32_t bnext = min(bs + ch, te);
    P.uflag[c0 + j] = (exact || (heavy && bnext <= end)) ? 1u : 0u;
  }
  if (heavy) {
    // row ids of the bucket: [klo, khi).  At most BWD_NB of them (tables up to BWD_NB^2 rows): one
    // counting pass on (row id - klo) sorts the bucket, tile by tile, one workgroup per tile.
    // Wider buckets (the hot rows of the big tables): several passes by one workgroup.
    int nb;
    uint64_t mult;
    bwd_bucket_params(tb.rows, &nb, &mult);
    const uint64_t klo = (((uint64_t)bin << 32) + mult - 1) / mult;
    uint64_t khi = (((uint64_t)(bin + 1) << 32) + mult - 1) / mult;
    if (khi > (uint64_t)tb.rows) khi = (uint64_t)tb.rows;
    // ... unless one row holds nearly all of such a bucket (the clipped Zipf tail, a default id:
    // tens of thousands of lookups): tile-parallel again, splitting around that row (hot items).
    const bool one_pass = khi - klo <= (uint64_t)BWD_NB;
    // (one_wg_heavy: every heavy bucket by ONE workgroup -- tzr_tune("bwd_one_wg_heavy"), see NOTES.md)
    const bool tiled = !one_wg_heavy && (one_pass || run > BWD_HT);
    const uint32_t tiles = tiled ? (run + BWD_HT - 1) / BWD_HT : 1u;
    const uint32_t slot = atomicAdd(P.hcount, tiles);
    for (uint32_t i = 0; i < tiles; ++i) {
      BwdHeavy hv;
      hv.t = t;
      hv.bin = (uint32_t)bin;
      hv.start = start;
      hv.end = end;
      hv.tile = tiled ? (int32_t)i : -1;
      hv.pad[0] = one_pass ? 0 : 1;  // 1: a wide bucket, tiled around its hot row
      hv.pad[1] = hv.pad[2] = 0;
      P.hlist[slot + i] = hv;
    }
  }
}

// ------------------------------------------------------------------------------------------
// scatter: the one global pass -- stable partition of every chunk into its table's buckets
// ------------------------------------------------------------------------------------------
// Element order inside a chunk is position order; bwd_rank_tile gives every element its index in
// the chunk's stable bucket-sorted order; the elements are laid out in THAT order in LDS and
// written back from there, so lanes that are neighbours in a wave store to neighbouring addresses
// whenever they share a bucket (one 8-byte {key, src} store per element; element-order stores are
// 2 x 4 bytes to unrelated lines, ~3x write amplification measured).
__global__ __launch_bounds__(BWD_THREADS) void tzr_bwd_scatter_kernel(
    const TzrTable* __restrict__ tables, int T, BwdSrcArgs A, BwdPlan P) {
  PLAN_PROF(2);
  __shared__ BwdRankLds<BWD_NB> L;
  __shared__ unsigned base0[BWD_NB];  // global position of the chunk's first element of each bucket
  __shared__ uint2 stage[BWD_CH];
  BwdChunkDesc cd;
  if (!bwd_chunk(P, blockIdx.x, &cd)) return;
  const int t = cd.t;
  const TzrTable tb = tables[t];
  const int n = (int)(cd.e - cd.s);
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const unsigned* hrow = P.hist + (size_t)blockIdx.x * BWD_NB;
  const unsigned* bb = P.binbase + (size_t)t * (BWD_NB + 1);
  if (P.nslices > 1) {  // the scan launch worked in slices of the table's chunks: + the counts of the slices before this one
    const int c0 = P.tab_chunk[t], C = P.tab_chunk[t + 1] - c0;
    const int SL = (C + P.nslices - 1) / P.nslices;
    const unsigned* sb = P.stot + ((size_t)t * P.nslices + ((int)blockIdx.x - c0) / SL) * BWD_NB;
    for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) base0[i] = bb[i] + hrow[i] + sb[i];
  } else {
    for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) base0[i] = bb[i] + hrow[i];
  }
  BwdGeo G;
  G.fstart = P.feat_start;
  G.fkey = P.feat_key;
  G.tchunk = P.tab_chunk;
  // all of the chunk's elements are loaded up front (independent coalesced loads): the ranking
  // then runs out of registers and pays one memory latency per workgroup
  constexpr int kRounds = BWD_CH / BWD_THREADS;
  const int pw = bwd_wave_span(n);
  const int rounds = pw / TZR_WAVE;
  uint32_t kreg[kRounds], sreg[kRounds], dig[kRounds], dest[kRounds];
  uint32_t vmask = 0;
  if (tb.n_feats == 1 && A.uniform) {  // (workgroup-uniform) one key, one id per bag: unconditional loads, see bwd_elem_one
    const BwdOneSeg sg = bwd_one_seg(G, tb, A);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int lp = wv * pw + r * TZR_WAVE + lane;
      // (every round loads, also the ones past this chunk's `rounds`: a condition on a value read from memory is a
      // divergent branch to the compiler, and a branch between two loads is a wait between them)
      bwd_elem_one(sg, tb, A, cd.s + lp, cd.e, &kreg[r], &sreg[r]);
      dig[r] = bwd_bucket(kreg[r], cd.mult);
      vmask |= (r < rounds && lp < n) ? 1u << r : 0u;
    }
  } else {
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int lp = wv * pw + r * TZR_WAVE + lane;
      kreg[r] = sreg[r] = dig[r] = 0u;
      if (r < rounds && lp < n) {
        vmask |= 1u << r;
        int64_t kk;
        bwd_elem0(G, tb, A, cd.s + lp, &kreg[r], &sreg[r], &kk);
        dig[r] = bwd_bucket(kreg[r], cd.mult);
        if (!A.uniform) {  // bag of every lookup, once (same value from every table a key feeds)
          const int64_t b = tzr_last_le(A.offsets + kk * A.B, A.B, (int64_t)sreg[r]);
          P.bag_of[sreg[r]] = (uint32_t)(kk * A.B + b);
        }
      }
    }
  }
  bwd_rank_tile<BWD_NB, kRounds>(dig, vmask, rounds, bwd_bits((uint32_t)cd.nb - 1u), L, dest);
#pragma unroll
  for (int r = 0; r < kRounds; ++r)
    if ((vmask >> r) & 1u) stage[dest[r]] = make_uint2(kreg[r], sreg[r]);
  __syncthreads();
  uint2* __restrict__ kout = P.ks[1];
  for (int i = threadIdx.x; i < n; i += BWD_THREADS) {
    const uint2 v = stage[i];
    const unsigned d = bwd_bucket(v.x, cd.mult);
    kout[base0[d] + ((unsigned)i - (unsigned)L.lstart[d])] = v;
  }
}

// ------------------------------------------------------------------------------------------
// sort: everything the partition pass left unordered, in ONE launch, ks[1] -> ks[0]
// ------------------------------------------------------------------------------------------
// Workgroups [0, max_chunks): one UNIT each -- the light buckets of the unit (whole buckets of
// consecutive row ids, in bucket order) get a stable LSD sort of (row id - smallest row id of the
// unit) over the bits that difference needs, in LDS; uniform ids at B = 65536 on a 40M-row table:
// ~9 buckets of ~128 lookups, 20 bits, 3 passes of 7 bits.  Lookups of heavy buckets inside the unit
// are skipped (their positions are written by the heavy workers below).
// Workgroups [max_chunks, ...): heavy-bucket workers, looping over the work items of the scan kernel.
//   one-pass item (bucket of <= BWD_NB row ids, tile i): counts the whole bucket per row id on its
//     own (no inter-workgroup traffic; the counts up to its tile are the cross-tile prefix), then
//     ranks and writes its tile: the tiles of a hot bucket are sorted in parallel;
//   serial item (a wide bucket: hot rows of the big tables): LSD passes tile by tile by one
//     workgroup; a single workgroup walks the tiles in order, so the running per-digit offsets ARE
//     the cross-tile prefix.

__device__ __forceinline__ void bwd_sort_unit(const TzrTable* __restrict__ tables, const BwdPlan& P,
                                              BwdSortLds& S, int c) {
  BwdChunkDesc cd;
  const uint32_t uf = P.uflag[c], um = P.umix[c], fz = P.hcount[1];  // (fetched with the descriptor)
  if (!bwd_chunk(P, c, &cd)) return;
  if (uf) return;
  if (fz && !um) return;  // fused plan: a unit without heavy lookups is sorted by the apply, in its LDS (bwd_stage_unit)
  const int64_t s = P.ucut[c];
  const int64_t e = c + 1 < cd.last_chunk ? (int64_t)P.ucut[c + 1] : cd.te;
  const int n = (int)(e - s);
  if (n <= 0 || n > BWD_UMAX) return;
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const uint2* __restrict__ src = P.ks[1] + s;
  uint2* __restrict__ dst = P.ks[0] + s;
  constexpr int kRounds = BWD_UMAX / BWD_THREADS;
  const int pw = bwd_wave_span(n);
  const int rounds = pw / TZR_WAVE;
  uint32_t kreg[kRounds], sreg[kRounds], bkt[kRounds], dest[kRounds];
  uint32_t vmask = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
  // the heavy-bucket bitmap of the table, one word per lane of the first 16: fetched together with
  // the lookups, consulted through a shuffle
  const uint32_t hword = lane < BWD_NB / 32 ? P.hbits[(size_t)cd.t * (BWD_NB / 32) + lane] : 0u;
  // heavy lookups ahead of each position = exclusive count of the heavy flags in position order
  // (wave-contiguous ownership: ballots inside a round, running count over rounds, waves by LDS)
  uint32_t hbefore[kRounds];
  uint32_t hrun = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int lp = wv * pw + r * TZR_WAVE + lane;
    kreg[r] = sreg[r] = bkt[r] = 0u;
    hbefore[r] = 0;
    const bool in = r < rounds && lp < n;
    {  // (the position is clamped, the load unconditional: `if (in) v = src[lp]` per round compiled to one dependent
       // round trip per round -- see bwd_elem_one)
      const uint2 v = src[lp < n ? lp : n - 1];
      kreg[r] = in ? v.x : 0u;
      sreg[r] = in ? v.y : 0u;
      bkt[r] = in ? bwd_bucket(v.x, cd.mult) : 0u;
    }
    if (r < rounds) {
      const uint32_t hw = (uint32_t)__shfl((int)hword, (int)(bkt[r] >> 5), TZR_WAVE);
      const bool heavy = in && ((hw >> (bkt[r] & 31)) & 1u);
      if (in && !heavy) {
        vmask |= 1u << r;
        kmin = min(kmin, kreg[r]);
        kmax = max(kmax, kreg[r]);
      }
      const unsigned long long hm = __ballot(heavy);
      hbefore[r] = hrun + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
      hrun += (uint32_t)__popcll(hm);
    }
  }
  for (int m = TZR_WAVE >> 1; m > 0; m >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, m, TZR_WAVE));
    kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, m, TZR_WAVE));
  }
  if (threadIdx.x == 0) S.gstart[0] = bkt[0];  // the unit is in bucket order: its first bucket
  if (lane == 0) {
    S.smm[wv] = kmin;
    S.smm[BWD_WAVES + wv] = kmax;
    S.wtot[wv] = hrun;
  }
  __syncthreads();
  const uint32_t b0 = S.gstart[0];
  uint32_t hwave = 0, htot = 0;
#pragma unroll
  for (int w = 0; w < BWD_WAVES; ++w) {
    kmin = min(kmin, S.smm[w]);
    kmax = max(kmax, S.smm[BWD_WAVES + w]);
    if (w < wv) hwave += S.wtot[w];
    htot += S.wtot[w];
  }
  // every light lookup of a bucket sees the same count: one entry per bucket of the unit
  if (htot) {
#pragma unroll
    for (int r = 0; r < kRounds; ++r)
      if ((vmask >> r) & 1u) S.hb[bkt[r] - b0] = (uint16_t)(hwave + hbefore[r]);
  }
  __syncthreads();  // smm is reused by the core
  if (kmin > kmax) return;  // nothing but heavy lookups (workgroup-uniform)
  bwd_sort_core<kRounds>(kreg, sreg, vmask, pw, rounds, kmin, max(1, bwd_bits(kmax - kmin)), htot == 0,
                         S, dest);
  // final position = unit start + rank among the unit's light lookups + heavy lookups ahead
#pragma unroll
  for (int r = 0; r < kRounds; ++r)
    if ((vmask >> r) & 1u) {
      const uint32_t ahead = htot ? (uint32_t)S.hb[bwd_bucket(kreg[r], cd.mult) - b0] : 0u;
      dst[dest[r] + ahead] = make_uint2(kreg[r], sreg[r]);
    }
}

// The most frequent row id among 64 evenly spaced samples of a bucket (ties: the earliest sample):
// every wave of every workgroup that walks the bucket gets the same answer.
__device__ __forceinline__ uint32_t bwd_sample_mode(const uint2* __restrict__ src, int n, int lane) {
  const uint32_t sk = src[(int)(((int64_t)lane * n) / TZR_WAVE)].x;
  unsigned long long peers = ~0ull;
  for (int bit = 0; bit < 32; ++bit) {
    const int on = (sk >> bit) & 1;
    const unsigned long long bm = __ballot(on);
    peers &= on ? bm : ~bm;
  }
  uint32_t best = ((uint32_t)__popcll(peers) << 6) | (uint32_t)(TZR_WAVE - 1 - lane);
  for (int m = TZR_WAVE >> 1; m > 0; m >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, m, TZR_WAVE));
  return (uint32_t)__shfl((int)sk, TZR_WAVE - 1 - (int)(best & 63u), TZR_WAVE);
}

// A tile workgroup of a heavy bucket has to look at the WHOLE bucket once (counts ahead of its tile, totals).  Walked
// tile by tile by the whole workgroup that is a chain of one L2 round trip per tile -- 43 of them for the 43-tile bucket a
// clipped Zipf tail makes (70 us: the sort launch of a skewed batch, profiles/r03bg).  Here every WAVE takes whole
// segments of BWD_HT positions (w, w + 4, ...) with the sixteen key loads of a lane in flight together: a quarter of the
// round trips, each four times as wide.  f(seg, valid, key) is called for the sixteen elements of a lane in position
// order; `seg` is wave-uniform.
#define BWD_SEGL (BWD_HT / TZR_WAVE)
template <class F>
__device__ __forceinline__ void bwd_walk_segments(const uint2* __restrict__ src, int n, int wv, int lane, F&& f) {
  for (int seg = wv; seg * BWD_HT < n; seg += BWD_WAVES) {
    const int base = seg * BWD_HT + lane;
    uint32_t k[BWD_SEGL];
#pragma unroll
    for (int j = 0; j < BWD_SEGL; ++j) k[j] = base + j * TZR_WAVE < n ? src[base + j * TZR_WAVE].x : 0u;
#pragma unroll
    for (int j = 0; j < BWD_SEGL; ++j) f(seg, j, base + j * TZR_WAVE < n, k[j]);
  }
}

__device__ __forceinline__ void bwd_sort_heavy_tile(const TzrTable* __restrict__ tables,
                                                    const BwdPlan& P, BwdSortLds& S,
                                                    const BwdHeavy& H) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int64_t rows = tables[H.t].rows;
  int nb;
  uint64_t mult;
  bwd_bucket_params(rows, &nb, &mult);
  const uint64_t klo64 = (((uint64_t)H.bin << 32) + mult - 1) / mult;
  uint64_t khi = (((uint64_t)(H.bin + 1) << 32) + mult - 1) / mult;
  if (khi > (uint64_t)rows) khi = (uint64_t)rows;
  const uint32_t klo = (uint32_t)klo64;
  const int wbits = bwd_bits((uint32_t)(khi - klo64 - 1));
  const int n = (int)(H.end - H.start);
  const uint2* __restrict__ src = P.ks[1] + H.start;
  uint2* __restrict__ dst = P.ks[0] + H.start;
  const int t0 = H.tile * BWD_HT;
  for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) S.gstart[i] = S.pre[i] = 0;
  __syncthreads();
  // counts of the bucket per row id: S.pre collects the segments ahead of this tile, S.gstart the others (added below)
  constexpr int kRounds = BWD_HT / BWD_THREADS;
  // (a heavy bucket usually is heavy because of ONE row: its lookups are counted with a ballot into
  // a wave register, the others -- few per wave, on different counters -- with one LDS atomic each)
  const uint32_t hot = bwd_sample_mode(src, n, lane);
  {
    const int tseg = t0 / BWD_HT;
    uint32_t hot_pre = 0, hot_post = 0;
    bwd_walk_segments(src, n, wv, lane, [&](int seg, int, bool v, uint32_t k) {
      const bool before = seg < tseg;  // wave-uniform
      const uint32_t c = (uint32_t)__popcll(__ballot(v && k == hot));
      if (before) hot_pre += c; else hot_post += c;
      if (v && k != hot) atomicAdd(before ? &S.pre[k - klo] : &S.gstart[k - klo], 1u);
    });
    if (lane == 0) {
      if (hot_pre) atomicAdd(&S.pre[hot - klo], hot_pre);
      if (hot_post) atomicAdd(&S.gstart[hot - klo], hot_post);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) S.gstart[i] += S.pre[i];
  __syncthreads();
  bwd_block_scan(S.gstart, BWD_NB, S.wtot);
  const int nt = min(BWD_HT, n - t0);
  const int pw = bwd_wave_span(nt);
  const int rounds = pw / TZR_WAVE;
  uint32_t kreg[kRounds], sreg[kRounds], dig[kRounds], dest[kRounds];
  uint32_t vmask = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int lp = wv * pw + r * TZR_WAVE + lane;
    kreg[r] = sreg[r] = dig[r] = 0u;
    if (r < rounds && lp < nt) {
      vmask |= 1u << r;
      const uint2 v = src[t0 + lp];
      kreg[r] = v.x;
      sreg[r] = v.y;
      dig[r] = v.x - klo;
    }
  }
  bwd_rank_tile<BWD_NB, kRounds>(dig, vmask, rounds, wbits, S.L, dest);
#pragma unroll
  for (int r = 0; r < kRounds; ++r)
    if ((vmask >> r) & 1u)
      dst[S.gstart[dig[r]] + S.pre[dig[r]] + (dest[r] - (uint32_t)S.L.lstart[dig[r]])] =
          make_uint2(kreg[r], sreg[r]);
  __syncthreads();
}

__device__ __forceinline__ void bwd_sort_heavy_serial(const TzrTable* __restrict__ tables,
                                                      const BwdPlan& P, BwdSortLds& S,
                                                      const BwdHeavy& H) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int64_t rows = tables[H.t].rows;
  int nb;
  uint64_t mult;
  bwd_bucket_params(rows, &nb, &mult);
  const uint64_t klo64 = (((uint64_t)H.bin << 32) + mult - 1) / mult;
  uint64_t khi = (((uint64_t)(H.bin + 1) << 32) + mult - 1) / mult;
  if (khi > (uint64_t)rows) khi = (uint64_t)rows;
  const uint32_t klo = (uint32_t)klo64;
  const int bits = max(1, bwd_bits((uint32_t)(khi - klo64 - 1)));
  // an odd number of passes ends in ks[0], where the apply reads
  const int npass = bits <= BWD_RB ? 1 : (bits <= 3 * BWD_RB ? 3 : 5);
  const int width = (bits + npass - 1) / npass;
  const unsigned mask = (1u << width) - 1u;
  const int n = (int)(H.end - H.start);
  constexpr int kRounds = BWD_HT / BWD_THREADS;
  if (n <= BWD_HT) {  // one tile: all passes without leaving LDS
    const uint2* __restrict__ src = P.ks[1] + H.start;
    uint2* __restrict__ dst = P.ks[0] + H.start;
    const int pw = bwd_wave_span(n);
    const int rounds = pw / TZR_WAVE;
    uint32_t kreg[kRounds], sreg[kRounds], dest[kRounds];
    uint32_t vmask = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int lp = wv * pw + r * TZR_WAVE + lane;
      kreg[r] = sreg[r] = 0u;
      if (r < rounds && lp < n) {
        vmask |= 1u << r;
        const uint2 v = src[lp];
        kreg[r] = v.x;
        sreg[r] = v.y;
      }
    }
    bwd_sort_core<kRounds>(kreg, sreg, vmask, pw, rounds, klo, bits, false, S, dest);
#pragma unroll
    for (int r = 0; r < kRounds; ++r)
      if ((vmask >> r) & 1u) dst[dest[r]] = make_uint2(kreg[r], sreg[r]);
    __syncthreads();
    return;
  }
  // ks[1] -> ks[0] -> ks[2] -> ks[0] (-> ks[2] -> ks[0]).  Never INTO ks[1]: when this is the fallback of a
  // hot-row bucket (bwd_sort_heavy_hot), the bucket's other tile workgroups may still be walking ks[1] to
  // take the very decision that sent tile 0 here -- writing it raced with them (found by review in round 3;
  // reachable only for a wide bucket holding > BWD_UMAX lookups besides its most frequent row).
  for (int pass = 0; pass < npass; ++pass) {
    const uint2* __restrict__ src = (pass == 0 ? P.ks[1] : ((pass & 1) ? P.ks[0] : P.ks[2])) + H.start;
    uint2* __restrict__ dst = ((pass & 1) ? P.ks[2] : P.ks[0]) + H.start;
    const int shift = pass * width;
    for (int i = threadIdx.x; i < BWD_NB; i += BWD_THREADS) S.gstart[i] = 0;
    __syncthreads();
    for (int base = 0; base < n; base += BWD_HT) {
      uint32_t k8[kRounds];
#pragma unroll
      for (int r = 0; r < kRounds; ++r) {
        const int i = base + r * BWD_THREADS + (int)threadIdx.x;
        k8[r] = i < n ? src[i].x : 0u;
      }
#pragma unroll
      for (int r = 0; r < kRounds; ++r) {
        if (base + r * BWD_THREADS >= n) break;  // wave-uniform
        const int i = base + r * BWD_THREADS + (int)threadIdx.x;
        bwd_wave_count(S.gstart, ((k8[r] - klo) >> shift) & mask, i < n, width, lane);
      }
    }
    __syncthreads();
    bwd_block_scan(S.gstart, BWD_NB, S.wtot);
    for (int t0 = 0; t0 < n; t0 += BWD_HT) {
      const int nt = min(BWD_HT, n - t0);
      const int pw = bwd_wave_span(nt);
      const int rounds = pw / TZR_WAVE;
      uint32_t kreg[kRounds], sreg[kRounds], dig[kRounds], dest[kRounds];
      uint32_t vmask = 0;
#pragma unroll
      for (int r = 0; r < kRounds; ++r) {
        const int lp = wv * pw + r * TZR_WAVE + lane;
        kreg[r] = sreg[r] = dig[r] = 0u;
        if (r < rounds && lp < nt) {
          vmask |= 1u << r;
          const uint2 v = src[t0 + lp];
          kreg[r] = v.x;
          sreg[r] = v.y;
          dig[r] = ((v.x - klo) >> shift) & mask;
        }
      }
      bwd_rank_tile<BWD_NB, kRounds>(dig, vmask, rounds, width, S.L, dest);
#pragma unroll
      for (int r = 0; r < kRounds; ++r)
        if ((vmask >> r) & 1u)
          dst[S.gstart[dig[r]] + (dest[r] - (uint32_t)S.L.lstart[dig[r]])] = make_uint2(kreg[r], sreg[r]);
      __syncthreads();
      for (int d = threadIdx.x; d < BWD_NB; d += BWD_THREADS)
        S.gstart[d] += (unsigned)S.L.lstart[d + 1] - (unsigned)S.L.lstart[d];
      __syncthreads();
    }
    __threadfence();  // this workgroup reads the pass's output back in the next pass
    __syncthreads();
  }
}

// Hot item: tile `H.tile` of a WIDE heavy bucket (more than BWD_NB row ids, more than one tile of
// lookups).  Such a bucket is almost always one hot row plus a sprinkle of cold ones, so instead of
// LSD passes by one workgroup (26 tiles x 3 passes for the clipped tail of a 40M-row table) every
// tile workgroup
//   1. picks the same candidate row: the most frequent of 64 evenly spaced samples of the bucket;
//   2. walks the bucket once counting lookups below / equal to the candidate (ballots only), and
//      remembers the counts at its own tile: they place its hot lookups, in position order, after
//      the cold rows below the candidate;
//   3. tile 0 also gathers the cold lookups (at most BWD_UMAX, else see below) in position order,
//      sorts them in LDS and writes them around the hot run.
// Every workgroup derives the same counts, so all of them take the same decision: when the cold
// lookups do not fit, tile 0 falls back to the LSD passes over the whole bucket and the others
// leave.  Resulting order: ascending row ids, position order inside a row, like everywhere else.
__device__ __forceinline__ void bwd_sort_heavy_serial(const TzrTable* __restrict__ tables,
                                                      const BwdPlan& P, BwdSortLds& S,
                                                      const BwdHeavy& H);

__device__ __forceinline__ void bwd_sort_heavy_hot(const TzrTable* __restrict__ tables,
                                                   const BwdPlan& P, BwdSortLds& S,
                                                   const BwdHeavy& H) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int n = (int)(H.end - H.start);
  const uint2* __restrict__ src = P.ks[1] + H.start;
  uint2* __restrict__ dst = P.ks[0] + H.start;
  const int t0 = H.tile * BWD_HT;
  constexpr int kRounds = BWD_HT / BWD_THREADS;
  // 1. candidate (identical in every wave of every tile workgroup of the bucket)
  const uint32_t hot = bwd_sample_mode(src, n, lane);
  // 2. one walk: lookups below / equal to the candidate, in the whole bucket and ahead of this tile
  uint32_t lt_tot = 0, eq_tot = 0, eq_pre = 0;
  const int nseg = (n + BWD_HT - 1) / BWD_HT;
  const bool seg_lists = H.tile == 0 && nseg < BWD_NB;  // tile 0 also notes the cold lookups of every segment (step 3)
  {
    const int tseg = t0 / BWD_HT;
    uint32_t eq_seg = 0;
    int cur_seg = -1;
    bwd_walk_segments(src, n, wv, lane, [&](int seg, int j, bool v, uint32_t k) {
      if (seg != cur_seg) {  // (wave-uniform: a new segment of this wave)
        cur_seg = seg;
        eq_seg = 0;
      }
      lt_tot += (uint32_t)__popcll(__ballot(v && k < hot));
      const uint32_t c = (uint32_t)__popcll(__ballot(v && k == hot));
      eq_tot += c;
      eq_seg += c;
      if (seg < tseg) eq_pre += c;
      if (seg_lists && j == BWD_SEGL - 1 && lane == 0) S.pre[seg] = (uint32_t)min(BWD_HT, n - seg * BWD_HT) - eq_seg;
    });
  }
  if (lane == 0) {  // wave-level partial counts (a tile's lookups are dealt over the four waves)
    S.gstart[wv] = lt_tot;
    S.gstart[BWD_WAVES + wv] = eq_tot;
    S.gstart[2 * BWD_WAVES + wv] = eq_pre;
  }
  __syncthreads();
  uint32_t n_lt = 0, n_eq = 0, eq_ahead = 0;
#pragma unroll
  for (int w = 0; w < BWD_WAVES; ++w) {
    n_lt += S.gstart[w];
    n_eq += S.gstart[BWD_WAVES + w];
    eq_ahead += S.gstart[2 * BWD_WAVES + w];
  }
  __syncthreads();
  const int n_cold = n - (int)n_eq;
  if (n_cold > BWD_UMAX) {  // not one hot row: every tile workgroup of the bucket sees the same numbers
    if (H.tile == 0) bwd_sort_heavy_serial(tables, P, S, H);
    return;
  }
  // the hot lookups of this tile, in position order, behind the hot lookups of the tiles before
  {
    const int nt = min(BWD_HT, n - t0);
    const int pw = bwd_wave_span(nt);
    const int rounds = pw / TZR_WAVE;
    uint32_t sreg[kRounds], hpos[kRounds];
    uint32_t hmask = 0, run = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int lp = wv * pw + r * TZR_WAVE + lane;
      bool is_hot = false;
      sreg[r] = hpos[r] = 0;
      if (r < rounds && lp < nt) {
        const uint2 v = src[t0 + lp];
        sreg[r] = v.y;
        is_hot = v.x == hot;
      }
      if (r < rounds) {
        const unsigned long long hm = __ballot(is_hot);
        hpos[r] = run + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
        run += (uint32_t)__popcll(hm);
        if (is_hot) hmask |= 1u << r;
      }
    }
    if (lane == 0) S.wtot[wv] = run;
    __syncthreads();
    uint32_t ahead = n_lt + eq_ahead;
    for (int w = 0; w < wv; ++w) ahead += S.wtot[w];
#pragma unroll
    for (int r = 0; r < kRounds; ++r)
      if ((hmask >> r) & 1u) dst[ahead + hpos[r]] = make_uint2(hot, sreg[r]);
    __syncthreads();
  }
  if (H.tile != 0 || n_cold == 0) return;
  // 3. the cold lookups of the whole bucket: ordered gather into LDS, stable sort, write
  if (seg_lists) {
    // S.pre[seg] = cold lookups of segment seg (noted by the walk above) -> their offsets; then every wave places the
    // cold lookups of its segments: position order = segment, round, lane.  No workgroup barrier per tile.
    for (int i = nseg + (int)threadIdx.x; i < BWD_NB; i += BWD_THREADS) S.pre[i] = 0;
    __syncthreads();
    bwd_block_scan(S.pre, BWD_NB - 1, S.wtot);  // (the scan stores the total behind its last element: S.pre[BWD_NB - 1])
    uint32_t run = 0;
    int cur_seg = -1;
    bwd_walk_segments(src, n, wv, lane, [&](int seg, int j, bool v, uint32_t k) {
      if (seg != cur_seg) {
        cur_seg = seg;
        run = S.pre[seg];
      }
      const bool cold = v && k != hot;
      const unsigned long long cm = __ballot(cold);
      if (cold) {
        const uint32_t pos = run + (uint32_t)__popcll(cm & ((1ull << lane) - 1ull));
        S.pk[pos] = k;
        S.ps[pos] = src[seg * BWD_HT + j * TZR_WAVE + lane].y;
      }
      run += (uint32_t)__popcll(cm);
    });
    __syncthreads();
  } else {
    uint32_t gathered = 0;  // cold lookups in the tiles walked so far (workgroup-uniform)
    for (int base = 0; base < n; base += BWD_HT) {
      const int nt = min(BWD_HT, n - base);
      const int pw = bwd_wave_span(nt);
      const int rounds = pw / TZR_WAVE;
      uint32_t kc[kRounds], sc[kRounds], cpos[kRounds];
      uint32_t cmask = 0, run = 0;
  #pragma unroll
      for (int r = 0; r < kRounds; ++r) {
        const int lp = wv * pw + r * TZR_WAVE + lane;
        bool cold = false;
        kc[r] = sc[r] = cpos[r] = 0;
        if (r < rounds && lp < nt) {
          const uint2 v = src[base + lp];
          kc[r] = v.x;
          sc[r] = v.y;
          cold = v.x != hot;
        }
        if (r < rounds) {
          const unsigned long long cm = __ballot(cold);
          cpos[r] = run + (uint32_t)__popcll(cm & ((1ull << lane) - 1ull));
          run += (uint32_t)__popcll(cm);
          if (cold) cmask |= 1u << r;
        }
      }
      if (lane == 0) S.wtot[wv] = run;
      __syncthreads();
      uint32_t ahead = gathered, tile_cold = 0;
  #pragma unroll
      for (int w = 0; w < BWD_WAVES; ++w) {
        if (w < wv) ahead += S.wtot[w];
        tile_cold += S.wtot[w];
      }
  #pragma unroll
      for (int r = 0; r < kRounds; ++r)
        if ((cmask >> r) & 1u) {
          S.pk[ahead + cpos[r]] = kc[r];
          S.ps[ahead + cpos[r]] = sc[r];
        }
      gathered += tile_cold;
      __syncthreads();
    }
  }
  {
    constexpr int cRounds = BWD_UMAX / BWD_THREADS;
    const int64_t rows = tables[H.t].rows;
    int nb;
    uint64_t mult;
    bwd_bucket_params(rows, &nb, &mult);
    const uint64_t klo64 = (((uint64_t)H.bin << 32) + mult - 1) / mult;
    uint64_t khi = (((uint64_t)(H.bin + 1) << 32) + mult - 1) / mult;
    if (khi > (uint64_t)rows) khi = (uint64_t)rows;
    const int bits = max(1, bwd_bits((uint32_t)(khi - klo64 - 1)));
    const int pw = bwd_wave_span(n_cold);
    const int rounds = pw / TZR_WAVE;
    uint32_t kreg[cRounds], sreg[cRounds], dest[cRounds];
    uint32_t vmask = 0;
#pragma unroll
    for (int r = 0; r < cRounds; ++r) {
      const int lp = wv * pw + r * TZR_WAVE + lane;
      kreg[r] = sreg[r] = 0;
      if (r < rounds && lp < n_cold) {
        vmask |= 1u << r;
        kreg[r] = S.pk[lp];
        sreg[r] = S.ps[lp];
      }
    }
    __syncthreads();  // the exchange buffer is the core's from here on
    bwd_sort_core<cRounds>(kreg, sreg, vmask, pw, rounds, (uint32_t)klo64, bits, false, S, dest);
#pragma unroll
    for (int r = 0; r < cRounds; ++r)
      if ((vmask >> r) & 1u) dst[dest[r] + (kreg[r] > hot ? n_eq : 0u)] = make_uint2(kreg[r], sreg[r]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(BWD_THREADS) TZR_WAVES_PER_EU(8) void tzr_bwd_sort_kernel(
    const TzrTable* __restrict__ tables, int n_units, unsigned total_blocks, BwdPlan P) {
  PLAN_PROF(3);
  __shared__ BwdSortLds S;
  const unsigned bid = blockIdx.x;
  if ((int)bid < n_units) {
    bwd_sort_unit(tables, P, S, (int)bid);
    return;
  }
  const unsigned nh = P.hcount[0];
  const unsigned workers = total_blocks - (unsigned)n_units;
  for (unsigned hi = bid - (unsigned)n_units; hi < nh; hi += workers) {
    const BwdHeavy H = P.hlist[hi];
    if (H.tile < 0) bwd_sort_heavy_serial(tables, P, S, H);
    else if (H.pad[0]) bwd_sort_heavy_hot(tables, P, S, H);
    else bwd_sort_heavy_tile(tables, P, S, H);
  }
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

int g_tzr_bwd_force_prep = 0;  // tzr_tune("bwd_force_prep"): take the > BWD_GEO geometry path
int g_tzr_bwd_ch = 0;          // tzr_tune("bwd_ch"): positions per chunk (0 = by problem size)
int g_tzr_bwd_one_wg_heavy = 0;  // tzr_tune("bwd_one_wg_heavy"): no tile-parallel heavy buckets
int g_tzr_bwd_no_fuse_sort = 0;  // tzr_tune("bwd_no_fuse_sort"): 1 = every unit is sorted by the sort launch (ks[0] complete: tzr_pooled_bwd_plan_view)

extern "C" int tzr_pooled_bwd_plan(const TzrTable* d_tables, int n_tables,
                                   const TzrFeature* d_feats, int n_feats, int n_keys,
                                   int64_t max_rows, int max_dim, const int64_t* d_values, const int64_t* d_offsets,
                                   int64_t n_values, int64_t n_positions, int64_t B,
                                   int uniform_bag_len, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (!d_tables || !d_feats || n_tables <= 0 || n_feats <= 0 || n_values < 0 || B < 0 ||
      max_dim <= 0 || max_rows < 0)
    return TZR_ERR_INVALID;
  const bool uniform = uniform_bag_len == 1;
  if (!uniform && !d_offsets) return TZR_ERR_INVALID;
  if (n_keys <= 0) return TZR_ERR_INVALID;
  if (n_values >= (1LL << 32) || (int64_t)n_keys * B >= (1LL << 32)) return TZR_ERR_UNSUPPORTED;
  if (max_rows > (1LL << 32)) return TZR_ERR_UNSUPPORTED;  // row ids travel as 32-bit keys
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return TZR_ERR_WORKSPACE;
  BwdPlan P;
  if (n_positions < 0 || n_positions >= (1LL << 32)) return TZR_ERR_UNSUPPORTED;
  if (bwd_layout(&P, ws, n_values, n_positions, n_feats, n_tables, max_dim) > ws_bytes)
    return TZR_ERR_WORKSPACE;
  if (n_values == 0 || B == 0) return TZR_OK;
  if (!d_values) return TZR_ERR_INVALID;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned chunks = (unsigned)P.max_chunks;
  P.fuse = g_tzr_bwd_no_fuse_sort ? 0 : 1;
  BwdSrcArgs A;
  A.feats = d_feats;
  A.values = d_values;
  A.offsets = d_offsets;
  A.B = B;
  A.uniform = (int)uniform;
  if (n_feats > BWD_GEO || n_tables > BWD_GEO || g_tzr_bwd_force_prep) {
    hipLaunchKernelGGL(tzr_bwd_prep_kernel, dim3(1), dim3(BWD_THREADS), 0, s, d_tables, n_tables, A,
                       n_feats, P);
    hipLaunchKernelGGL(tzr_bwd_hist_kernel<false>, dim3(chunks), dim3(BWD_THREADS), 0, s, d_tables,
                       n_tables, n_feats, A, P);
  } else {
    hipLaunchKernelGGL(tzr_bwd_hist_kernel<true>, dim3(chunks), dim3(BWD_THREADS), 0, s, d_tables,
                       n_tables, n_feats, A, P);
  }
  hipLaunchKernelGGL(tzr_bwd_scan_kernel, dim3(n_tables * P.nslices), dim3(BWD_NB), 0, s, d_tables, n_tables,
                     g_tzr_bwd_one_wg_heavy, P);
  hipLaunchKernelGGL(tzr_bwd_scatter_kernel, dim3(chunks), dim3(BWD_THREADS), 0, s, d_tables,
                     n_tables, A, P);
  const unsigned workers = (unsigned)std::min<int64_t>(P.max_heavy, 1024);
  hipLaunchKernelGGL(tzr_bwd_sort_kernel, dim3(chunks + workers), dim3(BWD_THREADS), 0, s, d_tables,
                     (int)chunks, chunks + workers, P);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
