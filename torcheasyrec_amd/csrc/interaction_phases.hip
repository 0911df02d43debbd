// Two launches of the DLRM-Criteo training step as PHASES of the persistent interaction launches (gfx950).
//
// The step's kernel times add up to the step: there is no idle time between launches to recover, but every dependent launch
// pays a fixed price -- the drain of its slowest workgroup, the dispatch, a cold prologue.  The two persistent interaction
// kernels own their samples per workgroup, so two neighbours can move in without a change to any sum:
//
//   tzr_ia_top_fwd_mlp2_kernel   phase 0: the bottom MLP's forward (mlp2_fwd16_body.h) on exactly the 16-sample tiles whose dense
//                                rows this workgroup's interaction forward reads -- workgroup c owns tiles c, c + G, ...; wave k
//                                takes c + (k + 16 j) G.  A workgroup barrier (the rows a wave reads next were stored by other
//                                waves of the SAME workgroup: workgroup-scope release / acquire is enough), then phase 1 =
//                                it_fwd_criteo unchanged with the dense row = hb.  The W1 fragment loads are issued behind phase
//                                0, whose 89 registers would not fit beside the 48 fragment registers.
//   tzr_ia_top_bwd_wgrad_kernel  phase 1: it_bwd_loop<3, true> (dX of the interaction + first layer) on the first it_grid(B)
//                                workgroups; phase 2: the weight gradient's workgroup (interaction_wgrad_body.h) on the first
//                                4 x slices.  The weight gradient reads dense, sparse and g1 only -- inputs of the backward,
//                                nothing it writes -- so a workgroup goes on without waiting for the chip.  One raw LDS buffer
//                                serves both phases.
//
// Same bodies, same tiles per workgroup, same order of every addition, same partial-sum slices as the two-launch forms, which
// stay the path of every other shape.
#include "interaction_top_body.h"
#include "interaction_wgrad_body.h"
#include "mlp2_fwd16_body.h"

extern int g_tzr_mlp_mfma;  // mlp_ops.hip

struct PhMlp2Args {
  const float *x, *Wa, *ba, *Wb, *bb;
  float *ha, *hb;
  int64_t xs, has, hbs;
  int K0;
};

static_assert(IT_WAVES * MM_TS * MT_P1 <= 2 * IT_C_ZT, "phase 0's ha tiles (one per wave) lie in the z tiles' space");
static_assert(MM_TS == IT_TS, "the bottom MLP's tiles are the interaction's tiles");

__global__ __launch_bounds__(IT_THREADS) void tzr_ia_top_fwd_mlp2_kernel(ItFwdArgs a, PhMlp2Args m) {
  __shared__ __attribute__((aligned(16))) float Sm[IT_C_LDS_FLOATS];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TZR_WAVE));  // (scalar: per-wave bases stay in SGPRs)
  const int64_t G = gridDim.x;
  mb_fwd16_tiles(m.x, m.xs, a.B, m.K0, m.Wa, m.ba, m.Wb, m.bb, m.ha, m.has, m.hb, m.hbs, Sm + wv * (MM_TS * MT_P1), lane,
                 (int64_t)blockIdx.x + wv * G, IT_WAVES * G);
  __syncthreads();  // hb of this workgroup's tiles is visible to all of its waves; the ha tiles in LDS are dead
  it_fwd_criteo(a, Sm, Sm + 2 * IT_C_ZT, lane, wv);
}

__device__ __forceinline__ int ph_lane_id() {
#ifdef __AMDGCN__
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#else
  return (int)(threadIdx.x & (TZR_WAVE - 1));  // (host pass, lane emulator)
#endif
}

#define PH_B_LDS_FLOATS (IT_B_LDS_FLOATS > WG_LDS_FLOATS ? IT_B_LDS_FLOATS : WG_LDS_FLOATS)
static_assert(PH_B_LDS_FLOATS * 4 <= 160 * 1024, "one workgroup per CU: its LDS");

__global__ __launch_bounds__(IT_THREADS) void tzr_ia_top_bwd_wgrad_kernel(ItBwdArgs a, WgArgs w, int it_wgs) {
  __shared__ __attribute__((aligned(16))) float Sm[PH_B_LDS_FLOATS];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TZR_WAVE));  // (scalar: per-wave bases stay in SGPRs)
  if ((int)blockIdx.x < it_wgs)
    it_bwd_loop<3, true>(a, Sm + IT_B_Z, Sm + IT_B_XS + wv * IT_XS, Sm + IT_B_GS, Sm + IT_B_WX, reinterpret_cast<uint16_t*>(Sm + IT_B_TAB),
                         lane, wv, it_wgs);
  __syncthreads();  // every wave is done with the backward's LDS
  // (the thread's index anew, out of the wave's scalar and the lane counter: nothing of it stays in a vector register across
  // phase 1, which has none to spare)
  if ((int)blockIdx.x < WG_NG * w.slices) wg_workgroup(w, Sm, Sm + 2 * WG_ZT, (unsigned)(wv * TZR_WAVE + ph_lane_id()));
}

extern "C" int tzr_dot_interaction_top_fwd_mlp2(const float* d_x, int64_t x_stride, int64_t B, int K0, const float* d_Wa,
                                                const float* d_ba, int H1, const float* d_Wb, const float* d_bb, int H2, float* d_ha,
                                                int64_t ha_stride, float* d_hb, int64_t hb_stride, const float* d_dense,
                                                int64_t dense_stride, const float* d_sparse, int64_t sparse_stride, int F, int D,
                                                const float* d_W1, int64_t ldw, const float* d_bias, int H, int relu, float* d_z,
                                                int64_t z_stride, float* d_y1, int64_t y1_stride, const float* d_W1_fwd_packed,
                                                void* stream) {
  if (!d_x || !d_Wa || !d_Wb || !d_ha || !d_hb || B < 0 || K0 <= 0 || H1 <= 0 || H2 <= 0) return TZR_ERR_INVALID;
  // the one shape: the bottom MLP on the matrix cores, its output the dense row of the 27-vector interaction, z not written,
  // W1 in fragment order
  if (g_tzr_mlp_mfma < 0 || !mb_fwd16_fits(K0, H1, H2, d_Wb, d_ha, ha_stride)) return TZR_ERR_UNSUPPORTED;
  if (d_dense != d_hb || dense_stride != hb_stride || d_z || !d_W1_fwd_packed || F + 1 != IT_N_CRITEO) return TZR_ERR_UNSUPPORTED;
  ItFwdArgs a;
  const int rc = it_fwd_prepare(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_W1, ldw, d_bias, H, relu, d_z, z_stride, d_y1,
                                y1_stride, d_W1_fwd_packed, &a);
  if (rc != TZR_OK || B == 0) return rc;
  PhMlp2Args m;
  m.x = d_x; m.Wa = d_Wa; m.ba = d_ba; m.Wb = d_Wb; m.bb = d_bb; m.ha = d_ha; m.hb = d_hb;
  m.xs = x_stride; m.has = ha_stride; m.hbs = hb_stride; m.K0 = K0;
  hipLaunchKernelGGL(tzr_ia_top_fwd_mlp2_kernel, dim3(it_grid(B)), dim3(IT_THREADS), 0, static_cast<hipStream_t>(stream), a, m);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_dot_interaction_top_bwd_wgrad_parts(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                                       int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1,
                                                       int64_t g1_stride, int H, const float* d_W1, int64_t ldw, const float* d_scale,
                                                       float* d_grad_dense, int64_t grad_dense_stride, float* d_grad_sparse,
                                                       int64_t grad_sparse_stride, const float* d_W1_bwd_packed, void* d_ws,
                                                       int64_t ws_bytes, TzrWgradParts* h_out, void* stream) {
  static_assert(sizeof(WgReduceArgs) <= sizeof(TzrWgradParts), "the opaque blob of the C ABI holds the reduce arguments");
  if (!h_out || B <= 0) return TZR_ERR_INVALID;
  if (!d_dense || F + 1 != IT_N_CRITEO) return TZR_ERR_UNSUPPORTED;  // (the phase is it_bwd_loop<3, true>: 27 vectors)
  ItBwdArgs a;
  int rc = it_bwd_prepare(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_W1, ldw, d_scale, d_grad_dense,
                          grad_dense_stride, d_grad_sparse, grad_sparse_stride, d_W1_bwd_packed, &a);
  if (rc != TZR_OK) return rc;
  WgArgs w;
  WgReduceArgs ra;
  rc = wg_prepare(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_scale, d_ws, ws_bytes, &ra, &w);
  if (rc != TZR_OK) return rc;
  const unsigned it_wgs = it_grid(B), wg_wgs = (unsigned)(WG_NG * w.slices);
  hipLaunchKernelGGL(tzr_ia_top_bwd_wgrad_kernel, dim3(it_wgs > wg_wgs ? it_wgs : wg_wgs), dim3(IT_THREADS), 0,
                     static_cast<hipStream_t>(stream), a, w, (int)it_wgs);
  TZR_CHECK_LAUNCH();
  std::memset(h_out, 0, sizeof(*h_out));
  std::memcpy(h_out, &ra, sizeof(ra));
  return TZR_OK;
}
