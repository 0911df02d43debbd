// K9c: the weight gradient of the Linear behind the DLRM dot interaction, dW1 = g1^T z, WITHOUT z in HBM (gfx950): the kernels and
// the C entry points.  The device bodies, the column-group plan and the slice count are in interaction_wgrad_body.h.
#include "interaction_wgrad_body.h"

__global__ __launch_bounds__(WG_THREADS) void tzr_ia_wgrad_kernel(WgArgs a) {
  __shared__ __attribute__((aligned(16))) float zT[2 * WG_ZT];  // [tile][sample][column]
  __shared__ __attribute__((aligned(16))) float gT[2 * WG_S * WG_PG];  // [tile][sample][h]
  wg_workgroup(a, zT, gT, threadIdx.x);
}

__global__ __launch_bounds__(256) void tzr_ia_wgrad_reduce_kernel(WgReduceArgs a) {
  const int lane = threadIdx.x & 63;
  const int o = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (lane & 15);
  int h, c;
  bool live;
  const float v = wg_reduce_output(a, o, lane, &h, &c, &live);
  if (live && (lane >> 4) == 0) a.dW[(int64_t)h * a.ldw + c] = v;
}

int g_tzr_wg_debug = 0;  // tzr_tune("wg_debug"): phase-skipping bits for timing experiments (1 no product, 2 no tile build, 4 no loads, 8 no main kernel, 16 no reduce kernel): wrong results

extern "C" int64_t tzr_dot_interaction_top_wgrad_workspace(int F, int D, int has_dense, int H) {
  if (!tzr_dot_interaction_top_supported(F, D, has_dense, H)) return 0;
  WgGroup g[WG_NG];
  int vw;
  wg_plan(F + (has_dense ? 1 : 0), g, &vw);
  return (int64_t)WG_MAXSLICES * WG_H * vw * (int64_t)sizeof(float);
}

// The weight-gradient kernel alone: the batch slices' partial sums stay in d_ws and `ra` says how to add them up
// (wg_reduce_output) -- for tzr_dot_interaction_top_wgrad's own reduce launch, or for a consumer that takes them as they are
// (tzr_dense_adam_fused).
static int wgrad_partials(const float* d_dense, int64_t dense_stride, const float* d_sparse, int64_t sparse_stride, int F, int D,
                          int64_t B, const float* d_g1, int64_t g1_stride, int H, const float* d_scale, void* d_ws, int64_t ws_bytes,
                          WgReduceArgs* ra, void* stream) {
  WgArgs a;
  const int rc = wg_prepare(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_scale, d_ws, ws_bytes, ra, &a);
  if (rc != TZR_OK) return rc;
  if (B > 0) {
    if (!(g_tzr_wg_debug & 8))
      hipLaunchKernelGGL(tzr_ia_wgrad_kernel, dim3(WG_NG * a.slices), dim3(WG_THREADS), 0, static_cast<hipStream_t>(stream), a);
    TZR_CHECK_LAUNCH();
  }
  return TZR_OK;
}

extern "C" int tzr_dot_interaction_top_wgrad(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                             int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1,
                                             int64_t g1_stride, int H, const float* d_scale, float* d_dW1, int64_t ldw,
                                             void* d_ws, int64_t ws_bytes, void* stream) {
  const int n = F + (d_dense ? 1 : 0);
  const int width = n * (n - 1) / 2 + WG_D * n;
  if (!d_dW1 || ldw < width || (reinterpret_cast<uintptr_t>(d_dW1) & 3)) return TZR_ERR_INVALID;
  WgReduceArgs ra;
  const int rc = wgrad_partials(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_scale, d_ws, ws_bytes, &ra,
                                stream);
  if (rc != TZR_OK) return rc;
  ra.dW = d_dW1;
  ra.ldw = ldw;
  if (!(g_tzr_wg_debug & 16))
    hipLaunchKernelGGL(tzr_ia_wgrad_reduce_kernel, dim3((WG_H * width + 63) / 64), dim3(256), 0, static_cast<hipStream_t>(stream), ra);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// ... without the reduce launch: h_out (TzrWgradParts, include/tzrec_hip.h) describes the partial sums for tzr_dense_adam_fused,
// which adds them up on its way to the Adam update of W1 (B > 0; d_ws stays the caller's until that call has run).
extern "C" int tzr_dot_interaction_top_wgrad_parts(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                                   int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1,
                                                   int64_t g1_stride, int H, const float* d_scale, void* d_ws, int64_t ws_bytes,
                                                   TzrWgradParts* h_out, void* stream) {
  static_assert(sizeof(WgReduceArgs) <= sizeof(TzrWgradParts), "the opaque blob of the C ABI holds the reduce arguments");
  if (!h_out || B <= 0) return TZR_ERR_INVALID;
  WgReduceArgs ra;
  const int rc = wgrad_partials(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_scale, d_ws, ws_bytes, &ra,
                                stream);
  if (rc != TZR_OK) return rc;
  std::memset(h_out, 0, sizeof(*h_out));
  std::memcpy(h_out, &ra, sizeof(ra));
  return TZR_OK;
}
