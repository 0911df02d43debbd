// K9b: the DLRM dot interaction FUSED with the first layer of the MLP behind it (gfx950): the kernels and the C entry points.
// The device bodies and what they do are in interaction_top_body.h.
#include "interaction_top_body.h"

#ifdef IT_PROF
uint64_t* g_tzr_it_prof = nullptr;
extern "C" void tzr_it_prof_table(uint64_t* d_table) { g_tzr_it_prof = d_table; }
#endif

__global__ __launch_bounds__(IT_THREADS) void tzr_ia_top_bwd_kernel(ItBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float Z[2 * IT_TS * IT_ZPD];  // the dz tile(s); 2 x 16 x 884 >= 16 x 1028
  __shared__ float Xs[IT_WAVES][IT_XS];     // per wave: the X image of its sample
  __shared__ __attribute__((aligned(16))) float Gs[2 * IT_TS * IT_GP];   // the g1 tile, double-buffered
  __shared__ float Wx[IT_KS * TZR_WAVE];    // W1 fragment of wave 0's extra block (it_bwd_loop<NB, true>)
  __shared__ uint16_t Tab[32 * IT_TP];      // byte offset of pair (k, c) in a sample's dz row
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TZR_WAVE));  // (scalar: per-wave bases stay in SGPRs)
  const int n = a.n;
  const int P = n * (n - 1) / 2;
  const int npb = (P + 15) >> 4, nblk = npb + n;
  // DLRM-Criteo: 49 blocks = 3 per wave and one more for wave 0 (fragment in LDS); up to 48: 3 per wave, zero-weighted;
  // more: 4 per wave in registers (spills, correct)
  if (nblk <= 3 * IT_WAVES) it_bwd_loop<3, false>(a, Z, &Xs[wv][0], Gs, Wx, Tab, lane, wv, 0);
  else if (n == IT_N_CRITEO) it_bwd_loop<3, true>(a, Z, &Xs[wv][0], Gs, Wx, Tab, lane, wv, 0);  // (the one n with 3 x 16 + 1 blocks)
  else it_bwd_loop<4, false>(a, Z, &Xs[wv][0], Gs, Wx, Tab, lane, wv, 0);
}

template <bool ZOUT>
__device__ __forceinline__ void it_fwd_body(const ItFwdArgs& a) {
  // two z tiles at the pitch of the body + the partial sums (it_fwd_criteo: two sets of them behind its smaller tiles)
  constexpr int kZCriteo = 2 * IT_TS * (16 * 49 + 4), kYs = 4 * IT_TS * IT_YP;
  __shared__ __attribute__((aligned(16))) float Sm[2 * IT_TS * IT_ZP + kYs];
  __shared__ float trash[IT_THREADS];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TZR_WAVE));  // (scalar: per-wave bases stay in SGPRs)
  float* tr = trash + threadIdx.x;
  // Criteo (27 vectors: 22 pair blocks + 27 = 49): 12 blocks + 1 k-step per wave (49 MFMAs, 49 registers of W1); other
  // shapes run the longest body, zero-weighted
  if (a.n == IT_N_CRITEO) {
    if (ZOUT) it_fwd_loop<12, 1, ZOUT, IT_N_CRITEO>(a, Sm, Sm + kZCriteo, tr, lane, wv);
    else it_fwd_criteo(a, Sm, Sm + 2 * IT_C_ZT, lane, wv);
  } else {
    it_fwd_loop<IT_KB, 3, ZOUT, 0>(a, Sm, Sm + 2 * IT_TS * IT_ZP, tr, lane, wv);
  }
}

// two kernels, not one branch: the registers of the z-writing body (store addresses, a second set of X rows) would be the
// budget of the other one too, and W1 fragments of the training step's forward (z = null) would be spilled
__global__ __launch_bounds__(IT_THREADS) void tzr_ia_top_fwd_kernel(ItFwdArgs a) { it_fwd_body<false>(a); }
__global__ __launch_bounds__(IT_THREADS) void tzr_ia_top_fwd_z_kernel(ItFwdArgs a) { it_fwd_body<true>(a); }

// tzr_tune("it_fwd_stagger"): forward, order of row building and product in a wave's turn: 0 / 1 = half of the waves each way
// (two of the four on every SIMD), 2 / 3 = every wave row-first / row-second.  Half and half is the default for both
// kernels: with the z stores it hides them behind the other half's product (111.6 vs 116-118 us, profiles/r04ap); without
// them (it_fwd_criteo) the row-first waves give the MFMA pipe work right behind the barrier (84.5 vs 85.9 us, profiles/r05ba)
int g_tzr_it_fwd_stagger = 0;
int g_tzr_it_wgs = 0;  // tzr_tune("it_wgs"): workgroups of the fused kernels (0 = one per CU)

extern "C" int tzr_dot_interaction_top_supported(int F, int D, int has_dense, int H) {
  const int n = F + (has_dense ? 1 : 0);
  if (D != IT_D || H != IT_H || n < 2 || n > 32) return 0;
  return ((n * (n - 1) / 2 + 15) / 16 + n) <= IT_MAXBLK ? 1 : 0;
}

// W1 [64][ldw] of the 27-vector shape -> its two copies in fragment order (either destination may be null)
__global__ __launch_bounds__(256) void tzr_ia_top_pack_w1_kernel(const float* __restrict__ W1, int64_t ldw, float* __restrict__ fwd,
                                                                 float* __restrict__ bwd) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= IT_PACK_H * IT_PACK_VCOLS) return;
  const int h = idx / IT_PACK_VCOLS, vc = idx - h * IT_PACK_VCOLS;
  const int col = it_real_col(vc, IT_PACK_P, IT_PACK_NPB, IT_PACK_NPB + IT_PACK_N);
  const float w = col >= 0 ? W1[(int64_t)h * ldw + col] : 0.f;
  int pf, pb;
  it_pack_pos(h, vc, &pf, &pb);
  if (fwd) fwd[pf] = w;
  if (bwd) bwd[pb] = w;
}

extern "C" int tzr_ia_top_pack_w1(const float* d_W1, int64_t ldw, int n, float* d_fwd_packed, float* d_bwd_packed, void* stream) {
  if (!d_W1 || (!d_fwd_packed && !d_bwd_packed)) return TZR_ERR_INVALID;
  if (n != IT_PACK_N) return TZR_ERR_UNSUPPORTED;
  if (ldw < IT_PACK_WIDTH || ((reinterpret_cast<uintptr_t>(d_fwd_packed) | reinterpret_cast<uintptr_t>(d_bwd_packed)) & 15)) return TZR_ERR_INVALID;
  hipLaunchKernelGGL(tzr_ia_top_pack_w1_kernel, dim3((IT_PACK_H * IT_PACK_VCOLS + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     d_W1, ldw, d_fwd_packed, d_bwd_packed);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_ia_top_packed_floats(void) { return IT_PACK_FLOATS; }

extern "C" int tzr_dot_interaction_top_bwd_packed(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                                  int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1,
                                                  int64_t g1_stride, int H, const float* d_W1, int64_t ldw,
                                                  const float* d_scale, float* d_grad_dense, int64_t grad_dense_stride,
                                                  float* d_grad_sparse, int64_t grad_sparse_stride, const float* d_W1_bwd_packed,
                                                  void* stream) {
  ItBwdArgs a;
  const int rc = it_bwd_prepare(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_W1, ldw, d_scale, d_grad_dense,
                                grad_dense_stride, d_grad_sparse, grad_sparse_stride, d_W1_bwd_packed, &a);
  if (rc != TZR_OK || B == 0) return rc;
  hipLaunchKernelGGL(tzr_ia_top_bwd_kernel, dim3(it_grid(B)), dim3(IT_THREADS), 0, static_cast<hipStream_t>(stream), a);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_dot_interaction_top_bwd(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                           int64_t sparse_stride, int F, int D, int64_t B, const float* d_g1,
                                           int64_t g1_stride, int H, const float* d_W1, int64_t ldw,
                                           const float* d_scale, float* d_grad_dense, int64_t grad_dense_stride,
                                           float* d_grad_sparse, int64_t grad_sparse_stride, void* stream) {
  return tzr_dot_interaction_top_bwd_packed(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_g1, g1_stride, H, d_W1, ldw, d_scale,
                                            d_grad_dense, grad_dense_stride, d_grad_sparse, grad_sparse_stride, nullptr, stream);
}

extern "C" int tzr_dot_interaction_top_fwd_packed(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                                  int64_t sparse_stride, int F, int D, int64_t B, const float* d_W1,
                                                  int64_t ldw, const float* d_bias, int H, int relu, float* d_z,
                                                  int64_t z_stride, float* d_y1, int64_t y1_stride, const float* d_W1_fwd_packed,
                                                  void* stream) {
  ItFwdArgs a;
  const int rc = it_fwd_prepare(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_W1, ldw, d_bias, H, relu, d_z, z_stride, d_y1,
                                y1_stride, d_W1_fwd_packed, &a);
  if (rc != TZR_OK || B == 0) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d_z) hipLaunchKernelGGL(tzr_ia_top_fwd_z_kernel, dim3(it_grid(B)), dim3(IT_THREADS), 0, st, a);
  else hipLaunchKernelGGL(tzr_ia_top_fwd_kernel, dim3(it_grid(B)), dim3(IT_THREADS), 0, st, a);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_dot_interaction_top_fwd(const float* d_dense, int64_t dense_stride, const float* d_sparse,
                                           int64_t sparse_stride, int F, int D, int64_t B, const float* d_W1,
                                           int64_t ldw, const float* d_bias, int H, int relu, float* d_z,
                                           int64_t z_stride, float* d_y1, int64_t y1_stride, void* stream) {
  return tzr_dot_interaction_top_fwd_packed(d_dense, dense_stride, d_sparse, sparse_stride, F, D, B, d_W1, ldw, d_bias, H, relu, d_z, z_stride,
                                            d_y1, y1_stride, nullptr, stream);
}
