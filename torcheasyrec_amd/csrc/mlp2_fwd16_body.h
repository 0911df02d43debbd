// The bottom MLP's forward on the matrix cores, one wave per 16-sample tile (mlp_mfma.hip: tzr_mlp2_fwd16_kernel), as a body
// that another unit's launch can run as well: interaction_phases.hip runs it as phase 0 of the fused interaction forward (no
// -fgpu-rdc: a body two units call has to be visible in both).
#pragma once
#include "tzr_common.h"

#define MM_TS 16
#define MT_H1 64
#define MT_P1 (MT_H1 + 4)  // row pitches: 16-byte aligned rows, b128 reads of 16 rows spread over the banks

typedef float mm_f32x4 __attribute__((ext_vector_type(4)));

// ---- bottom MLP: ha = relu(x Wa^T + ba) [B, 64], hb = relu(ha Wb^T + bb) [B, 16]; K0 <= 16 ---------------------------------
#define MB_H1 64
#define MB_H2 16
#define MB_PX 20  // row pitch of the [16 x 16] tiles (x, masked dhb)

// One wave: the tiles t0, t0 + step, ... of 16 samples.  T1: the wave's own ha tile in LDS (MM_TS * MT_P1 floats, 16-byte
// aligned); no workgroup barrier.
__device__ __forceinline__ void mb_fwd16_tiles(
    const float* __restrict__ x, int64_t xs, int64_t B, int K0, const float* __restrict__ Wa, const float* __restrict__ ba,
    const float* __restrict__ Wb, const float* __restrict__ bb, float* __restrict__ ha, int64_t has, float* __restrict__ hb,
    int64_t hbs, float* T1, int lane, int64_t t0, int64_t step) {
  const int r = lane & 15, q = lane >> 4;
  // B operands: first layer k = 4 ks + q over the inputs (zero beyond K0): Wa[16 hb + r][k]; second layer k = 16 q + ks over
  // the 64 hidden units: Wb[r][k]
  float Wfa[4][4], Wfb[16], bav[4];
#pragma unroll
  for (int hbk = 0; hbk < 4; ++hbk) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = 4 * ks + q;
      const float w = Wa[(16 * hbk + r) * K0 + (k < K0 ? k : 0)];
      Wfa[hbk][ks] = k < K0 ? w : 0.f;
    }
    bav[hbk] = ba ? ba[16 * hbk + r] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 v = tzr_ld4(Wb + r * MB_H1 + 16 * q + 4 * i);
    Wfb[4 * i] = v.x; Wfb[4 * i + 1] = v.y; Wfb[4 * i + 2] = v.z; Wfb[4 * i + 3] = v.w;
  }
  const float bbv = bb ? bb[r] : 0.f;
  const int64_t tiles = (B + MM_TS - 1) / MM_TS;
  for (int64_t t = t0; t < tiles; t += step) {
    const int64_t b0 = t * MM_TS;
    // ---- A = x[sample r][4 ks + q] straight from HBM (the whole tile is 16 x K0 floats)
    float xa[4];
    {
      const int64_t b = b0 + r < B ? b0 + r : B - 1;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int k = 4 * ks + q;
        const float v = x[b * xs + (k < K0 ? k : 0)];
        xa[ks] = (k < K0 && b0 + r < B) ? v : 0.f;
      }
    }
    mm_f32x4 acc[4];
#pragma unroll
    for (int hbk = 0; hbk < 4; ++hbk) acc[hbk] = mm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int hbk = 0; hbk < 4; ++hbk) acc[hbk] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks], Wfa[hbk][ks], acc[hbk], 0, 0, 0);
    // reg j of lane (r, q): sample 4 q + j, unit 16 hbk + r -> the ha tile in LDS
#pragma unroll
    for (int hbk = 0; hbk < 4; ++hbk)
#pragma unroll
      for (int j = 0; j < 4; ++j) T1[(4 * q + j) * MT_P1 + 16 * hbk + r] = fmaxf(acc[hbk][j] + bav[hbk], 0.f);
    __builtin_amdgcn_wave_barrier();
    // ---- ha out (rows of 256 bytes, 16 bytes per lane) and hb = relu(ha Wb^T + bb): A = ha[sample r][16 q + ks]
    mm_f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + TZR_WAVE * i, row = e >> 4, c4 = e & 15;
      if (b0 + row < B) tzr_st4(ha + (b0 + row) * has + 4 * c4, tzr_ld4(T1 + row * MT_P1 + 4 * c4));
      const float4 av = tzr_ld4(T1 + r * MT_P1 + 16 * q + 4 * i);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, Wfb[4 * i], acc2, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, Wfb[4 * i + 1], acc2, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, Wfb[4 * i + 2], acc2, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, Wfb[4 * i + 3], acc2, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (b0 + 4 * q + j < B) hb[(b0 + 4 * q + j) * hbs + r] = fmaxf(acc2[j] + bbv, 0.f);
    __builtin_amdgcn_wave_barrier();  // (the next tile overwrites T1)
  }
}

// whether tzr_mlp2_fwd runs this body for a shape (mlp_ops.hip decides; g_tzr_mlp_mfma < 0 switches the MFMA kernels off)
static inline bool mb_fwd16_fits(int K0, int H1, int H2, const float* d_Wb, const float* d_ha, int64_t ha_stride) {
  return K0 > 0 && K0 <= 16 && H1 == MB_H1 && H2 == MB_H2 && !(ha_stride & 3) && !(reinterpret_cast<uintptr_t>(d_ha) & 15) &&
         !(reinterpret_cast<uintptr_t>(d_Wb) & 15);
}
