// W1 of the fused interaction layer (csrc/interaction_top.hip) in the order of the kernels' MFMA fragments, DLRM-Criteo shape
// only (27 vectors of 16, H = 64: 49 virtual column blocks of 16, pairs padded to 22 blocks, then one block per X row).
//
// The two persistent kernels keep W1 in registers for the whole launch.  Out of the plain [64][ldw] matrix every workgroup
// has to re-order it through LDS first; out of these copies a lane's fragment is a run of 16-byte loads, coalesced over the
// wave.  Both copies hold every element of W1 exactly once, and the 64 slots of the one pad column (virtual column 351) as zeros:
//
//   forward  (wave = (K-group kg, output block hb), lane = (r, q)): [16 waves][12 blocks][64 lanes][4 k-steps], then the k-step
//            kg of the 49th block as [16 waves][64 lanes]
//   backward (wave w owns blocks w, w + 16, w + 32; lane = (r, q)): [16 waves][12 quads][64 lanes][4], quad j element e =
//            fragment register 4 j + e = 16 m + ks of block m; then the 49th block (wave 0's, kept in LDS) as [16 k-steps][64 lanes]
//
// it_pack_pos is THE definition: the pack kernel, the dense optimizer's launch and (through the it_pack_*_off helpers it is
// built on) both prologues use it.
#pragma once
#include <cstdint>

#ifndef TZR_PACK_HD
#define TZR_PACK_HD __host__ __device__ __forceinline__
#endif

#define IT_PACK_N 27                                        // vectors
#define IT_PACK_H 64                                        // rows of W1
#define IT_PACK_P (IT_PACK_N * (IT_PACK_N - 1) / 2)         // 351 pairs
#define IT_PACK_NPB ((IT_PACK_P + 15) / 16)                 // 22 blocks of them
#define IT_PACK_VCOLS (16 * (IT_PACK_NPB + IT_PACK_N))      // 784 virtual columns
#define IT_PACK_WIDTH (IT_PACK_P + 16 * IT_PACK_N)          // 783 columns of W1
#define IT_PACK_MAIN (16 * 12 * 64 * 4)                     // floats of the 48 whole blocks
#define IT_PACK_FLOATS (IT_PACK_MAIN + 16 * 64)             // floats of either copy (50 176)

// forward: the float4 of block m (0..11 of the wave's K-group) of lane `lane` of wave `wv`; the wave's k-step of the 49th block
TZR_PACK_HD int it_pack_fwd_off(int wv, int m, int lane) { return ((wv * 12 + m) * 64 + lane) * 4; }
TZR_PACK_HD int it_pack_fwd_x_off(int wv, int lane) { return IT_PACK_MAIN + wv * 64 + lane; }
// backward: quad j (registers 4 j .. 4 j + 3 of the 48) of lane `lane` of wave `wv`; k-step ks of the 49th block
TZR_PACK_HD int it_pack_bwd_off(int wv, int j, int lane) { return ((wv * 12 + j) * 64 + lane) * 4; }
TZR_PACK_HD int it_pack_bwd_x_off(int ks, int lane) { return IT_PACK_MAIN + ks * 64 + lane; }

// column of W1 -> virtual column (the pairs are padded to whole blocks)
TZR_PACK_HD int it_pack_vcol(int col) { return col < IT_PACK_P ? col : col + (16 * IT_PACK_NPB - IT_PACK_P); }

// where element [h][virtual column vc] of W1 lies in the two copies
TZR_PACK_HD void it_pack_pos(int h, int vc, int* fwd, int* bwd) {
  const int v = vc >> 4, w = vc & 15;
  {  // forward: B operand W1[h = 16 hb + r][column 4 q + kk of block v]
    const int hb = h >> 4, r = h & 15, q = w >> 2, kk = w & 3;
    const int lane = 16 * q + r;
    if (v < 48) *fwd = it_pack_fwd_off(4 * (v / 12) + hb, v % 12, lane) + kk;
    else *fwd = it_pack_fwd_x_off(4 * kk + hb, lane);  // (k-step kg of the last block belongs to K-group kg)
  }
  {  // backward: B operand W1[k = 16 q + ks][column r of block v]
    const int q = h >> 4, ks = h & 15;
    const int lane = 16 * q + w;
    if (v < 48) {
      const int f = 16 * (v >> 4) + ks;
      *bwd = it_pack_bwd_off(v & 15, f >> 2, lane) + (f & 3);
    } else {
      *bwd = it_pack_bwd_x_off(ks, lane);
    }
  }
}
