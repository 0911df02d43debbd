// Adding up rows of per-workgroup partial sums: the ONE implementation of each of the two fixed orders that
// include/tzrec_hip.h documents as part of the ABI.  A backward kernel leaves G rows in a workspace (row g is workgroup g's),
// a small second launch -- or the fused dense optimizer's own -- adds them per column.  No atomics; the order of additions is
// a function of G alone, so every result is bit-reproducible.
//
//   interleaved   sixteen chains take the rows s, s + 16, s + 32, ... (s = 0..15), eight loads in flight each; the sixteen
//                 chain sums are then added 0..15.  1024 threads, 64 columns per workgroup.
//                 Who: tzr_parts_sum_finish_kernel (every finish of dense_ops.hip, linear_bwd.hip), tzr_gemm_tn_finish_kernel,
//                 tzr_cross_bwd_finish_kernel, tzr_ln_mask_bwd_finish_kernel.
//   blocked       sixteen contiguous ranges of ceil(G / 16) rows, eight loads in flight each; the sixteen range sums are then
//                 added 0..15.  256 threads, 16 columns per workgroup.
//                 Who: tzr_mlp_finish_kernel and every TZR_ADAM_SRC_ROWS source of the fused dense optimizers (fused_grad.h)
//                 -- also for rows whose separate finish is the interleaved one (tzr_relu_bwd_colsum_parts,
//                 tzr_skinny_linear_bwd_parts): equal to it up to fp32 rounding, as tzrec_hip.h says.
//
// Eight independent loads per pass because a serial walk is pure latency (60 us for 1024 rows, 120 us for 512 strided ones).
// A chain starts at +0.0f and a row that does not exist contributes +0.0f: x + (+0) is x and (+0) + (-0) is +0 under
// round-to-nearest, so a chain never holds -0.0f and `0 + c0 + c1 + ...` has the bits of `c0 + c1 + ...`.
//
// The callers pass the LDS in (the emulator's __shared__ is a function-local static).  The rows are device memory.
#pragma once
#include "tzr_common.h"

#define TZR_FIN_THREADS 1024
#define TZR_FIN_WAVES (TZR_FIN_THREADS / TZR_WAVE)

// Interleaved order.  Every thread of a TZR_FIN_THREADS workgroup calls it (a barrier inside); thread (chain = threadIdx.x /
// 64, column = threadIdx.x % 64 of the workgroup's 64).  `col0`: the thread's column in row 0, or null for a column that does
// not exist; `stride`: floats between rows; `red`: TZR_FIN_THREADS floats of LDS.  The column's total, in the threads of chain 0.
// ROLLED: the same chain -- the same additions, the same bits -- as a loop the compiler unrolls by eight without a bounds
// check per load, for tzr_cross_bwd_finish_kernel alone: with its odd row stride the eight guarded loads measured 5.95
// against 5.4 us (NOTES.md); the other four finishes measure the same either way and keep the explicit form.
template <bool ROLLED = false>
__device__ __forceinline__ float tzr_parts_sum_interleaved(const float* __restrict__ col0, int G, size_t stride, float* red) {
  const int chain = threadIdx.x / TZR_WAVE;
  float t = 0.f;
  if (col0 && ROLLED) {
#pragma unroll 8
    for (int k = chain; k < G; k += TZR_FIN_WAVES) t += tzr_ldg(col0 + (size_t)k * stride);
  } else if (col0) {
    for (int k0 = chain; k0 < G; k0 += TZR_FIN_WAVES * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + TZR_FIN_WAVES * u;
        v[u] = k < G ? tzr_ldg(col0 + (size_t)k * stride) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) t += v[u];
    }
  }
  red[threadIdx.x] = t;
  __syncthreads();
  float r = 0.f;
  if (chain == 0)
    for (int s = 0; s < TZR_FIN_WAVES; ++s) r += red[s * TZR_WAVE + threadIdx.x];
  return r;
}

// out[c] = the interleaved sum of column c of parts[G][N]: grid (N + 63) / 64, TZR_FIN_THREADS threads.  (static: the library
// is built without -fgpu-rdc, every file that launches it has a copy of its own; a template, launched as
// tzr_parts_sum_finish_kernel<>, so that a file that only calls the device functions has none.)
template <int = 0>
static __global__ __launch_bounds__(TZR_FIN_THREADS) void tzr_parts_sum_finish_kernel(const float* __restrict__ parts, int G, int N,
                                                                                      float* __restrict__ out) {
  __shared__ float red[TZR_FIN_THREADS];
  const int col = blockIdx.x * TZR_WAVE + (threadIdx.x & (TZR_WAVE - 1));
  const float r = tzr_parts_sum_interleaved(col < N ? parts + col : nullptr, G, (size_t)N, red);
  if (threadIdx.x < TZR_WAVE && col < N) out[col] = r;
}

// Blocked order.  Every thread of a 256-thread workgroup calls it (a barrier inside); thread (range = threadIdx.x / 16,
// column = threadIdx.x % 16 of the workgroup's 16).  `col0`, `stride`: as above; `sl`: 16 x 17 floats of LDS.  The column's
// total, in the threads of range 0.
__device__ __forceinline__ float tzr_parts_sum_blocked(const float* __restrict__ col0, int G, size_t stride, float (*sl)[17]) {
  const int ol = threadIdx.x & 15, range = threadIdx.x >> 4;
  const int per = (G + 15) / 16;
  const int g0 = range * per, g1 = min(G, g0 + per);
  float v = 0.f;
  if (col0) {
    for (int g = g0; g < g1; g += 8) {
      float t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = g + j < g1 ? tzr_ldg(col0 + (size_t)(g + j) * stride) : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) v += t[j];
    }
  }
  sl[range][ol] = v;
  __syncthreads();
  v = 0.f;
  if (range == 0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) v += sl[q][ol];
  }
  return v;
}
