// The vocabulary of the MFMA tile kernels: the accumulator type, the four-chain product, the clamped jagged span and the small
// scalar helpers, once.  Plain HIP, nothing gfx950-only: the lane emulator of tests/ compiles this file as it is.
// A helper here replaces a private copy only where the expression tree is the same -- the same operations in the same order,
// the same shuffle masks in the same sequence; a look-alike that rounds differently stays private, with a comment saying why.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the accumulator of v_mfma_f32_16x16x4_f32 (and the 16-byte builtin vector of tzr_ldg4 / tzr_stg4)
typedef float tzr_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ tzr_f32x4 tzr_acc_zero() { return tzr_f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ void tzr_acc_zero(tzr_f32x4* acc, int n) {
#pragma unroll
  for (int e = 0; e < n; ++e) acc[e] = tzr_acc_zero();
}

// Four k-slots of one float4 into four accumulator chains, and the chains' join.  __forceinline__: a kernel compiled with
// packed fp32 off (mwdin, hstu) relies on the inlined body taking its setting.
__device__ __forceinline__ void tzr_mfma4(float4 a, float4 b, tzr_f32x4* acc) {
  acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[1], 0, 0, 0);
  acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[2], 0, 0, 0);
  acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[3], 0, 0, 0);
}
__device__ __forceinline__ tzr_f32x4 tzr_join4(const tzr_f32x4* acc) { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }

// The rows of the samples b0 .. b1 - 1 of a jagged batch over N rows, as first row and length, with the offsets clamped into
// [0, N] and the end not in front of the start: whatever the offsets hold, no access derived from the span leaves the buffers.
__device__ __forceinline__ void tzr_jagged_span(const int64_t* off, int64_t b0, int64_t b1, int64_t N, int64_t* start, int64_t* len) {
  int64_t s0 = off[b0], s1 = off[b1];
  s0 = s0 < 0 ? 0 : (s0 > N ? N : s0);
  s1 = s1 < s0 ? s0 : (s1 > N ? N : s1);
  *start = s0;
  *len = s1 - s0;
}

__device__ __forceinline__ float tzr_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float tzr_sigmoid(float s) { return 1.0f / (1.0f + expf(-s)); }
// over the 16 lanes that share lane >> 4, by the xor tree with masks 1, 2, 4, 8: every one of them ends with the sum
__device__ __forceinline__ float tzr_sum16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// host side: a width the float4 accesses of a tile kernel take; a persistent grid of one workgroup a sample, capped
static inline bool tzr_dim4_ok(int d, int max) { return d >= 4 && d <= max && !(d & 3); }
static inline int64_t tzr_capped_grid(int64_t B, int64_t max) { return B < max ? B : max; }
