// The bf16 vocabulary of the MFMA tile kernels: the 8-wide operand fragment of v_mfma_f32_16x16x32_bf16, the one rounding
// (fp32 -> bf16, to nearest even), 16-byte moves of eight bf16, and the product itself.  Values travel as bits (uint16_t in
// memory and LDS, four dwords in registers); a fragment becomes __bf16 only as the instruction's operand.
// Under TZR_EMU (the lane emulator of tests/, which knows the two fp32 MFMAs alone) the product has a plain C++ body on
// __shfl that follows the instruction's lane map; the fp64 tests on the device settle that the map is the device's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tzr_tile.h"

typedef __bf16 tzr_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t tzr_u32x4 __attribute__((ext_vector_type(4)));  // eight bf16 as bits

__device__ __forceinline__ tzr_u32x4 tzr_zero16() { return tzr_u32x4{0u, 0u, 0u, 0u}; }
__device__ __forceinline__ tzr_u32x4 tzr_ld16(const uint16_t* p) { return *reinterpret_cast<const tzr_u32x4*>(p); }
__device__ __forceinline__ void tzr_st16(uint16_t* p, tzr_u32x4 v) { *reinterpret_cast<tzr_u32x4*>(p) = v; }
// through a pointer KNOWN to be device memory (global, not FLAT, instructions: tzr_gfx950.h says why that matters next to LDS)
#ifdef TZR_EMU
__device__ __forceinline__ tzr_u32x4 tzr_ldg16(const uint16_t* p) { return tzr_ld16(p); }
__device__ __forceinline__ void tzr_stg16(uint16_t* p, tzr_u32x4 v) { tzr_st16(p, v); }
__device__ __forceinline__ void tzr_stg2(uint16_t* p, uint16_t v) { *p = v; }
#else
__device__ __forceinline__ tzr_u32x4 tzr_ldg16(const uint16_t* p) { return *(const __attribute__((address_space(1))) tzr_u32x4*)p; }
__device__ __forceinline__ void tzr_stg16(uint16_t* p, tzr_u32x4 v) { *(__attribute__((address_space(1))) tzr_u32x4*)p = v; }
__device__ __forceinline__ void tzr_stg2(uint16_t* p, uint16_t v) { *(__attribute__((address_space(1))) uint16_t*)p = v; }
#endif

// fp32 -> bf16, round to nearest even, as bits (a NaN stays a quiet NaN).  The device's conversion instruction rounds the same way.
__device__ __forceinline__ uint16_t tzr_bf16_rne(float f) {
#ifdef TZR_EMU
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
#else
  return __builtin_bit_cast(uint16_t, (__bf16)f);
#endif
}
__device__ __forceinline__ float tzr_bf16_widen(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// eight fp32 (lo: elements 0 .. 3, hi: 4 .. 7), each rounded once, as bits
__device__ __forceinline__ tzr_u32x4 tzr_pack_bf16x8(tzr_f32x4 lo, tzr_f32x4 hi) {
  tzr_u32x4 r;
  r[0] = (uint32_t)tzr_bf16_rne(lo[0]) | ((uint32_t)tzr_bf16_rne(lo[1]) << 16);
  r[1] = (uint32_t)tzr_bf16_rne(lo[2]) | ((uint32_t)tzr_bf16_rne(lo[3]) << 16);
  r[2] = (uint32_t)tzr_bf16_rne(hi[0]) | ((uint32_t)tzr_bf16_rne(hi[1]) << 16);
  r[3] = (uint32_t)tzr_bf16_rne(hi[2]) | ((uint32_t)tzr_bf16_rne(hi[3]) << 16);
  return r;
}

// v_mfma_f32_16x16x32_bf16, D = A B + C with fp32 accumulators: lane l supplies A[l & 15][8 (l >> 4) .. + 7] and
// B[8 (l >> 4) .. + 7][l & 15]; register r of lane l is D[4 (l >> 4) + r][l & 15].  Every lane of the wave calls it.
__device__ __forceinline__ tzr_f32x4 tzr_mfma_bf16(tzr_u32x4 a, tzr_u32x4 b, tzr_f32x4 c) {
#ifdef TZR_EMU
  struct Pair { tzr_u32x4 a, b; };
  const Pair mine{a, b};
  const int l = (int)(threadIdx.x & 63u), col = l & 15, g = l >> 4;
  float av[4][32], bv[32];
  for (int kg = 0; kg < 4; ++kg) {
    const Pair pb = __shfl(mine, col + 16 * kg);
    for (int e = 0; e < 8; ++e) bv[8 * kg + e] = tzr_bf16_widen((uint16_t)(pb.b[e >> 1] >> (16 * (e & 1))));
    for (int r = 0; r < 4; ++r) {
      const Pair pa = __shfl(mine, 4 * g + r + 16 * kg);
      for (int e = 0; e < 8; ++e) av[r][8 * kg + e] = tzr_bf16_widen((uint16_t)(pa.a[e >> 1] >> (16 * (e & 1))));
    }
  }
  tzr_f32x4 d;
  for (int r = 0; r < 4; ++r) {  // a k-ordered fmaf chain over the widened operands
    float acc = c[r];
    for (int k = 0; k < 32; ++k) acc = fmaf(av[r][k], bv[k], acc);
    d[r] = acc;
  }
  return d;
#else
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tzr_bf16x8, a), __builtin_bit_cast(tzr_bf16x8, b), c, 0, 0, 0);
#endif
}

// host side: a width the 16-byte accesses of a bf16 tile kernel take
static inline bool tzr_dim8_ok(int d, int max) { return d >= 8 && d <= max && !(d & 7); }
