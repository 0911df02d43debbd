// What the one-wave-per-sample row kernels (cross_net.hip, ln_mask.hip) share on the host side: lane i of a wave holds
// elements i, i + 64, ... of a sample's row (KR = D / 64 rounded up to a power of two of them, a compile-time bound), a
// workgroup is four waves.  (Their common ending -- the four waves' accumulators through LDS into one row of partial sums,
// ((0 + 1) + 2) + 3 -- stays written out in both kernels: as a shared function it moved tzr_cross_bwd_kernel<16, *>'s
// register allocation, NOTES.md.)
#pragma once
#include "tzr_common.h"

// LAUNCH(KR) for the row width `D` of the calling scope
#define TZR_BY_KR(LAUNCH)          \
  do {                             \
    if (D <= 64) LAUNCH(1);        \
    else if (D <= 128) LAUNCH(2);  \
    else if (D <= 256) LAUNCH(4);  \
    else if (D <= 512) LAUNCH(8);  \
    else LAUNCH(16);               \
  } while (0)

// workgroups of a grid-stride launch over B samples, `waves` samples per workgroup and pass
static inline unsigned tzr_row_grid(int64_t B, int waves, int max_grid) {
  return (unsigned)std::min<int64_t>(max_grid, (B + waves - 1) / waves);
}
