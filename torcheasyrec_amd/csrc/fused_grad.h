// What the one-launch dense optimizers (csrc/adam_fused.hip, csrc/dense_optim_fused.hip) share: the table of gradient sources
// of a launch, the host code that lays a launch out, the summation of a gradient element out of its source, Adam's element and
// the arrival tree that moves a tensor's step count on.  Both entries add a gradient up through fused_grad_each, and that adds
// partial-sum rows by parts_sum.h's blocked order: the summation exists once.
#pragma once
#include <tzr_gfx950.h>

#include <algorithm>
#include <cstring>

#include "parts_sum.h"
#include "tzr_common.h"
#include "wgrad_reduce.h"

struct FusedSrc {
  int kind;  // 0 finished gradient, 1 partial-sum rows, 2 weight-gradient slices
  int G, P, col;
  const float* parts;
};

struct FusedPlan {
  FusedSrc s[TZR_ADAM_MAX_TENSORS];
  int first[TZR_ADAM_MAX_TENSORS + 1];  // first workgroup of every tensor
  int n;
  WgReduceArgs wg;
};

struct AdamK {
  float lr, b1, b2, eps, wd, step_size, bc2_sqrt;
};

// the bias corrections of step `step` (torch.optim.Adam: step_size = lr / (1 - b1^step), denominators over sqrt(1 - b2^step))
__device__ __forceinline__ void adam_bias(AdamK& k, float step) {
  k.step_size = k.lr / (1.0f - powf(k.b1, step));
  k.bc2_sqrt = sqrtf(1.0f - powf(k.b2, step));
}

// torch.optim.Adam (amsgrad off, L2 weight decay k.wd), element i with gradient gi and parameter value pi (the caller has read
// it: AdamW decays it first)
__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const AdamK& k, int64_t i,
                                            float pi, float gi) {
  if (k.wd != 0.f) gi = fmaf(k.wd, pi, gi);
  const float mi = fmaf(1.0f - k.b1, gi - m[i], m[i]);  // lerp, as torch's fused kernel
  const float vi = fmaf(k.b2, v[i], (1.0f - k.b2) * gi * gi);
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
  p[i] = pi - k.step_size * (mi / denom);
}

// Workgroup `lb` of the `nblk` of a tensor of `numel` elements: f(i, g_i) for every element i that is this workgroup's, g_i
// added up out of the tensor's source.  `sl`: 16 x 17 floats of LDS.  Every thread of the workgroup calls it (a barrier inside).
template <class F>
__device__ __forceinline__ void fused_grad_each(const FusedSrc& src, const WgReduceArgs& wg, const float* __restrict__ grad, int64_t numel,
                                                int lb, int nblk, float (*sl)[17], F f) {
  if (src.kind == 0) {
    // (src.parts != 0 with a finished tensor: the gradient is read from THERE -- a store-only call then copies it to `grad`, which is
    // how a set of gradients is packed into one flat buffer for a collective, partial sums and finished tensors in one launch)
    const float* __restrict__ g = src.parts ? src.parts : grad;
    for (int64_t i = (int64_t)lb * 256 + threadIdx.x; i < numel; i += (int64_t)nblk * 256) f(i, g[i]);
  } else if (src.kind == 1) {
    // 16 outputs per workgroup, added in the blocked order of parts_sum.h (tzr_mlp_finish_kernel's too)
    const int64_t o = (int64_t)lb * 16 + (threadIdx.x & 15);
    const float v = tzr_parts_sum_blocked(o < numel ? src.parts + src.col + o : nullptr, src.G, (size_t)src.P, sl);
    if (threadIdx.x < 16 && o < numel) f(o, v);
  } else {
    const int lane = threadIdx.x & 63;
    const int o = (lb * 4 + (int)(threadIdx.x >> 6)) * 16 + (lane & 15);
    int h, c;
    bool live;
    const float v = wg_reduce_output(wg, o, lane, &h, &c, &live);
    if (live && (lane >> 4) == 0) f((int64_t)o, v);  // (the parameter is [64, width] contiguous: element o)
  }
}

// The tensor's step count moves on when its last workgroup is done.  Arrivals go through a two-level tree -- groups of 32
// workgroups (state[2 + group]), the last of a group then arrives at state[1]: every counter is zero between launches, and none
// of them sees more than 32 arrivals (783 workgroups arriving at ONE word cost 11 us of a 20 us launch: profiles/r06k).
__device__ __forceinline__ void fused_step_arrive(float* state, int lb, int nblk, float step) {
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t* cnt = reinterpret_cast<uint32_t*>(state + 1);
    const int grp = lb >> 5, ngrp = (nblk + 31) >> 5;
    const uint32_t in_grp = (uint32_t)min(32, nblk - (grp << 5));
    if (tzr_arrive(cnt + 1 + grp) == in_grp - 1u) {
      tzr_publish_u32(cnt + 1 + grp, 0u);
      if (tzr_arrive(cnt) == (uint32_t)ngrp - 1u) {
        tzr_publish_u32(cnt, 0u);
        state[0] = step;
      }
    }
  }
}

// Host: tensor i of a launch (numel elements, gradient at `grad`, stepped or only stored) and its source `src` (nullable: a
// finished tensor) -> P.s[i], P.first[i]; *blocks moves on by the tensor's workgroups.  At most one TZR_ADAM_SRC_WGRAD source
// per launch (P.wg, zero before the first tensor).  Refuses a partial-sum source whose workgroups would not
// fit the arrival counters of a state row, and a partial-sum source with nowhere to go.
static inline int fused_plan_tensor(FusedPlan& P, int i, int64_t numel, bool has_param, bool has_grad, const TzrAdamSource* src,
                                    const TzrWgradParts* h_wgrad, int* blocks) {
  const int skind = src ? src->kind : TZR_ADAM_SRC_TENSOR;
  if (numel < 0) return TZR_ERR_INVALID;
  if (!has_grad && (skind == TZR_ADAM_SRC_TENSOR || !has_param)) return TZR_ERR_INVALID;
  FusedSrc& fs = P.s[i];
  fs.kind = 0; fs.G = fs.P = fs.col = 0; fs.parts = nullptr;
  P.first[i] = *blocks;
  int nb;
  if (skind == TZR_ADAM_SRC_ROWS) {
    if (!src->parts || src->G <= 0 || src->P <= 0 || src->col < 0 || src->col + numel > src->P) return TZR_ERR_INVALID;
    if ((numel + 15) / 16 > 1024) return TZR_ERR_UNSUPPORTED;  // (32 groups of 32 arrivals: TZR_ADAM_FUSED_STATE)
    fs.kind = 1; fs.G = src->G; fs.P = src->P; fs.col = src->col; fs.parts = reinterpret_cast<const float*>(src->parts);
    nb = (int)((numel + 15) / 16);
  } else if (skind == TZR_ADAM_SRC_WGRAD) {
    if (!h_wgrad || P.wg.part) return TZR_ERR_INVALID;
    std::memcpy(&P.wg, h_wgrad, sizeof(P.wg));
    const int n = P.wg.n, width = n * (n - 1) / 2 + WG_D * n;
    if (!P.wg.part || numel != (int64_t)WG_H * width) return TZR_ERR_INVALID;
    if ((WG_H * width + 63) / 64 > 1024) return TZR_ERR_UNSUPPORTED;
    fs.kind = 2;
    nb = (WG_H * width + 63) / 64;
  } else {
    if (src && src->parts) fs.parts = reinterpret_cast<const float*>(src->parts);
    nb = (int)std::min<int64_t>(1024, (numel + 255) / 256);
  }
  *blocks += std::max(nb, numel > 0 ? 1 : 0);
  if (numel == 0) P.first[i] = *blocks;  // (no workgroup: its step count does not move, as a tensor without a gradient's)
  return TZR_OK;
}
