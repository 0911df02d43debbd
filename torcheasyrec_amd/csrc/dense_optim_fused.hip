// The dense optimizer step of every kind the config can name -- SGD, Adagrad, Adam, AdamW, Adadelta, RMSprop -- over every
// dense tensor of the step, whatever mix of kinds, in ONE launch.
//
// Replaces TZRecOptimizer.step() of the reference for the dense parameters (tzrec/optim/optimizer.py:56-68) where
// tzrec/optim/optimizer_builder.py:100-136 builds a torch.optim class out of train_config.dense_optimizer and :139-260 more of
// them for the `part_optimizers`: one foreach launch chain per optimizer there.  Here a tensor carries the index of its group
// {kind, learning rate, hyper-parameters}; per element the arithmetic is torch.optim's single-tensor path in fp32.  Gradients
// are taken as they lie, as tzr_dense_adam_fused takes them (csrc/fused_grad.h: the same summation, the same step-count
// arrival tree), so every kind can consume the partial sums a backward left behind.
#include "fused_grad.h"

namespace {

struct OptTable {
  TzrDenseOptTensor t[TZR_ADAM_MAX_TENSORS];
  TzrDenseOptGroup g[TZR_DENSE_OPT_MAX_GROUPS];
  FusedPlan p;
};

}  // namespace

__global__ __launch_bounds__(256) void tzr_dense_optim_fused_kernel(OptTable T) {
  __shared__ float sl[16][17];
  int y = 0;
  while (y + 1 < T.p.n && (int)blockIdx.x >= T.p.first[y + 1]) ++y;  // (workgroup-uniform, <= 32 steps through kernel arguments)
  const TzrDenseOptTensor a = T.t[y];
  const int lb = (int)blockIdx.x - T.p.first[y], nblk = T.p.first[y + 1] - T.p.first[y];
  float* __restrict__ gout = reinterpret_cast<float*>(a.grad);
  if (!a.param) {  // the gradient is only stored
    fused_grad_each(T.p.s[y], T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) { gout[i] = gi; });
    return;
  }
  const TzrDenseOptGroup grp = T.g[a.group];
  // every workgroup of the tensor reads the SAME step count (it only moves when the last of them is done)
  float* const state = reinterpret_cast<float*>(a.state);
  const float step = state[0] + 1.0f;
  const float lr = grp.d_lr ? *reinterpret_cast<const float*>(grp.d_lr) : grp.lr;
  const float wd = grp.weight_decay, eps = grp.eps, h0 = grp.hp0, h1 = grp.hp1;
  float* __restrict__ p = reinterpret_cast<float*>(a.param);
  float* __restrict__ s0 = reinterpret_cast<float*>(a.state0);
  float* __restrict__ s1 = reinterpret_cast<float*>(a.state1);
  const FusedSrc src = T.p.s[y];
  // (the kind is workgroup-uniform: one branch per workgroup, the element loops are each kind's own)
  switch (grp.kind) {
    case TZR_DENSE_OPT_SGD: {
      const bool first = step == 1.0f, nesterov = (grp.flags & TZR_DENSE_OPT_NESTEROV) != 0;
      fused_grad_each(src, T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) {
        const float pi = p[i];
        if (wd != 0.f) gi = fmaf(wd, pi, gi);
        if (s0) {  // momentum != 0
          const float b = first ? gi : fmaf(h0, s0[i], (1.0f - h1) * gi);
          s0[i] = b;
          gi = nesterov ? fmaf(h0, b, gi) : b;
        }
        p[i] = fmaf(-lr, gi, pi);
      });
      break;
    }
    case TZR_DENSE_OPT_ADAGRAD:
      fused_grad_each(src, T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) {
        const float pi = p[i];
        if (wd != 0.f) gi = fmaf(wd, pi, gi);
        const float si = fmaf(gi, gi, s0[i]);
        s0[i] = si;
        p[i] = pi + (-lr * gi) / (sqrtf(si) + eps);
      });
      break;
    case TZR_DENSE_OPT_ADAM:
    case TZR_DENSE_OPT_ADAMW: {
      AdamK k;
      k.lr = lr; k.b1 = h0; k.b2 = h1; k.eps = eps;
      k.wd = grp.kind == TZR_DENSE_OPT_ADAM ? wd : 0.f;
      adam_bias(k, step);
      const float decay = grp.kind == TZR_DENSE_OPT_ADAMW ? 1.0f - lr * wd : 1.0f;  // AdamW: p *= 1 - lr wd first
      fused_grad_each(src, T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) {
        float pi = p[i];
        if (decay != 1.0f) pi *= decay;
        adam_update(p, s0, s1, k, i, pi, gi);
      });
      break;
    }
    case TZR_DENSE_OPT_ADADELTA:
      fused_grad_each(src, T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) {
        const float pi = p[i];
        if (wd != 0.f) gi = fmaf(wd, pi, gi);
        const float sq = fmaf(h0, s0[i], (1.0f - h0) * gi * gi);
        const float acc = s1[i];
        const float delta = sqrtf(acc + eps) / sqrtf(sq + eps) * gi;
        s0[i] = sq;
        s1[i] = fmaf(h0, acc, (1.0f - h0) * delta * delta);
        p[i] = fmaf(-lr, delta, pi);
      });
      break;
    default:  // TZR_DENSE_OPT_RMSPROP (the host refuses every other value)
      fused_grad_each(src, T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) {
        const float pi = p[i];
        if (wd != 0.f) gi = fmaf(wd, pi, gi);
        const float sq = fmaf(h0, s0[i], (1.0f - h0) * gi * gi);
        s0[i] = sq;
        p[i] = pi + (-lr * gi) / (sqrtf(sq) + eps);
      });
      break;
  }
  fused_step_arrive(state, lb, nblk, step);
}

// state tensors a kind reads and writes: -1 an unknown kind
static int dense_opt_states(const TzrDenseOptGroup& g) {
  switch (g.kind) {
    case TZR_DENSE_OPT_SGD: return g.hp0 != 0.f ? 1 : 0;
    case TZR_DENSE_OPT_ADAGRAD: case TZR_DENSE_OPT_RMSPROP: return 1;
    case TZR_DENSE_OPT_ADAM: case TZR_DENSE_OPT_ADAMW: case TZR_DENSE_OPT_ADADELTA: return 2;
    default: return -1;
  }
}

// Everything is checked before the first launch: an error code means nothing was launched.
extern "C" int tzr_dense_optim_fused(const TzrDenseOptTensor* h_tensors, const TzrAdamSource* h_sources, int n_tensors,
                                     const TzrDenseOptGroup* h_groups, int n_groups, const TzrWgradParts* h_wgrad, void* stream) {
  if (!h_tensors || n_tensors <= 0 || n_groups < 0 || (n_groups > 0 && !h_groups)) return TZR_ERR_INVALID;
  if (n_groups > TZR_DENSE_OPT_MAX_GROUPS) return TZR_ERR_UNSUPPORTED;
  for (int j = 0; j < n_groups; ++j)
    if (dense_opt_states(h_groups[j]) < 0) return TZR_ERR_INVALID;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int pass = 0; pass < 2; ++pass) {  // 0: check every launch, 1: launch
    for (int base = 0; base < n_tensors; base += TZR_ADAM_MAX_TENSORS) {
      OptTable T;
      std::memset(&T, 0, sizeof(T));
      T.p.n = std::min(TZR_ADAM_MAX_TENSORS, n_tensors - base);
      for (int j = 0; j < n_groups; ++j) T.g[j] = h_groups[j];
      int blocks = 0;
      for (int i = 0; i < T.p.n; ++i) {
        const TzrDenseOptTensor& a = h_tensors[base + i];
        T.t[i] = a;
        if (a.param) {
          if (a.group < 0 || a.group >= n_groups || !a.state) return TZR_ERR_INVALID;
          const int ns = dense_opt_states(h_groups[a.group]);
          if ((ns >= 1 && !a.state0) || (ns >= 2 && !a.state1)) return TZR_ERR_INVALID;
          if (ns == 0) T.t[i].state0 = 0;  // (the kernel tells SGD without momentum by it)
        }
        const int rc = fused_plan_tensor(T.p, i, a.numel, a.param != 0, a.grad != 0, h_sources ? &h_sources[base + i] : nullptr, h_wgrad, &blocks);
        if (rc != TZR_OK) return rc;
      }
      T.p.first[T.p.n] = blocks;
      if (pass == 0 || blocks == 0) continue;
      hipLaunchKernelGGL(tzr_dense_optim_fused_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T);
    }
  }
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
