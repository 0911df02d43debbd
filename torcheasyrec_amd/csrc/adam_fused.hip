// Dense Adam that takes its gradients as they lie: finished tensors, rows of per-workgroup partial sums (tzr_mlp2_bwd_parts) or
// the batch slices of the first top-MLP layer's weight gradient (tzr_dot_interaction_top_wgrad_parts) -- ONE launch for every
// tensor of the step.
//
// Replaces TZRecOptimizer.step() of the reference for the dense parameters (/root/reference/tzrec/optim/optimizer.py:56-68:
// torch.optim.Adam built by optim/optimizer_builder.py; same arithmetic as tzr_dense_adam, csrc/dense_ops.hip) AND the
// launches that used to stand between the backward and it in the DLRM step (models/dlrm.py:101-135): two column-sum
// finishes, the weight gradient's slice reduction and the optimizer's own step-counter launch were 4 of the step's 17
// launches, 20 us of dependent round trips for < 14 MB (profiles/r05final3/kernel_stats.csv).  Here a gradient element is
// summed by the threads that then update its parameter (csrc/fused_grad.h: partial-sum rows in the blocked order of
// csrc/parts_sum.h, as tzr_mlp2_bwd's finish, and the slice reduction's own order -- bit-identical to those two; the column sums
// whose separate finish is the interleaved order differ from it by fp32 rounding); the step counter of a tensor is read by every workgroup and moved on by the LAST of the
// tensor's workgroups to finish.
#include "fused_grad.h"
#include "interaction_pack.h"

namespace {

struct FusedTable {
  TzrAdamTensor t[TZR_ADAM_MAX_TENSORS];
  FusedPlan p;
};

// the tensor of the launch (-1: none) that is the fused interaction layer's W1 [64][783], and its copies in fragment order
struct PackedW1 {
  float *fwd, *bwd;
  int tensor;
};

}  // namespace

__global__ __launch_bounds__(256) void tzr_adam_fused_kernel(FusedTable T, PackedW1 W, const float* __restrict__ lr_ptr, float lr_host,
                                                             float b1, float b2, float eps, float wd) {
  __shared__ float sl[16][17];
  int y = 0;
  while (y + 1 < T.p.n && (int)blockIdx.x >= T.p.first[y + 1]) ++y;  // (workgroup-uniform, <= 32 steps through kernel arguments)
  const TzrAdamTensor a = T.t[y];
  const int lb = (int)blockIdx.x - T.p.first[y], nblk = T.p.first[y + 1] - T.p.first[y];
  // every workgroup of the tensor reads the SAME step count (it only moves when the last of them is done)
  float* const state = reinterpret_cast<float*>(a.state);
  AdamK k;
  k.lr = lr_ptr ? *lr_ptr : lr_host;
  k.b1 = b1; k.b2 = b2; k.eps = eps; k.wd = wd;
  float step = 1.0f;
  if (a.param) {
    step = state[0] + 1.0f;
    adam_bias(k, step);
  }
  float* __restrict__ p = reinterpret_cast<float*>(a.param);
  float* __restrict__ m = reinterpret_cast<float*>(a.exp_avg);
  float* __restrict__ v = reinterpret_cast<float*>(a.exp_avg_sq);
  float* __restrict__ gout = reinterpret_cast<float*>(a.grad);
  // a.param == 0: the gradient is only stored (a caller that wants the finished tensor after all)
  fused_grad_each(T.p.s[y], T.p.wg, gout, a.numel, lb, nblk, sl, [&](int64_t i, float gi) {
    if (!p) gout[i] = gi;
    else adam_update(p, m, v, k, i, p[i], gi);
    if (y == W.tensor) {  // (workgroup-uniform) the new value into W1's packed copies too: the interaction kernels read those
      const int h = (int)(i / IT_PACK_WIDTH), col = (int)(i - (int64_t)h * IT_PACK_WIDTH);
      int pf, pb;
      it_pack_pos(h, it_pack_vcol(col), &pf, &pb);
      const float w = p[i];
      if (W.fwd) W.fwd[pf] = w;
      if (W.bwd) W.bwd[pb] = w;
    }
  });
  if (a.param) fused_step_arrive(state, lb, nblk, step);
}

// h_sources (nullable: every gradient is a finished tensor) runs parallel to h_tensors; at most one source of kind
// TZR_ADAM_SRC_WGRAD, described by h_wgrad.  A tensor with param == 0 only gets its finished gradient stored into `grad`.
extern "C" int tzr_dense_adam_fused_w1(const TzrAdamTensor* h_tensors, const TzrAdamSource* h_sources, int n_tensors,
                                       const TzrWgradParts* h_wgrad, const float* d_lr, float lr, float beta1, float beta2, float eps,
                                       float weight_decay, const TzrPackedW1* h_w1, void* stream) {
  if (!h_tensors || n_tensors <= 0) return TZR_ERR_INVALID;
  if (h_w1 && ((h_w1->fwd_packed | h_w1->bwd_packed) & 15)) return TZR_ERR_INVALID;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int base = 0; base < n_tensors; base += TZR_ADAM_MAX_TENSORS) {
    FusedTable T;
    T.p.n = std::min(TZR_ADAM_MAX_TENSORS, n_tensors - base);
    std::memset(&T.p.wg, 0, sizeof(T.p.wg));
    PackedW1 W = {nullptr, nullptr, -1};
    int blocks = 0;
    for (int i = 0; i < T.p.n; ++i) {
      const TzrAdamTensor& a = h_tensors[base + i];
      T.t[i] = a;
      if (h_w1 && h_w1->param && a.param == h_w1->param) {
        if (a.numel != (int64_t)IT_PACK_H * IT_PACK_WIDTH) return TZR_ERR_INVALID;
        W.fwd = reinterpret_cast<float*>(h_w1->fwd_packed);
        W.bwd = reinterpret_cast<float*>(h_w1->bwd_packed);
        W.tensor = i;
      }
      if (a.param && (!a.exp_avg || !a.exp_avg_sq || !a.state)) return TZR_ERR_INVALID;
      const int rc = fused_plan_tensor(T.p, i, a.numel, a.param != 0, a.grad != 0, h_sources ? &h_sources[base + i] : nullptr, h_wgrad, &blocks);
      if (rc != TZR_OK) return rc;
    }
    T.p.first[T.p.n] = blocks;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(tzr_adam_fused_kernel, dim3((unsigned)blocks), dim3(256), 0, s, T, W, d_lr, lr, beta1, beta2, eps, weight_decay);
  }
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_dense_adam_fused(const TzrAdamTensor* h_tensors, const TzrAdamSource* h_sources, int n_tensors,
                                    const TzrWgradParts* h_wgrad, const float* d_lr, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, void* stream) {
  return tzr_dense_adam_fused_w1(h_tensors, h_sources, n_tensors, h_wgrad, d_lr, lr, beta1, beta2, eps, weight_decay, nullptr, stream);
}
