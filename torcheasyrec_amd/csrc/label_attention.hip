// MIND's label-aware attention (tzrec/models/mind.py:303-333): the positive item of a sample attends over the sample's interests.
//   a_k = <I_bk, v_b>;  w = softmax over the valid capsules of simi_pow a_k (a masked capsule's weight is exactly 0);
//   user_emb_b = sum_k w_k I_bk
//   backward:  t_k = <g_b, I_bk>;  da_k = simi_pow w_k (t_k - sum_j w_j t_j);  dI_bk = w_k g_b + da_k v_b (zero rows for masked
//   capsules);  dv_b = sum_k da_k I_bk
// One wave per sample, four samples a workgroup, one launch each way; lane l holds the float4 at columns 4 l of every row (D <=
// 256), the K <= 8 interests of the sample in registers.  Dots by a fixed xor tree, sums over k ascending: two runs are bit-equal.
// A sample without a valid capsule (the capsule layer never makes one) gets zeros.
#include "tzr_common.h"

#define LA_THREADS 256
#define LA_WAVES (LA_THREADS / TZR_WAVE)
#define LA_MAXK TZR_LABEL_ATTN_MAX_K
#define LA_MAXD TZR_LABEL_ATTN_MAX_D

static_assert(LA_MAXD <= 4 * TZR_WAVE, "one float4 a lane");

__device__ __forceinline__ float la_dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// grid ceil(B / 4)
__global__ __launch_bounds__(LA_THREADS) void tzr_label_attn_fwd_kernel(const float* __restrict__ I, int64_t is, const float* __restrict__ V, int64_t vs,
                                                                        const unsigned char* __restrict__ mask, int64_t B, int K, int D, float simi_pow,
                                                                        float* __restrict__ out, int64_t os, float* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * LA_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;  // (a whole wave)
  const bool cok = 4 * lane < D;
  const float4 v = cok ? tzr_ld4(V + b * vs + 4 * lane) : tzr_zero4();
  float4 x[LA_MAXK];
  float s[LA_MAXK];
  bool valid[LA_MAXK];
  float m = -3.0e38f;
#pragma unroll
  for (int k = 0; k < LA_MAXK; ++k) {
    valid[k] = k < K && mask[b * K + k] != 0;
    x[k] = cok && valid[k] ? tzr_ld4(I + (b * K + k) * is + 4 * lane) : tzr_zero4();
    s[k] = tzr_wave_sum(la_dot4(x[k], v)) * simi_pow;
    if (valid[k]) m = fmaxf(m, s[k]);
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < LA_MAXK; ++k) {
    s[k] = valid[k] ? expf(s[k] - m) : 0.f;
    sum += s[k];
  }
  float4 u = tzr_zero4();
#pragma unroll
  for (int k = 0; k < LA_MAXK; ++k) {
    s[k] = valid[k] ? s[k] / sum : 0.f;
    u = tzr_fma4(s[k], x[k], u);
    if (lane == 0 && k < K) w[b * K + k] = s[k];
  }
  if (cok) tzr_st4(out + b * os + 4 * lane, u);
}

__global__ __launch_bounds__(LA_THREADS) void tzr_label_attn_bwd_kernel(const float* __restrict__ G, int64_t gs, const float* __restrict__ I, int64_t is,
                                                                        const float* __restrict__ V, int64_t vs, const float* __restrict__ w,
                                                                        const unsigned char* __restrict__ mask, int64_t B, int K, int D, float simi_pow,
                                                                        float* __restrict__ dI, int64_t dis, float* __restrict__ dV, int64_t dvs) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * LA_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const bool cok = 4 * lane < D;
  const float4 v = cok ? tzr_ld4(V + b * vs + 4 * lane) : tzr_zero4();
  const float4 g = cok ? tzr_ld4(G + b * gs + 4 * lane) : tzr_zero4();
  float4 x[LA_MAXK];
  float wk[LA_MAXK], t[LA_MAXK];
  bool valid[LA_MAXK];
  float tw = 0.f;
#pragma unroll
  for (int k = 0; k < LA_MAXK; ++k) {
    valid[k] = k < K && mask[b * K + k] != 0;
    x[k] = cok && valid[k] ? tzr_ld4(I + (b * K + k) * is + 4 * lane) : tzr_zero4();
    wk[k] = valid[k] ? w[b * K + k] : 0.f;
    t[k] = tzr_wave_sum(la_dot4(g, x[k]));
    tw = fmaf(wk[k], t[k], tw);
  }
  float4 dv = tzr_zero4();
#pragma unroll
  for (int k = 0; k < LA_MAXK; ++k) {
    const float da = simi_pow * wk[k] * (t[k] - tw);
    dv = tzr_fma4(da, x[k], dv);
    if (cok && k < K) {
      const float4 d = tzr_fma4(da, v, make_float4(wk[k] * g.x, wk[k] * g.y, wk[k] * g.z, wk[k] * g.w));
      tzr_st4(dI + (b * K + k) * dis + 4 * lane, valid[k] ? d : tzr_zero4());
    }
  }
  if (cok) tzr_st4(dV + b * dvs + 4 * lane, dv);
}

static int la_check(const float* d_i, int64_t i_stride, const float* d_v, int64_t v_stride, const void* d_mask, int64_t B, int K, int D, float simi_pow) {
  if (B < 0) return TZR_ERR_INVALID;
  if (D < 4 || (D & 3) || D > LA_MAXD || K < 1 || K > LA_MAXK || !(simi_pow > 0.f) || B >= (1ll << 31)) return TZR_ERR_UNSUPPORTED;
  TZR_TRY(tzr_rows_operand(reinterpret_cast<uint64_t>(d_i), i_stride, D));
  TZR_TRY(tzr_rows_operand(reinterpret_cast<uint64_t>(d_v), v_stride, D));
  return d_mask ? TZR_OK : TZR_ERR_INVALID;
}

extern "C" int tzr_label_attn_fwd(const float* d_i, int64_t i_stride, const float* d_v, int64_t v_stride, const uint8_t* d_mask, int64_t B, int K, int D,
                                  float simi_pow, float* d_out, int64_t out_stride, float* d_w, void* stream) {
  TZR_TRY(la_check(d_i, i_stride, d_v, v_stride, d_mask, B, K, D, simi_pow));
  TZR_TRY(tzr_rows_operand(reinterpret_cast<uint64_t>(d_out), out_stride, D));
  if (!d_w || (reinterpret_cast<uint64_t>(d_w) & 3)) return TZR_ERR_INVALID;
  if (B == 0) return TZR_OK;
  hipLaunchKernelGGL(tzr_label_attn_fwd_kernel, dim3((unsigned)((B + LA_WAVES - 1) / LA_WAVES)), dim3(LA_THREADS), 0, static_cast<hipStream_t>(stream), d_i,
                     i_stride, d_v, v_stride, d_mask, B, K, D, simi_pow, d_out, out_stride, d_w);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_label_attn_bwd(const float* d_grad_out, int64_t grad_out_stride, const float* d_i, int64_t i_stride, const float* d_v, int64_t v_stride,
                                  const float* d_w, const uint8_t* d_mask, int64_t B, int K, int D, float simi_pow, float* d_di, int64_t di_stride,
                                  float* d_dv, int64_t dv_stride, void* stream) {
  TZR_TRY(la_check(d_i, i_stride, d_v, v_stride, d_mask, B, K, D, simi_pow));
  TZR_TRY(tzr_rows_operand(reinterpret_cast<uint64_t>(d_grad_out), grad_out_stride, D));
  TZR_TRY(tzr_rows_operand(reinterpret_cast<uint64_t>(d_di), di_stride, D));
  TZR_TRY(tzr_rows_operand(reinterpret_cast<uint64_t>(d_dv), dv_stride, D));
  if (!d_w || (reinterpret_cast<uint64_t>(d_w) & 3)) return TZR_ERR_INVALID;
  if (B == 0) return TZR_OK;
  hipLaunchKernelGGL(tzr_label_attn_bwd_kernel, dim3((unsigned)((B + LA_WAVES - 1) / LA_WAVES)), dim3(LA_THREADS), 0, static_cast<hipStream_t>(stream),
                     d_grad_out, grad_out_stride, d_i, i_stride, d_v, v_stride, d_w, d_mask, B, K, D, simi_pow, d_di, di_stride, d_dv, dv_stride);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
