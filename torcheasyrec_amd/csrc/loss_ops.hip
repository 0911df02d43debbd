// The losses a pipeline config names (tzrec/protos/loss.proto:44-63), each as loss + d(loss)/d(logits) from two or three
// launches instead of the 10-20 elementwise launches torch issues for one (what tzr_bce_logits, dense_ops.hip, did for
// plain BCE), with the reference's sample weights (tzrec/models/rank_model.py:264-287, multi_task_rank.py:97-142) inside:
//
//   tzr_loss_pointwise   [B] logits: binary cross entropy with label smoothing, binary focal loss (the focal weight is
//                        a constant of the gradient, as the reference detaches it), L2 -- tzr_bce_logits_kernel's tiling
//   tzr_softmax_ce       [B, C] logits, label smoothing; one lane per row up to C = 8, one wave per row beyond; a label
//                        outside [0, C) is counted, never used as an index.  A class masked out by -inf (not the
//                        label's own) has probability and gradient 0; the smoothing term u (C lse - sum x) is +inf
//                        then, as torch's is, and is not formed at all when label_smoothing == 0 (0 * inf)
//   tzr_jrc_loss         JRC (tzrec/loss/jrc_loss.py) grouped by session: O(B) memory where the reference builds [B, B]
//                        masks (17 GB each at B = 65536).  A batch with no positive or no negative row makes the
//                        reference's mean form NaN (mean of an empty tensor times 0); here it is the finite sum.
//
// Row weight w_i = weight_i * (space_label_i > 0 ? in_w : out_w); loss = task_weight * sum(w l) / sum(w) (0 when the
// weights sum to 0); the gradient is written WITHOUT the normaliser and `scale = task_weight / sum(w)` next to it, so that
// nothing is normalised in a pre-pass and the autograd backward is one multiply.  sum(w l) and sum(w) are two partials per
// workgroup, finished in index order by one workgroup: no float atomics, same inputs -> same bits.  No host sync.
#include "tzr_common.h"

#define LS_THREADS 256
#define LS_ITEMS 4  // rows per thread
#define LS_WAVES (LS_THREADS / TZR_WAVE)
#define LS_MAX_PARTS 4096
#define LS_SMALL_C 8

struct LsLabel {
  const void* p;
  int type;  // 0 float32, 1 int32, 2 int64
};
__device__ __forceinline__ float ls_label_f(LsLabel l, int64_t i) {
  if (l.type == 0) return static_cast<const float*>(l.p)[i];
  if (l.type == 1) return (float)static_cast<const int32_t*>(l.p)[i];
  return (float)static_cast<const int64_t*>(l.p)[i];
}
__device__ __forceinline__ int64_t ls_label_i(LsLabel l, int64_t i) {
  if (l.type == 1) return static_cast<const int32_t*>(l.p)[i];
  return static_cast<const int64_t*>(l.p)[i];
}

struct LsWeights {
  const float* weight;
  LsLabel space;
  float in_w, out_w;
};
__device__ __forceinline__ float ls_row_weight(const LsWeights& W, int64_t i) {
  float w = W.weight ? W.weight[i] : 1.0f;
  if (W.space.p) w *= ls_label_f(W.space, i) > 0.f ? W.in_w : W.out_w;
  return w;
}

// the workgroup's (sum w l, sum w) in tzr_bce_logits_kernel's fixed tree -> parts[2 wg], parts[2 wg + 1]
__device__ __forceinline__ void ls_block_sum2(float a, float b, float* sa, float* sb, float* __restrict__ parts) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) {
    a += __shfl_down(a, d, TZR_WAVE);
    b += __shfl_down(b, d, TZR_WAVE);
  }
  if (lane == 0) { sa[wv] = a; sb[wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float va = 0.f, vb = 0.f;
    for (int i = 0; i < LS_WAVES; ++i) { va += sa[i]; vb += sb[i]; }
    parts[2 * blockIdx.x] = va;
    parts[2 * blockIdx.x + 1] = vb;
  }
}

__device__ __forceinline__ float ls_softplus(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float ls_sigmoid(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

template <int KIND>
__global__ __launch_bounds__(LS_THREADS) void tzr_loss_pointwise_kernel(
    const float* __restrict__ logits, LsLabel labels, LsWeights W, float p0, float p1, int64_t B, int64_t per_wg,
    float* __restrict__ parts, float* __restrict__ grad) {
  __shared__ float sa[LS_WAVES], sb[LS_WAVES];
  float acc = 0.f, accw = 0.f;
  const int64_t lo = (int64_t)blockIdx.x * per_wg;
  const int64_t hi = min(B, lo + per_wg);
  for (int64_t base = lo; base < hi; base += LS_THREADS * LS_ITEMS) {
    float x[LS_ITEMS], y[LS_ITEMS], w[LS_ITEMS];
#pragma unroll
    for (int j = 0; j < LS_ITEMS; ++j) {  // independent loads first
      const int64_t i = base + (int64_t)j * LS_THREADS + threadIdx.x;
      const bool ok = i < hi;
      x[j] = ok ? logits[i] : 0.f;
      y[j] = ok ? ls_label_f(labels, i) : 0.f;
      w[j] = ok ? ls_row_weight(W, i) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < LS_ITEMS; ++j) {
      const int64_t i = base + (int64_t)j * LS_THREADS + threadIdx.x;
      if (i >= hi) continue;
      float l, g;
      if (KIND == TZR_LOSS_L2) {
        const float d = x[j] - y[j];
        l = d * d;
        g = 2.0f * d;
      } else {
        // bce = max(x,0) - x*y + log1p(exp(-|x|));  d/dx = sigmoid(x) - y
        const float e = expf(-fabsf(x[j]));
        const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
        const float p = x[j] >= 0.f ? big : small;    // sigmoid(x)
        const float omp = x[j] >= 0.f ? small : big;  // 1 - sigmoid(x), without the cancellation
        const float yy = KIND == TZR_LOSS_BCE ? y[j] * (1.0f - p0) + 0.5f * p0 : y[j];
        l = fmaf(-x[j], yy, fmaxf(x[j], 0.f)) + log1pf(e);  // (one rounding: x - x y' cancels for a smoothed label and a large logit)
        g = p - yy;
        if (KIND == TZR_LOSS_FOCAL) {
          const float f = p1 * yy * powf(omp, p0) + (1.0f - p1) * (1.0f - yy) * powf(p, p0);
          l *= f;
          g *= f;
        }
      }
      acc += w[j] * l;
      accw += w[j];
      grad[i] = w[j] * g;
    }
  }
  ls_block_sum2(acc, accw, sa, sb, parts);
}

// sum(w l), sum(w) of row losses that an earlier launch left in rowloss[B]
__global__ __launch_bounds__(LS_THREADS) void tzr_loss_rows_kernel(const float* __restrict__ rowloss, LsWeights W, int64_t B,
                                                                   int64_t per_wg, float* __restrict__ parts) {
  __shared__ float sa[LS_WAVES], sb[LS_WAVES];
  float acc = 0.f, accw = 0.f;
  const int64_t lo = (int64_t)blockIdx.x * per_wg;
  const int64_t hi = min(B, lo + per_wg);
  for (int64_t base = lo; base < hi; base += LS_THREADS * LS_ITEMS) {
    float l[LS_ITEMS], w[LS_ITEMS];
#pragma unroll
    for (int j = 0; j < LS_ITEMS; ++j) {
      const int64_t i = base + (int64_t)j * LS_THREADS + threadIdx.x;
      const bool ok = i < hi;
      l[j] = ok ? rowloss[i] : 0.f;
      w[j] = ok ? ls_row_weight(W, i) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < LS_ITEMS; ++j) {
      acc += w[j] * l[j];
      accw += w[j];
    }
  }
  ls_block_sum2(acc, accw, sa, sb, parts);
}

__global__ __launch_bounds__(LS_THREADS) void tzr_loss_finish_kernel(const float* __restrict__ parts, int n, int has_w, float rows,
                                                                      float task_weight, float* __restrict__ loss,
                                                                      float* __restrict__ scale) {
  __shared__ float sa[LS_WAVES], sb[LS_WAVES];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < n; i += LS_THREADS) {
    a += parts[2 * i];
    b += parts[2 * i + 1];
  }
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) {
    a += __shfl_down(a, d, TZR_WAVE);
    b += __shfl_down(b, d, TZR_WAVE);
  }
  if (lane == 0) { sa[wv] = a; sb[wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float va = 0.f, vb = 0.f;
    for (int i = 0; i < LS_WAVES; ++i) { va += sa[i]; vb += sb[i]; }
    const float sw = has_w ? vb : rows;
    const bool ok = sw != 0.f;  // div_no_nan
    *loss = ok ? task_weight * (va / sw) : 0.f;
    *scale = ok ? task_weight / sw : 0.f;
  }
}

// ---- softmax cross entropy -------------------------------------------------------------------------------------------
// one lane per row, the row in registers (C <= LS_SMALL_C)
__global__ __launch_bounds__(LS_THREADS) void tzr_softmax_ce_small_kernel(
    const float* __restrict__ logits, int64_t row_stride, int C, LsLabel labels, float eps, LsWeights W, int64_t B,
    float* __restrict__ rowloss, float* __restrict__ grad, int64_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (i >= B) return;
  float x[LS_SMALL_C];
#pragma unroll
  for (int c = 0; c < LS_SMALL_C; ++c) x[c] = c < C ? logits[i * row_stride + c] : -INFINITY;
  const int64_t y = ls_label_i(labels, i);
  const float w = ls_row_weight(W, i);
  if (y < 0 || y >= C) {
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
    rowloss[i] = 0.f;
    for (int c = 0; c < C; ++c) grad[i * C + c] = 0.f;
    return;
  }
  float m = x[0];
#pragma unroll
  for (int c = 1; c < LS_SMALL_C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f, sx = 0.f, xy = 0.f;
#pragma unroll
  for (int c = 0; c < LS_SMALL_C; ++c) {
    if (c < C) {
      s += expf(x[c] - m);
      sx += x[c];
      if (c == (int)y) xy = x[c];
    }
  }
  // lse = m + ls is formed for the smoothing term alone: lse - x = (m - x) + ls keeps the rounding at the size of the difference,
  // not of lse (logits of scale 120: an ulp of lse is 3e-5, and so was the relative error of exp(x - lse))
  const float ls = logf(s), lse = m + ls;
  const float u = eps / (float)C;
  const float ce = (1.0f - eps) * ((m - xy) + ls);
  rowloss[i] = eps > 0.f ? ce + u * ((float)C * lse - sx) : ce;  // (uniform: 0 * (sx = -inf) would be NaN)
#pragma unroll
  for (int c = 0; c < LS_SMALL_C; ++c)
    if (c < C) grad[i * C + c] = w * (expf((x[c] - m) - ls) - ((c == (int)y ? 1.0f - eps : 0.f) + u));
}

// one wave per row, lanes stride over the classes
__global__ __launch_bounds__(LS_THREADS) void tzr_softmax_ce_wave_kernel(
    const float* __restrict__ logits, int64_t row_stride, int C, LsLabel labels, float eps, LsWeights W, int64_t B,
    float* __restrict__ rowloss, float* __restrict__ grad, int64_t* __restrict__ bad) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int64_t i = (int64_t)blockIdx.x * LS_WAVES + threadIdx.x / TZR_WAVE;
  if (i >= B) return;  // (the whole wave)
  const float* __restrict__ x = logits + i * row_stride;
  const int64_t y = ls_label_i(labels, i);
  const float w = ls_row_weight(W, i);
  if (y < 0 || y >= C) {
    if (lane == 0) {
      if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
      rowloss[i] = 0.f;
    }
    for (int c = lane; c < C; c += TZR_WAVE) grad[i * C + c] = 0.f;
    return;
  }
  float m = -INFINITY;
  for (int c = lane; c < C; c += TZR_WAVE) m = fmaxf(m, x[c]);
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, TZR_WAVE));
  float s = 0.f, sx = 0.f;
  for (int c = lane; c < C; c += TZR_WAVE) {
    s += expf(x[c] - m);
    sx += x[c];
  }
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) {
    s += __shfl_down(s, d, TZR_WAVE);
    sx += __shfl_down(sx, d, TZR_WAVE);
  }
  s = __shfl(s, 0, TZR_WAVE);
  sx = __shfl(sx, 0, TZR_WAVE);
  const float ls = logf(s), lse = m + ls;  // (as in the small kernel)
  const float u = eps / (float)C;
  if (lane == 0) {
    const float ce = (1.0f - eps) * ((m - x[y]) + ls);
    rowloss[i] = eps > 0.f ? ce + u * ((float)C * lse - sx) : ce;  // (uniform, as in the small kernel)
  }
  for (int c = lane; c < C; c += TZR_WAVE)
    grad[i * C + c] = w * (expf((x[c] - m) - ls) - ((c == (int)y ? 1.0f - eps : 0.f) + u));
}

// ---- JRC -------------------------------------------------------------------------------------------------------------
// running logsumexp as (max, sum of exp(. - max)); the empty set is (-inf, 0)
__device__ __forceinline__ void ls_lse_add(float& m, float& s, float v) {
  if (v > m) {
    s = s * expf(m - v) + 1.0f;
    m = v;
  } else {
    s += expf(v - m);
  }
}
__device__ __forceinline__ void ls_lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  s = nm == -INFINITY ? 0.f : s * expf(m - nm) + os * expf(om - nm);
  m = nm;
}
// the wave's (max, sum of exp(. - max)), the same bits in every lane
__device__ __forceinline__ void ls_lse_wave(float& m, float& s) {
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) {
    const float om = __shfl_down(m, d, TZR_WAVE), os = __shfl_down(s, d, TZR_WAVE);
    ls_lse_merge(m, s, om, os);
  }
  m = __shfl(m, 0, TZR_WAVE);
  s = __shfl(s, 0, TZR_WAVE);
}
__device__ __forceinline__ float ls_sum_wave(float v) {
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, TZR_WAVE);
  return __shfl(v, 0, TZR_WAVE);
}

__global__ __launch_bounds__(LS_THREADS) void tzr_jrc_kernel(
    const float* __restrict__ logits, LsLabel labels, const int64_t* __restrict__ sid, const int64_t* __restrict__ order,
    LsWeights W, float alpha, int64_t B, float* __restrict__ rowloss, float* __restrict__ grad) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int64_t c0 = ((int64_t)blockIdx.x * LS_WAVES + threadIdx.x / TZR_WAVE) * TZR_WAVE;  // the wave's sorted rows [c0, c0 + 64)
  if (c0 >= B) return;  // (the whole wave)
  const int64_t p = c0 + lane;
  bool head = false;
  if (p < B) head = p == 0 || sid[order[p - 1]] != sid[order[p]];
  unsigned long long heads = __ballot(head);
  const float beta = 1.0f - alpha;
  while (heads) {  // (uniform over the wave)
    const int64_t h = c0 + (__ffsll(heads) - 1);
    heads &= heads - 1;
    int64_t e;
    if (heads) {
      e = c0 + (__ffsll(heads) - 1);
    } else {  // the session runs past the wave's rows, or to the end: the first sorted row with a larger id
      const int64_t key = sid[order[h]];
      int64_t lo = min(c0 + TZR_WAVE, B), hi = B;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sid[order[mid]] <= key) lo = mid + 1; else hi = mid;
      }
      e = lo;
    }
    // sweep 1: A = logsumexp of l1 over the negatives, Bs = logsumexp of l0 over the positives
    float mA = -INFINITY, sA = 0.f, mB = -INFINITY, sB = 0.f;
    for (int64_t q = h + lane; q < e; q += TZR_WAVE) {
      const int64_t i = order[q];
      const float2 l = *reinterpret_cast<const float2*>(logits + 2 * i);
      if (ls_label_f(labels, i) == 1.0f) ls_lse_add(mB, sB, l.x); else ls_lse_add(mA, sA, l.y);
    }
    ls_lse_wave(mA, sA);
    ls_lse_wave(mB, sB);
    // A = mA + lA, Bs = mB + lB are never formed: A - l1 = (mA - l1) + lA keeps the rounding at the size of the difference, not
    // of A (logits of scale 8: |A| ~ 20, an ulp of 2e-6 in the exponent), and exp(l1 - A) = exp(l1 - mA) / sA
    const float lA = sA > 0.f ? logf(sA) : -INFINITY, lB = sB > 0.f ? logf(sB) : -INFINITY;
    // sweep 2: the row losses, P = sum over positives of w q, Q = sum over negatives of w r
    float P = 0.f, Q = 0.f;
    for (int64_t q = h + lane; q < e; q += TZR_WAVE) {
      const int64_t i = order[q];
      const float2 l = *reinterpret_cast<const float2*>(logits + 2 * i);
      const bool pos = ls_label_f(labels, i) == 1.0f;
      const float w = ls_row_weight(W, i);
      const float ce = fmaxf(l.x, l.y) + log1pf(expf(-fabsf(l.x - l.y))) - (pos ? l.y : l.x);
      const float z = pos ? (mA - l.y) + lA : (mB - l.x) + lB;
      rowloss[i] = alpha * ce + beta * ls_softplus(z);
      if (pos) P += w * ls_sigmoid(z); else Q += w * ls_sigmoid(z);
    }
    P = ls_sum_wave(P);
    Q = ls_sum_wave(Q);
    // sweep 3: the gradients, both elements of a row from the lane that holds it
    for (int64_t q = h + lane; q < e; q += TZR_WAVE) {
      const int64_t i = order[q];
      const float2 l = *reinterpret_cast<const float2*>(logits + 2 * i);
      const bool pos = ls_label_f(labels, i) == 1.0f;
      const float w = ls_row_weight(W, i);
      const float p1 = ls_sigmoid(l.y - l.x), p0 = ls_sigmoid(l.x - l.y);
      float2 g;
      g.x = alpha * w * (p0 - (pos ? 0.f : 1.0f));
      g.y = alpha * w * (p1 - (pos ? 1.0f : 0.f));
      if (pos) {
        g.y -= beta * w * ls_sigmoid((mA - l.y) + lA);
        g.x += beta * Q * (expf(l.x - mB) / sB);  // (sB >= 1: this row is one of its terms)
      } else {
        g.x -= beta * w * ls_sigmoid((mB - l.x) + lB);
        g.y += beta * P * (expf(l.y - mA) / sA);
      }
      *reinterpret_cast<float2*>(grad + 2 * i) = g;
    }
  }
}

// ---- entry points ----------------------------------------------------------------------------------------------------
static inline int ls_label_type(int itemsize, int is_float) {
  if (is_float && itemsize == 4) return 0;
  if (!is_float && itemsize == 4) return 1;
  if (!is_float && itemsize == 8) return 2;
  return -1;
}

static inline size_t ls_parts_bytes() { return tzr_align_up((size_t)2 * LS_MAX_PARTS * sizeof(float)); }

// tzr_bce_logits' partition: a tile per workgroup, several above LS_MAX_PARTS tiles
static inline void ls_partition(int64_t B, int64_t* n_wg, int64_t* per_wg) {
  const int64_t tile = LS_THREADS * LS_ITEMS;
  *n_wg = (B + tile - 1) / tile;
  *per_wg = tile;
  if (*n_wg > LS_MAX_PARTS) {
    *per_wg = ((B + LS_MAX_PARTS - 1) / LS_MAX_PARTS + tile - 1) / tile * tile;
    *n_wg = (B + *per_wg - 1) / *per_wg;
  }
}

static void ls_rows_and_finish(const float* rowloss, const LsWeights& W, float task_weight, int64_t B, float* parts, float* d_loss,
                               float* d_scale, hipStream_t s) {
  int64_t n_wg, per_wg;
  ls_partition(B, &n_wg, &per_wg);
  hipLaunchKernelGGL(tzr_loss_rows_kernel, dim3((unsigned)n_wg), dim3(LS_THREADS), 0, s, rowloss, W, B, per_wg, parts);
  hipLaunchKernelGGL(tzr_loss_finish_kernel, dim3(1), dim3(LS_THREADS), 0, s, parts, (int)n_wg,
                     (W.weight || W.space.p) ? 1 : 0, (float)B, task_weight, d_loss, d_scale);
}

extern "C" size_t tzr_loss_pointwise_workspace(int64_t B) {
  (void)B;
  return ls_parts_bytes();
}

extern "C" int tzr_loss_pointwise(int kind, float p0, float p1, const float* d_logits, const void* d_labels, int labels_itemsize,
                                  int labels_are_float, const float* d_weight, const void* d_space_label, int space_itemsize,
                                  int space_is_float, float in_w, float out_w, float task_weight, int64_t B, float* d_loss,
                                  float* d_grad, float* d_scale, void* ws, size_t ws_bytes, void* stream) {
  if (!d_logits || !d_labels || !d_loss || !d_grad || !d_scale || B <= 0) return TZR_ERR_INVALID;
  if (kind != TZR_LOSS_BCE && kind != TZR_LOSS_FOCAL && kind != TZR_LOSS_L2) return TZR_ERR_INVALID;
  const int lt = ls_label_type(labels_itemsize, labels_are_float);
  const int st = d_space_label ? ls_label_type(space_itemsize, space_is_float) : 0;
  if (lt < 0 || st < 0) return TZR_ERR_UNSUPPORTED;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < tzr_loss_pointwise_workspace(B)) return TZR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* parts = static_cast<float*>(ws);
  const LsLabel labels{d_labels, lt};
  const LsWeights W{d_weight, LsLabel{d_space_label, st}, in_w, out_w};
  int64_t n_wg, per_wg;
  ls_partition(B, &n_wg, &per_wg);
#define TZR_LOSS_LAUNCH(K)                                                                                              \
  hipLaunchKernelGGL(tzr_loss_pointwise_kernel<K>, dim3((unsigned)n_wg), dim3(LS_THREADS), 0, s, d_logits, labels, W, p0, \
                     p1, B, per_wg, parts, d_grad)
  if (kind == TZR_LOSS_BCE) TZR_LOSS_LAUNCH(TZR_LOSS_BCE);
  else if (kind == TZR_LOSS_FOCAL) TZR_LOSS_LAUNCH(TZR_LOSS_FOCAL);
  else TZR_LOSS_LAUNCH(TZR_LOSS_L2);
#undef TZR_LOSS_LAUNCH
  hipLaunchKernelGGL(tzr_loss_finish_kernel, dim3(1), dim3(LS_THREADS), 0, s, parts, (int)n_wg,
                     (d_weight || d_space_label) ? 1 : 0, (float)B, task_weight, d_loss, d_scale);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

static inline size_t ls_rows_workspace(int64_t B) {
  return ls_parts_bytes() + tzr_align_up((size_t)(B > 0 ? B : 0) * sizeof(float));
}

extern "C" size_t tzr_softmax_ce_workspace(int64_t B, int C) {
  (void)C;
  return ls_rows_workspace(B);
}

extern "C" int tzr_softmax_ce(const float* d_logits, int64_t row_stride, int C, const void* d_labels, int labels_itemsize,
                              int labels_are_float, float eps, const float* d_weight, const void* d_space_label,
                              int space_itemsize, int space_is_float, float in_w, float out_w, float task_weight, int64_t B,
                              float* d_loss, float* d_grad, float* d_scale, int64_t* d_bad_labels, void* ws, size_t ws_bytes,
                              void* stream) {
  if (!d_logits || !d_labels || !d_loss || !d_grad || !d_scale || B <= 0 || C < 2 || row_stride < C) return TZR_ERR_INVALID;
  const int lt = ls_label_type(labels_itemsize, labels_are_float);
  const int st = d_space_label ? ls_label_type(space_itemsize, space_is_float) : 0;
  if (lt <= 0 || st < 0 || B >= ((int64_t)1 << 30)) return TZR_ERR_UNSUPPORTED;  // (class labels are integers)
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < tzr_softmax_ce_workspace(B, C)) return TZR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TzrCarver carve(ws);
  float* parts = carve.take<float>((size_t)2 * LS_MAX_PARTS);
  float* rowloss = carve.take<float>((size_t)B);
  const LsLabel labels{d_labels, lt};
  const LsWeights W{d_weight, LsLabel{d_space_label, st}, in_w, out_w};
  if (C <= LS_SMALL_C)
    hipLaunchKernelGGL(tzr_softmax_ce_small_kernel, dim3((unsigned)((B + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, s,
                       d_logits, row_stride, C, labels, eps, W, B, rowloss, d_grad, d_bad_labels);
  else
    hipLaunchKernelGGL(tzr_softmax_ce_wave_kernel, dim3((unsigned)((B + LS_WAVES - 1) / LS_WAVES)), dim3(LS_THREADS), 0, s,
                       d_logits, row_stride, C, labels, eps, W, B, rowloss, d_grad, d_bad_labels);
  ls_rows_and_finish(rowloss, W, task_weight, B, parts, d_loss, d_scale, s);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" size_t tzr_jrc_loss_workspace(int64_t B) { return ls_rows_workspace(B); }

extern "C" int tzr_jrc_loss(const float* d_logits, const void* d_labels, int labels_itemsize, int labels_are_float,
                            const int64_t* d_session, const int64_t* d_order, float alpha, const float* d_weight,
                            const void* d_space_label, int space_itemsize, int space_is_float, float in_w, float out_w,
                            float task_weight, int64_t B, float* d_loss, float* d_grad, float* d_scale, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!d_logits || !d_labels || !d_session || !d_order || !d_loss || !d_grad || !d_scale || B <= 0) return TZR_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(d_logits) & 7 || reinterpret_cast<uintptr_t>(d_grad) & 7) return TZR_ERR_INVALID;  // (float2 rows)
  const int lt = ls_label_type(labels_itemsize, labels_are_float);
  const int st = d_space_label ? ls_label_type(space_itemsize, space_is_float) : 0;
  if (lt < 0 || st < 0 || B >= ((int64_t)1 << 30)) return TZR_ERR_UNSUPPORTED;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) || ws_bytes < tzr_jrc_loss_workspace(B)) return TZR_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TzrCarver carve(ws);
  float* parts = carve.take<float>((size_t)2 * LS_MAX_PARTS);
  float* rowloss = carve.take<float>((size_t)B);
  const LsLabel labels{d_labels, lt};
  const LsWeights W{d_weight, LsLabel{d_space_label, st}, in_w, out_w};
  hipLaunchKernelGGL(tzr_jrc_kernel, dim3((unsigned)((B + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, s, d_logits, labels,
                     d_session, d_order, W, alpha, B, rowloss, d_grad);
  ls_rows_and_finish(rowloss, W, task_weight, B, parts, d_loss, d_scale, s);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
