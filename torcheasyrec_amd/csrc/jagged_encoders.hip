// The two cheap sequence encoders of a DEEP group's `sequence_encoders`, over JAGGED positions: simple (dot-product) attention and
// sum / mean pooling.  Replaces SimpleAttention.forward and PoolingEncoder.forward of the reference on padded [B, L, D] tensors
// (tzrec/modules/sequence.py:131-218).  Conventions of din_attention.hip: a position is a ROW of the unpooled lookup's output
// [N, D]; sample b owns rows [offsets[b], offsets[b + 1]); positions at index >= max_len inside a sample do not exist for the
// encoder (the padded length / `max_seq_length`); nothing is padded.
//
//   tzr_jagged_dot_attn_fwd   s_n = k_n . q_b;  p = softmax of s over sample b's positions;  out_b = sum_n p_n k_n;  p -> [N]
//   tzr_jagged_dot_attn_bwd   t_n = g_b . k_n;  ds_n = p_n (t_n - sum_m p_m t_m);  dk_n = p_n g_b + ds_n q_b;  dq_b = sum_n ds_n k_n
//   tzr_jagged_pool_fwd       out_b = sum of the first min(len, max_len) rows (mean: / max(min(len, max_len), 1))
//   tzr_jagged_pool_bwd       dk_n = g_b (mean: / the same count); zero rows for the positions at or behind max_len
//
// Masking semantics of the reference, restated for rows (as din_attention.hip): a padding position's score is -(2^31 - 1), its
// exp() 0 exactly, so the softmax of a sample with >= 1 position is the softmax over its positions; a sample with NO position
// gets a uniform softmax over zero rows: out_b = 0, dq_b = 0.
//
// One wave per sample, the wave cut into G = 64 / P groups of P lanes (P = D / 4 rounded up to a power of two): group g takes
// positions g, g + G, ..., lane c of a group the float4 piece c of the row.  Every sum over a sample's positions has a fixed
// order, a function of the lengths and D alone: no atomics, two runs are bit-equal.
//
// The rows are read from HBM ONCE per kernel where a wave can hold them: a lane keeps the JE_HOLD pieces it loaded for the
// scores in registers and forms the weighted sum (the backward: dq) from them -- JE_HOLD * G positions, 64 at D = 48, 256 at
// D = 16, 16 at D = 256.  A longer sample's second pass reads its rows again.
#include "tzr_common.h"

#define JE_THREADS 256
#define JE_WAVES (JE_THREADS / TZR_WAVE)
#define JE_MAXLEN 2048  // positions of one sample whose scores a wave keeps in LDS (DA_MAXLEN of din_attention.hip)
#define JE_MAXDIM (4 * TZR_WAVE)  // one lane per float4 piece of a row
#define JE_HOLD 16  // float4 pieces of rows a lane keeps between the two passes over a sample

__device__ __forceinline__ float je_group_sum(float v, int P) {  // over the P lanes of a group (fixed tree)
  for (int m = P >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float4 je_across_groups(float4 a, int P) {  // same piece of every group, added by a fixed tree
  for (int m = P; m < TZR_WAVE; m <<= 1) {
    a.x += __shfl_xor(a.x, m); a.y += __shfl_xor(a.y, m); a.z += __shfl_xor(a.z, m); a.w += __shfl_xor(a.w, m);
  }
  return a;
}
__device__ __forceinline__ float je_dot4(float4 a, float4 b) {
  float d = a.x * b.x;
  d = fmaf(a.y, b.y, d); d = fmaf(a.z, b.z, d); d = fmaf(a.w, b.w, d);
  return d;
}

// sc[i] = row_i . v for the positions [s, s + len) of one sample (v: this lane's piece of the vector, zero in the lanes
// behind the row's last piece).  JE_HOLD * G positions per pass, their loads in flight together (a position behind the
// sample's last re-reads the last: no load sits inside a divergent branch).  After the call r[u] is row u * G + g of the
// LAST pass: all of the sample's rows when len <= JE_HOLD * G.
__device__ __forceinline__ void je_row_dots(const float* __restrict__ rows, int64_t stride, int64_t s, int len, int P, int G, int g,
                                            int c, int cl, float4 v, float* sc, float4 (&r)[JE_HOLD]) {
  for (int i0 = 0; i0 < len; i0 += JE_HOLD * G) {
#pragma unroll
    for (int u = 0; u < JE_HOLD; ++u)
      if (i0 + u * G < len) {  // (wave-uniform)
        const int i = i0 + u * G + g;
        r[u] = tzr_ld4(rows + (s + (i < len ? i : len - 1)) * stride + 4 * cl);
      }
#pragma unroll
    for (int u = 0; u < JE_HOLD; ++u)
      if (i0 + u * G < len) {
        const int i = i0 + u * G + g;
        const float d = je_group_sum(je_dot4(r[u], v), P);
        if (i < len && c == 0) sc[i] = d;
      }
  }
}

__global__ __launch_bounds__(JE_THREADS) void tzr_jagged_dot_attn_fwd_kernel(
    const float* __restrict__ kv, int64_t kvs, const float* __restrict__ q, int64_t qs, int lg, int P,
    const int64_t* __restrict__ offsets, int64_t B, int64_t max_len, float* __restrict__ out, int64_t outs, float* __restrict__ p) {
  __shared__ float scs[JE_WAVES][JE_MAXLEN];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  float* sc = scs[wv];
  const int G = TZR_WAVE / P, g = lane / P, c = lane & (P - 1);
  const bool on = c < lg;  // (P > lg: the lanes behind the row's last piece read piece 0 and add zeros)
  const int cl = on ? c : 0;
  for (int64_t b = (int64_t)blockIdx.x * JE_WAVES + wv; b < B; b += (int64_t)gridDim.x * JE_WAVES) {
    const int64_t s = offsets[b], e = offsets[b + 1];
    const int len = (int)min(e - s, max_len);
    // positions behind max_len do not exist for the encoder: probability 0
    for (int64_t n = s + len + lane; n < e; n += TZR_WAVE) p[n] = 0.f;
    const float4 qq = on ? tzr_ld4(q + b * qs + 4 * c) : tzr_zero4();
    float4 r[JE_HOLD];
    je_row_dots(kv, kvs, s, len, P, G, g, c, cl, qq, sc, r);
    __builtin_amdgcn_wave_barrier();
    float mx = -3.402823466e38f;
    for (int i = lane; i < len; i += TZR_WAVE) mx = fmaxf(mx, sc[i]);
    mx = tzr_wave_max(mx);
    float sum = 0.f;
    for (int i = lane; i < len; i += TZR_WAVE) {
      const float ex = expf(sc[i] - mx);
      sc[i] = ex;
      sum += ex;
    }
    sum = tzr_wave_sum(sum);  // (fixed tree)
    const float inv = len > 0 ? 1.0f / sum : 0.f;
    for (int i = lane; i < len; i += TZR_WAVE) {
      const float pi = sc[i] * inv;
      sc[i] = pi;
      p[s + i] = pi;
    }
    __builtin_amdgcn_wave_barrier();
    // out_b = sum_i p_i k_i: a group adds its positions in order, the groups are added by a fixed tree
    float4 a = tzr_zero4();
    if (len <= JE_HOLD * G) {  // the rows this wave still holds
#pragma unroll
      for (int u = 0; u < JE_HOLD; ++u)
        if (u * G < len) {
          const int i = u * G + g;
          if (i < len) a = tzr_fma4(sc[i], r[u], a);
        }
    } else {
      for (int i0 = g; i0 < len; i0 += 4 * G) {  // four of the group's positions per pass, loads together
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * G;
          x[u] = tzr_ld4(kv + (s + (i < len ? i : len - 1)) * kvs + 4 * cl);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i0 + u * G < len) a = tzr_fma4(sc[i0 + u * G], x[u], a);
      }
    }
    a = je_across_groups(a, P);
    if (g == 0 && on) tzr_st4(out + b * outs + 4 * c, a);
    __builtin_amdgcn_wave_barrier();  // (the next sample overwrites sc)
  }
}

static int je_group_lanes(int D) {  // P: D / 4 rounded up to a power of two (<= 64)
  int P = 1;
  while (P < (D >> 2)) P <<= 1;
  return P;
}

static bool je_misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

extern "C" int tzr_jagged_dot_attn_fwd(const float* d_kv, int64_t kv_stride, const float* d_q, int64_t q_stride, int D,
                                       const int64_t* d_offsets, int64_t B, int64_t N, int64_t max_len, float* d_out,
                                       int64_t out_stride, float* d_p, void* stream) {
  if (B < 0 || N < 0 || D <= 0 || max_len < 0) return TZR_ERR_INVALID;
  if ((D & 3) || D > JE_MAXDIM || ((kv_stride | q_stride | out_stride) & 3) || kv_stride < D || q_stride < D || out_stride < D ||
      max_len > JE_MAXLEN)
    return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_offsets || !d_q || !d_out || (N > 0 && (!d_kv || !d_p)) || je_misaligned(d_kv, d_q, d_out)) return TZR_ERR_INVALID;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (B + JE_WAVES - 1) / JE_WAVES);
  hipLaunchKernelGGL(tzr_jagged_dot_attn_fwd_kernel, dim3(grid), dim3(JE_THREADS), 0, static_cast<hipStream_t>(stream), d_kv, kv_stride,
                     d_q, q_stride, D >> 2, je_group_lanes(D), d_offsets, B, max_len, d_out, out_stride, d_p);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

__global__ __launch_bounds__(JE_THREADS) void tzr_jagged_dot_attn_bwd_kernel(
    const float* __restrict__ gout, int64_t gos, const float* __restrict__ p, const float* __restrict__ kv, int64_t kvs,
    const float* __restrict__ q, int64_t qs, int lg, int P, const int64_t* __restrict__ offsets, int64_t B, int64_t max_len,
    float* __restrict__ dkv, int64_t dks, float* __restrict__ dq, int64_t dqs) {
  __shared__ float scs[JE_WAVES][JE_MAXLEN];
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  float* sc = scs[wv];
  const int G = TZR_WAVE / P, g = lane / P, c = lane & (P - 1);
  const bool on = c < lg;
  const int cl = on ? c : 0;
  for (int64_t b = (int64_t)blockIdx.x * JE_WAVES + wv; b < B; b += (int64_t)gridDim.x * JE_WAVES) {
    const int64_t s = offsets[b], e = offsets[b + 1];
    const int len = (int)min(e - s, max_len);
    for (int64_t k = (int64_t)len * lg + lane; k < (e - s) * lg; k += TZR_WAVE) tzr_st4(dkv + (s + k / lg) * dks + 4 * (k % lg), tzr_zero4());
    const float4 gg = on ? tzr_ld4(gout + b * gos + 4 * c) : tzr_zero4();
    const float4 qq = on ? tzr_ld4(q + b * qs + 4 * c) : tzr_zero4();
    float4 r[JE_HOLD];
    je_row_dots(kv, kvs, s, len, P, G, g, c, cl, gg, sc, r);  // sc[i] = t_i = g_b . k_i
    __builtin_amdgcn_wave_barrier();
    float dot = 0.f;
    for (int i = lane; i < len; i += TZR_WAVE) dot = fmaf(p[s + i], sc[i], dot);
    dot = tzr_wave_sum(dot);
    for (int i = lane; i < len; i += TZR_WAVE) sc[i] = p[s + i] * (sc[i] - dot);  // ds_i
    __builtin_amdgcn_wave_barrier();
    // dk_i = p_i g_b + ds_i q_b;  dq_b = sum_i ds_i k_i (a group in position order, the groups by a fixed tree)
    float4 a = tzr_zero4();
    if (len <= JE_HOLD * G) {
#pragma unroll
      for (int u = 0; u < JE_HOLD; ++u)
        if (u * G < len) {
          const int i = u * G + g;
          if (i < len) {
            const float pi = p[s + i], dsi = sc[i];
            if (on) tzr_st4(dkv + (s + i) * dks + 4 * c, tzr_fma4(dsi, qq, make_float4(pi * gg.x, pi * gg.y, pi * gg.z, pi * gg.w)));
            a = tzr_fma4(dsi, r[u], a);
          }
        }
    } else {
      for (int i0 = g; i0 < len; i0 += 4 * G) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * G;
          x[u] = tzr_ld4(kv + (s + (i < len ? i : len - 1)) * kvs + 4 * cl);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * G;
          if (i < len) {
            const float pi = p[s + i], dsi = sc[i];
            if (on) tzr_st4(dkv + (s + i) * dks + 4 * c, tzr_fma4(dsi, qq, make_float4(pi * gg.x, pi * gg.y, pi * gg.z, pi * gg.w)));
            a = tzr_fma4(dsi, x[u], a);
          }
        }
      }
    }
    a = je_across_groups(a, P);
    if (g == 0 && on) tzr_st4(dq + b * dqs + 4 * c, a);
    __builtin_amdgcn_wave_barrier();
  }
}

extern "C" int tzr_jagged_dot_attn_bwd(const float* d_grad_out, int64_t grad_out_stride, const float* d_p, const float* d_kv,
                                       int64_t kv_stride, const float* d_q, int64_t q_stride, int D, const int64_t* d_offsets,
                                       int64_t B, int64_t N, int64_t max_len, float* d_dkv, int64_t dkv_stride, float* d_dq,
                                       int64_t dq_stride, void* stream) {
  if (B < 0 || N < 0 || D <= 0 || max_len < 0) return TZR_ERR_INVALID;
  if ((D & 3) || D > JE_MAXDIM || ((grad_out_stride | kv_stride | q_stride | dkv_stride | dq_stride) & 3) || grad_out_stride < D ||
      kv_stride < D || q_stride < D || dkv_stride < D || dq_stride < D || max_len > JE_MAXLEN)
    return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_offsets || !d_grad_out || !d_q || !d_dq || (N > 0 && (!d_kv || !d_p || !d_dkv)) ||
      je_misaligned(d_grad_out, d_kv, d_q, d_dkv) || je_misaligned(d_dq))
    return TZR_ERR_INVALID;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (B + JE_WAVES - 1) / JE_WAVES);
  hipLaunchKernelGGL(tzr_jagged_dot_attn_bwd_kernel, dim3(grid), dim3(JE_THREADS), 0, static_cast<hipStream_t>(stream), d_grad_out,
                     grad_out_stride, d_p, d_kv, kv_stride, d_q, q_stride, D >> 2, je_group_lanes(D), d_offsets, B, max_len, d_dkv,
                     dkv_stride, d_dq, dq_stride);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// ---- sum / mean over a sample's first min(len, max_len) positions -----------------------------------------------------------
__global__ __launch_bounds__(JE_THREADS) void tzr_jagged_pool_fwd_kernel(const float* __restrict__ kv, int64_t kvs, int lg, int P,
                                                                         const int64_t* __restrict__ offsets, int64_t B, int64_t max_len,
                                                                         int mode, float* __restrict__ out, int64_t outs) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  const int G = TZR_WAVE / P, g = lane / P, c = lane & (P - 1);
  const bool on = c < lg;
  const int cl = on ? c : 0;
  for (int64_t b = (int64_t)blockIdx.x * JE_WAVES + wv; b < B; b += (int64_t)gridDim.x * JE_WAVES) {
    const int64_t s = offsets[b];
    const int64_t len = min(offsets[b + 1] - s, max_len);
    float4 a = tzr_zero4();
    for (int64_t i0 = g; i0 < len; i0 += 4 * G) {  // four of the group's positions per pass, loads together, added in position order
      float4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u * G;
        x[u] = tzr_ld4(kv + (s + (i < len ? i : len - 1)) * kvs + 4 * cl);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u * G < len) a = tzr_add4(a, x[u]);
    }
    a = je_across_groups(a, P);
    if (mode == TZR_POOL_MEAN) {
      const float cnt = (float)(len > 1 ? len : 1);
      a = make_float4(a.x / cnt, a.y / cnt, a.z / cnt, a.w / cnt);
    }
    if (g == 0 && on) tzr_st4(out + b * outs + 4 * c, a);
  }
}

extern "C" int tzr_jagged_pool_fwd(const float* d_kv, int64_t kv_stride, int D, const int64_t* d_offsets, int64_t B, int64_t N,
                                   int64_t max_len, int mode, float* d_out, int64_t out_stride, void* stream) {
  if (B < 0 || N < 0 || D <= 0 || max_len < 0 || (mode != TZR_POOL_SUM && mode != TZR_POOL_MEAN)) return TZR_ERR_INVALID;
  if ((D & 3) || D > JE_MAXDIM || ((kv_stride | out_stride) & 3) || kv_stride < D || out_stride < D) return TZR_ERR_UNSUPPORTED;
  if (B == 0) return TZR_OK;
  if (!d_offsets || !d_out || (N > 0 && !d_kv) || je_misaligned(d_kv, d_out)) return TZR_ERR_INVALID;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (B + JE_WAVES - 1) / JE_WAVES);
  hipLaunchKernelGGL(tzr_jagged_pool_fwd_kernel, dim3(grid), dim3(JE_THREADS), 0, static_cast<hipStream_t>(stream), d_kv, kv_stride,
                     D >> 2, je_group_lanes(D), d_offsets, B, max_len, mode, d_out, out_stride);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// one wave per sample: lane k of a pass = (position, piece) k of the sample's rows, row-major: whole rows, consecutive addresses
__global__ __launch_bounds__(JE_THREADS) void tzr_jagged_pool_bwd_kernel(const float* __restrict__ gout, int64_t gos, int lg,
                                                                         const int64_t* __restrict__ offsets, int64_t B, int64_t max_len,
                                                                         int mode, float* __restrict__ dkv, int64_t dks) {
  const int lane = threadIdx.x & (TZR_WAVE - 1);
  const int wv = threadIdx.x / TZR_WAVE;
  for (int64_t b = (int64_t)blockIdx.x * JE_WAVES + wv; b < B; b += (int64_t)gridDim.x * JE_WAVES) {
    const int64_t s = offsets[b], e = offsets[b + 1];
    const int64_t len = min(e - s, max_len);
    const float cnt = mode == TZR_POOL_MEAN ? (float)(len > 1 ? len : 1) : 1.0f;
    for (int64_t k = lane; k < (e - s) * lg; k += TZR_WAVE) {
      const int64_t i = k / lg;
      const int c = (int)(k - i * lg);
      float4 v = tzr_zero4();  // (a position at or behind max_len: a zero row, as tzr_padded_dense_to_jagged writes)
      if (i < len) {
        const float4 x = tzr_ld4(gout + b * gos + 4 * c);
        v = make_float4(x.x / cnt, x.y / cnt, x.z / cnt, x.w / cnt);
      }
      tzr_st4(dkv + (s + i) * dks + 4 * c, v);
    }
  }
}

extern "C" int tzr_jagged_pool_bwd(const float* d_grad_out, int64_t grad_out_stride, int D, const int64_t* d_offsets, int64_t B,
                                   int64_t N, int64_t max_len, int mode, float* d_dkv, int64_t dkv_stride, void* stream) {
  if (B < 0 || N < 0 || D <= 0 || max_len < 0 || (mode != TZR_POOL_SUM && mode != TZR_POOL_MEAN)) return TZR_ERR_INVALID;
  if ((D & 3) || D > JE_MAXDIM || ((grad_out_stride | dkv_stride) & 3) || grad_out_stride < D || dkv_stride < D) return TZR_ERR_UNSUPPORTED;
  if (B == 0 || N == 0) return TZR_OK;
  if (!d_offsets || !d_grad_out || !d_dkv || je_misaligned(d_grad_out, d_dkv)) return TZR_ERR_INVALID;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (B + JE_WAVES - 1) / JE_WAVES);
  hipLaunchKernelGGL(tzr_jagged_pool_bwd_kernel, dim3(grid), dim3(JE_THREADS), 0, static_cast<hipStream_t>(stream), d_grad_out,
                     grad_out_stride, D >> 2, d_offsets, B, max_len, mode, d_dkv, dkv_stride);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
