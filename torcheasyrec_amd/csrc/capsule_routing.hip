// The behaviour-to-interest capsule layer of MIND (tzrec/modules/capsule.py:125-231) on the jagged rows: low capsules U = X W,
// num_iters rounds of dynamic routing, squash, capsule mask.  As torch ops that is a pad to [B, S, L], [B, S, H] low capsules, a
// normalized copy, [B, S, K] logits and six ops a round; here one launch forward and two backward, and nothing of shape [B, S, H]
// is ever in memory.
//
// A sample belongs to a WORKGROUP of 256 threads (4 waves), not to a wave: its low capsules (up to 128 x 64 or 64 x 128 floats,
// 32 KB) live in LDS for the whole routing, and four samples of that size in one workgroup's LDS would leave one workgroup a CU;
// the 16-row blocks of U = X W (four at S = 50, H = 64: sixteen tiles) spread over the four waves, and so do the K capsules of
// the squash.  Forward LDS: Us ceil16(S) x (H + 1) <= 8320 floats, Cs 128 x 8, Rn 128, Hs 8 x 128: 41 KB, three workgroups a CU of
// the 160 KB.  TZR_CAPSULE_MAX_SH = 8192 is that bound on ceil16(S) x H; the odd row stride H + 1 keeps the per-position reads of
// the agreement (thread n reads Us[n][h]) on distinct banks.
//
// U = X W is on v_mfma_f32_16x16x4_f32 (exact fp32): tile (row block, 16 columns of H) t on wave t mod 4; lane (li, q) loads the
// float4 at columns k0 + 4 q of X row li, and the four MFMAs of that load take its .x .y .z .w against W rows k0 + 4 q + e (the
// k-slot of an MFMA may stand for any column as long as A and B agree), four accumulator chains added pairwise.
// Routing: softmax one thread a position; high = C^T U one thread an element (k, h), positions ascending; agreement one thread a
// pair (n, k), h ascending; squash one wave a capsule, a fixed xor tree.  No atomics, every order fixed: two runs are bit-equal.
//
// Backward.  The routing weights are constants for autograd, so only the last round carries a gradient:
//   dpre_k = f g_k + pre_k (f / e) (2 p / (1 + e^2) - 1) t <pre_k, g_k> / |pre_k|,  f = r^p / e,  t = d max(|pre|, 1e-7) / d |pre|
//   (1 above, 1/2 at, 0 below the clamp, as torch.max passes it),  G = dpre W^T [K, L],  dx_n = sum_k c[n, k] G[k, :],
//   Z = c^T X [K, L],  dW += Z^T dpre.
// Workgroup g of min(B, TZR_CAPSULE_BWD_MAX_GRID) walks the samples g, g + grid, ... and keeps its dW partial in LDS (Ws, class
// L H <= 4096: 16 KB, else 64 KB; element e is thread e mod 256's alone; with the four 4 KB stages 32 KB / 80 KB a workgroup: five
// or two workgroups a CU), written to row g of the workspace at the end; the finishing launch is tzr_parts_sum_finish_kernel
// (interleaved order).
#include "parts_sum.h"
#include "tzr_common.h"

#define CP_THREADS 256
#define CP_WAVES (CP_THREADS / TZR_WAVE)
#define CP_MAXS TZR_CAPSULE_MAX_S
#define CP_MAXK TZR_CAPSULE_MAX_K
#define CP_MAXD TZR_CAPSULE_MAX_DIM
#define CP_US_FLOATS (TZR_CAPSULE_MAX_SH + CP_MAXS)  // ceil16(S) rows of H + 1 floats
#define CP_NORM_EPS 1e-12f                           // F.normalize
#define CP_SQUASH_EPS 1e-7f

static_assert(sizeof(TzrCapsule) == 192, "TzrCapsule: the layout _lib.py mirrors");
static_assert(CP_MAXD <= 2 * TZR_WAVE, "squash: two elements a lane");
static_assert(CP_MAXS <= CP_THREADS, "softmax: one thread a position");

typedef float cp_f4 __attribute__((ext_vector_type(4)));

struct CpArgs {
  const float* X;
  const int64_t* off;
  const float* W;
  const float* lg0;
  int64_t xs, B, N;
  int L, H, K, S, iters, constk;
  float scale, stddev, spow;
  float* high;
  int64_t hs;
  unsigned char* mask;
  float* c;
  float* pre;
  const float* gh;
  int64_t ghs;
  float* dX;
  int64_t dxs;
  float* parts;
};

// sample b: its first row, its length, the rows that take part, its valid capsules (offsets outside [0, N] are clamped: no
// access leaves the buffers whatever the offsets hold)
__device__ __forceinline__ void cp_sample(const CpArgs& A, int64_t b, int64_t* start, int64_t* len, int* s, int* kb) {
  int64_t s0 = A.off[b], s1 = A.off[b + 1];
  s0 = s0 < 0 ? 0 : (s0 > A.N ? A.N : s0);
  s1 = s1 < s0 ? s0 : (s1 > A.N ? A.N : s1);
  *start = s0;
  *len = s1 - s0;
  *s = (int)(*len < (int64_t)A.S ? *len : (int64_t)A.S);
  int k = 0;
  for (int j = 0; j < A.K; ++j) k += ((int64_t)1 << j) < *len ? 1 : 0;
  *kb = A.constk ? A.K : (k < 1 ? 1 : k);
}

__device__ __forceinline__ float cp_pow(float r, float p) { return p == 1.0f ? r : (p == 2.0f ? r * r : powf(r, p)); }

// grid B
__global__ __launch_bounds__(CP_THREADS) void tzr_capsule_fwd_kernel(CpArgs A) {
  __shared__ float Us[CP_US_FLOATS];
  __shared__ float Cs[CP_MAXS * CP_MAXK];
  __shared__ float Rn[CP_MAXS];
  __shared__ float Hs[CP_MAXK * CP_MAXD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, li = lane & 15;
  const int64_t b = blockIdx.x;
  const int L = A.L, H = A.H, K = A.K, HS = H + 1;
  int64_t start, len;
  int s, kb;
  cp_sample(A, b, &start, &len, &s, &kb);
  if (tid < K) A.mask[b * K + tid] = tid < kb ? 1 : 0;
  // U = X W
  const int nrb = (s + 15) >> 4, nct = (H + 15) >> 4;
  for (int t = wv; t < nrb * nct; t += CP_WAVES) {
    const int rb = t / nct, ct = t - rb * nct;
    const int row = 16 * rb + li, col = 16 * ct + li;
    const bool rok = row < s, cok = col < H;
    const float* xp = A.X + (start + (rok ? row : 0)) * A.xs;  // (s > 0 here: row 0 exists)
    cp_f4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = cp_f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < L; k0 += 16) {
      const int k = k0 + 4 * q;
      const bool kok = k < L;
      const float4 a = rok && kok ? tzr_ld4(xp + k) : tzr_zero4();
      float w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = cok && kok ? A.W[(int64_t)(k + e) * H + col] : 0.f;
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[0], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[1], acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[2], acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[3], acc[3], 0, 0, 0);
    }
    const cp_f4 u = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (cok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Us[(16 * rb + 4 * q + r) * HS + col] = u[r];
    }
  }
  __syncthreads();
  // 1 / max(|u_n|, eps) and the initial logits
  if (tid < s) {
    float ss = 0.f;
    for (int h = 0; h < H; ++h) {
      const float u = Us[tid * HS + h];
      ss = fmaf(u, u, ss);
    }
    Rn[tid] = 1.0f / fmaxf(sqrtf(ss), CP_NORM_EPS);
  }
  for (int i = tid; i < s * K; i += CP_THREADS) Cs[i] = A.lg0 ? A.lg0[start * K + i] * A.stddev : 0.f;
  for (int it = 0; it < A.iters; ++it) {
    __syncthreads();
    if (tid < s) {  // the weights over the valid capsules of logits * scale; a masked capsule's is 0
      float* row = Cs + tid * K;
      float v[CP_MAXK];
      float m = row[0] * A.scale;
#pragma unroll
      for (int k = 0; k < CP_MAXK; ++k) {
        v[k] = k < kb ? row[k] * A.scale : m;
        m = fmaxf(m, v[k]);
      }
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < CP_MAXK; ++k) {
        v[k] = k < kb ? expf(v[k] - m) : 0.f;
        sum += v[k];
      }
#pragma unroll
      for (int k = 0; k < CP_MAXK; ++k)
        if (k < K) row[k] = v[k] / sum;
    }
    __syncthreads();
    for (int o = tid; o < K * H; o += CP_THREADS) {  // high = C^T U, positions ascending
      const int k = o / H, h = o - k * H;
      float a = 0.f;
      if (k < kb)
        for (int n = 0; n < s; ++n) a = fmaf(Cs[n * K + k], Us[n * HS + h], a);
      Hs[o] = a;
    }
    __syncthreads();
    if (it + 1 < A.iters) {  // logits = weights + <high_k, u_n / max(|u_n|, eps)>
      for (int i = tid; i < s * kb; i += CP_THREADS) {
        const int k = i / s, n = i - k * s;
        float a = 0.f;
        for (int h = 0; h < H; ++h) a = fmaf(Hs[k * H + h], Us[n * HS + h], a);
        Cs[n * K + k] += a * Rn[n];
      }
    }
  }
  // squash: one wave a capsule
  for (int k = wv; k < K; k += CP_WAVES) {
    const bool h0 = lane < H, h1 = lane + TZR_WAVE < H;
    const float p0 = h0 ? Hs[k * H + lane] : 0.f, p1 = h1 ? Hs[k * H + lane + TZR_WAVE] : 0.f;
    const float ss = tzr_wave_sum(fmaf(p0, p0, p1 * p1));
    const float e = fmaxf(sqrtf(ss), CP_SQUASH_EPS), e2 = e * e;
    const float f = k < kb ? cp_pow(e2 / (1.0f + e2), A.spow) / e : 0.f;
    float* hp = A.high + (b * K + k) * A.hs;
    float* pp = A.pre + (b * K + k) * H;
    if (h0) hp[lane] = f * p0, pp[lane] = p0;
    if (h1) hp[lane + TZR_WAVE] = f * p1, pp[lane + TZR_WAVE] = p1;
  }
  for (int64_t i = tid; i < len * K; i += CP_THREADS) A.c[start * K + i] = i < (int64_t)s * K ? Cs[i] : 0.f;
}

// grid min(B, TZR_CAPSULE_BWD_MAX_GRID).  WN: the class's bound on L H (the dW partial in LDS)
template <int WN>
__global__ __launch_bounds__(CP_THREADS) void tzr_capsule_bwd_kernel(CpArgs A) {
  __shared__ float Ws[WN];
  __shared__ float Cs[CP_MAXS * CP_MAXK];
  __shared__ float Ps[CP_MAXK * CP_MAXD];  // dpre [K, H]
  __shared__ float Zs[CP_MAXK * CP_MAXD];  // c^T X [K, L]
  __shared__ float Gs[CP_MAXK * CP_MAXD];  // dpre W^T [K, L]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = A.L, H = A.H, K = A.K, LH = L * H, L4 = L >> 2;
  for (int e = tid; e < LH; e += CP_THREADS) Ws[e] = 0.f;
  for (int64_t b = blockIdx.x; b < A.B; b += gridDim.x) {
    int64_t start, len;
    int s, kb;
    cp_sample(A, b, &start, &len, &s, &kb);
    __syncthreads();  // (the sample before is read to its end)
    for (int i = tid; i < s * K; i += CP_THREADS) Cs[i] = A.c[start * K + i];
    for (int k = wv; k < K; k += CP_WAVES) {  // the squash backward: one wave a capsule
      const bool valid = k < kb, h0 = lane < H, h1 = lane + TZR_WAVE < H;
      const float* pp = A.pre + (b * K + k) * H;
      const float* gp = A.gh + (b * K + k) * A.ghs;
      const float p0 = h0 ? pp[lane] : 0.f, p1 = h1 ? pp[lane + TZR_WAVE] : 0.f;
      const float g0 = h0 && valid ? gp[lane] : 0.f, g1 = h1 && valid ? gp[lane + TZR_WAVE] : 0.f;
      const float ss = tzr_wave_sum(fmaf(p0, p0, p1 * p1));
      const float pg = tzr_wave_sum(fmaf(p0, g0, p1 * g1));
      const float norm = sqrtf(ss), e = fmaxf(norm, CP_SQUASH_EPS), e2 = e * e;
      const float f = cp_pow(e2 / (1.0f + e2), A.spow) / e;
      const float t = norm > CP_SQUASH_EPS ? 1.0f : (norm == CP_SQUASH_EPS ? 0.5f : 0.f);
      const float coef = t != 0.f ? (f / e) * (2.0f * A.spow / (1.0f + e2) - 1.0f) * t * (pg / norm) : 0.f;
      if (h0) Ps[k * H + lane] = valid ? fmaf(coef, p0, f * g0) : 0.f;
      if (h1) Ps[k * H + lane + TZR_WAVE] = valid ? fmaf(coef, p1, f * g1) : 0.f;
    }
    __syncthreads();
    for (int o = tid; o < K * L; o += CP_THREADS) {  // Z = c^T X (positions ascending) and G = dpre W^T
      const int k = o / L, l = o - k * L;
      float z = 0.f, g = 0.f;
      if (k < kb) {
        const float* xp = A.X + start * A.xs + l;
        for (int n = 0; n < s; ++n) z = fmaf(Cs[n * K + k], xp[n * A.xs], z);
        const float* wr = A.W + (int64_t)l * H;
        for (int h = 0; h < H; h += 4) {
          const float4 w = tzr_ld4(wr + h);
          const float* p = Ps + k * H + h;
          g = fmaf(p[0], w.x, g), g = fmaf(p[1], w.y, g), g = fmaf(p[2], w.z, g), g = fmaf(p[3], w.w, g);
        }
      }
      Zs[o] = z, Gs[o] = g;
    }
    __syncthreads();
    for (int64_t i = tid; i < len * L4; i += CP_THREADS) {  // dx_n = sum_k c[n, k] G[k, :]; rows behind S: zeros
      const int64_t n = i / L4;
      const int j = (int)(i - n * L4);
      float4 d = tzr_zero4();
      if (n < s)
        for (int k = 0; k < kb; ++k) {
          const float* g = Gs + k * L + 4 * j;
          d = tzr_fma4(Cs[n * K + k], make_float4(g[0], g[1], g[2], g[3]), d);
        }
      tzr_st4(A.dX + (start + n) * A.dxs + 4 * j, d);
    }
    for (int e = tid; e < LH; e += CP_THREADS) {  // dW += Z^T dpre
      const int l = e / H, h = e - l * H;
      float a = 0.f;
      for (int k = 0; k < kb; ++k) a = fmaf(Zs[k * L + l], Ps[k * H + h], a);
      Ws[e] += a;
    }
  }
  float* out = A.parts + (int64_t)blockIdx.x * LH;
  for (int e = tid; e < LH; e += CP_THREADS) out[e] = Ws[e];
}

// ---- host ------------------------------------------------------------------------------------------------------------

static inline int64_t cp_bwd_grid(int64_t B) { return B < TZR_CAPSULE_BWD_MAX_GRID ? B : TZR_CAPSULE_BWD_MAX_GRID; }
static inline size_t cp_ws_bytes(const TzrCapsule* c) { return tzr_align_up((size_t)cp_bwd_grid(c->B) * c->L * c->H * sizeof(float)); }

static bool cp_limits(const TzrCapsule* c) {
  if (c->L < 4 || (c->L & 3) || c->L > CP_MAXD || c->H < 4 || (c->H & 3) || c->H > CP_MAXD) return false;
  if (c->K < 1 || c->K > CP_MAXK || c->num_iters < 1 || c->num_iters > TZR_CAPSULE_MAX_ITERS) return false;
  if (c->S < 1 || c->S > CP_MAXS || (int64_t)((c->S + 15) / 16 * 16) * c->H > TZR_CAPSULE_MAX_SH) return false;
  if (!(c->scale > 0.f) || c->B >= (1ll << 31) || c->N >= (1ll << 31)) return false;
  return c->const_caps_num == 0 || c->const_caps_num == 1;
}

// sizes, limits (nothing else is looked at for a shape this build has no kernel for), then the pointers both directions read
static int cp_check(const TzrCapsule* c, CpArgs* A) {
  if (c->B < 0 || c->N < 0) return TZR_ERR_INVALID;
  if (!cp_limits(c)) return TZR_ERR_UNSUPPORTED;
  if (c->N > 0) TZR_TRY(tzr_rows_operand(c->x, c->x_stride, c->L));
  if (!c->offsets || (c->offsets & 7) || !c->w || (c->w & 15) || (c->logits0 & 3)) return TZR_ERR_INVALID;
  if (!c->pre || (c->pre & 3) || (c->N > 0 && (!c->c || (c->c & 3)))) return TZR_ERR_INVALID;
  A->X = reinterpret_cast<const float*>(c->x);
  A->off = reinterpret_cast<const int64_t*>(c->offsets);
  A->W = reinterpret_cast<const float*>(c->w);
  A->lg0 = reinterpret_cast<const float*>(c->logits0);
  A->xs = c->x_stride, A->B = c->B, A->N = c->N;
  A->L = c->L, A->H = c->H, A->K = c->K, A->S = c->S, A->iters = c->num_iters, A->constk = c->const_caps_num;
  A->scale = c->scale, A->stddev = c->stddev, A->spow = c->squash_pow;
  A->c = reinterpret_cast<float*>(c->c);
  A->pre = reinterpret_cast<float*>(c->pre);
  return TZR_OK;
}

extern "C" size_t tzr_capsule_workspace(const TzrCapsule* h_cap) {
  if (!h_cap || h_cap->B < 1 || !cp_limits(h_cap)) return 256;
  return cp_ws_bytes(h_cap) + 256;
}

extern "C" int tzr_capsule_fwd(const TzrCapsule* h_cap, void* stream) {
  if (!h_cap) return TZR_ERR_INVALID;
  CpArgs A = {};
  TZR_TRY(cp_check(h_cap, &A));
  TZR_TRY(tzr_rows_operand(h_cap->high, h_cap->high_stride, h_cap->H));
  if (!h_cap->mask) return TZR_ERR_INVALID;
  if (h_cap->B == 0) return TZR_OK;
  A.high = reinterpret_cast<float*>(h_cap->high);
  A.hs = h_cap->high_stride;
  A.mask = reinterpret_cast<unsigned char*>(h_cap->mask);
  hipLaunchKernelGGL(tzr_capsule_fwd_kernel, dim3((unsigned)h_cap->B), dim3(CP_THREADS), 0, static_cast<hipStream_t>(stream), A);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

extern "C" int tzr_capsule_bwd(const TzrCapsule* h_cap, void* stream) {
  if (!h_cap) return TZR_ERR_INVALID;
  CpArgs A = {};
  TZR_TRY(cp_check(h_cap, &A));
  TZR_TRY(tzr_rows_operand(h_cap->grad_high, h_cap->grad_high_stride, h_cap->H));
  if (h_cap->N > 0) TZR_TRY(tzr_rows_operand(h_cap->dx, h_cap->dx_stride, h_cap->L));
  if (!h_cap->dw || (h_cap->dw & 3)) return TZR_ERR_INVALID;
  if (h_cap->B == 0) return TZR_OK;
  if (!h_cap->ws || (h_cap->ws & 255) || h_cap->ws_bytes < cp_ws_bytes(h_cap)) return TZR_ERR_WORKSPACE;
  A.gh = reinterpret_cast<const float*>(h_cap->grad_high);
  A.ghs = h_cap->grad_high_stride;
  A.dX = reinterpret_cast<float*>(h_cap->dx);
  A.dxs = h_cap->dx_stride;
  A.parts = reinterpret_cast<float*>(h_cap->ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int G = (int)cp_bwd_grid(h_cap->B), LH = h_cap->L * h_cap->H;
  if (LH <= 4096) hipLaunchKernelGGL(tzr_capsule_bwd_kernel<4096>, dim3((unsigned)G), dim3(CP_THREADS), 0, s, A);
  else hipLaunchKernelGGL(tzr_capsule_bwd_kernel<CP_MAXD * CP_MAXD>, dim3((unsigned)G), dim3(CP_THREADS), 0, s, A);
  TZR_CHECK_LAUNCH();
  hipLaunchKernelGGL(tzr_parts_sum_finish_kernel<>, dim3((unsigned)((LH + TZR_WAVE - 1) / TZR_WAVE)), dim3(TZR_FIN_THREADS), 0, s, A.parts, G, LH,
                     reinterpret_cast<float*>(h_cap->dw));
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
