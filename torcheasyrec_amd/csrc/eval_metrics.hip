// K14: evaluation metrics whose state stays on the device (include/tzrec_hip.h, "evaluation metrics").
//
// Replaces, for the binary metrics of `model_config.metrics`, the torchmetrics modules the reference updates from
// RankModel.update_metric (tzrec/models/rank_model.py:375-443): the binned AUROC confusion matrix
// (preds[:, None] >= thresholds[None, :] then a bincount, one [B, T] intermediate per step), NormalizedEntropy's three
// sums, and GroupedAUC's Python loop over groups (tzrec/metrics/grouped_auc.py:96-125: a .tolist(),
// a torch.split and one AUROC call per group).
//
//   tzr_metric_update        B samples -> histogram over (threshold bin, class) + {sum ce, count, sum labels}: 12 bytes
//                            read per sample, one launch.  The [T, 2, 2] confusion matrix is suffix sums of the
//                            histogram (metrics.BinnedAUC.confmat): tp[t] = positives in bins > t.
//   tzr_grouped_auc_append   rows -> the caller's buffers at a device-side cursor
//   tzr_grouped_auc_reduce   sorted rows -> sum of per-group AUC, number of groups
#include "tzr_common.h"

#define EM_THREADS 256
#define EM_WAVES (EM_THREADS / TZR_WAVE)
#define EM_VEC 4           // samples per lane and iteration of the update (one float4 of probabilities)
#define EM_MAX_UPDATE_WGS 512

// ---- auc histogram + normalized entropy sums --------------------------------------------------------------------

// number of thresholds <= p (thr ascending, in LDS).  Written so that a NaN takes bin 0, like `p >= thr` being false.
__device__ __forceinline__ int em_bin(const float* thr, int T, float p) {
  int lo = 0, hi = T;  // invariant: thr[j] <= p for j < lo, !(thr[j] <= p) for j >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float em_bce(float p, bool y) {  // F.binary_cross_entropy: each log clamped at -100
  const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
  return y ? -lp : -lq;
}

__device__ __forceinline__ double em_wave_sum(double v) {
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;  // lane 0
}

struct alignas(16) EmLabel2 { int64_t x, y; };  // two labels, one 16-byte load

struct EmSample {
  unsigned* hist;
  const float* thr;
  int T;
  double ce, ys, cnt;
  __device__ __forceinline__ void operator()(float p, int64_t label) {
    const bool y = label != 0;
    if (hist) atomicAdd(hist + em_bin(thr, T, p) * 2 + (y ? 1 : 0), 1u);
    ce += (double)em_bce(p, y);
    ys += y ? 1.0 : 0.0;
    cnt += 1.0;
  }
};

template <bool VEC>
__global__ __launch_bounds__(EM_THREADS) void tzr_metric_update_kernel(
    const float* __restrict__ probs, const int64_t* __restrict__ labels, int64_t B, const float* __restrict__ thresholds, int T,
    unsigned long long* __restrict__ hist, double* __restrict__ ne) {
  __shared__ unsigned s_hist[(TZR_METRIC_MAX_THRESHOLDS + 1) * 2];
  __shared__ float s_thr[TZR_METRIC_MAX_THRESHOLDS];
  __shared__ double s_red[3 * EM_WAVES];
  const int nbins = hist ? (T + 1) * 2 : 0;
  for (int j = threadIdx.x; j < nbins; j += EM_THREADS) s_hist[j] = 0u;
  for (int j = threadIdx.x; j < (hist ? T : 0); j += EM_THREADS) s_thr[j] = thresholds[j];
  __syncthreads();
  EmSample acc{hist ? s_hist : nullptr, s_thr, T, 0.0, 0.0, 0.0};
  // (a workgroup counts at most B / gridDim.x + EM_THREADS * EM_VEC samples into a 32-bit LDS cell: the host side refuses
  // B >= 2^40, which keeps that below 2^32)
  if (VEC) {
    const int64_t nv = B / EM_VEC;  // whole float4s; the tail below
    for (int64_t v = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x; v < nv; v += (int64_t)gridDim.x * EM_THREADS) {
      const float4 p = *reinterpret_cast<const float4*>(probs + v * EM_VEC);
      const EmLabel2 l0 = *reinterpret_cast<const EmLabel2*>(labels + v * EM_VEC);
      const EmLabel2 l1 = *reinterpret_cast<const EmLabel2*>(labels + v * EM_VEC + 2);
      acc(p.x, l0.x); acc(p.y, l0.y); acc(p.z, l1.x); acc(p.w, l1.y);
    }
    if (blockIdx.x == 0) {
      const int64_t i = nv * EM_VEC + threadIdx.x;
      if (threadIdx.x < EM_VEC && i < B) acc(probs[i], labels[i]);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x; i < B; i += (int64_t)gridDim.x * EM_THREADS)
      acc(probs[i], labels[i]);
  }
  if (ne) {
    const double ce = em_wave_sum(acc.ce), ys = em_wave_sum(acc.ys), cnt = em_wave_sum(acc.cnt);
    const int wave = threadIdx.x / TZR_WAVE;
    if (threadIdx.x % TZR_WAVE == 0) { s_red[wave] = ce; s_red[EM_WAVES + wave] = ys; s_red[2 * EM_WAVES + wave] = cnt; }
  }
  __syncthreads();  // (also: every lane's LDS histogram adds)
  if (ne && threadIdx.x == 0) {
    double ce = 0.0, ys = 0.0, cnt = 0.0;  // (counts in double: exact integers)
    for (int w = 0; w < EM_WAVES; ++w) { ce += s_red[w]; ys += s_red[EM_WAVES + w]; cnt += s_red[2 * EM_WAVES + w]; }
    atomicAdd(ne + 0, ce);
    atomicAdd(ne + 1, cnt);
    atomicAdd(ne + 2, ys);
  }
  for (int j = threadIdx.x; j < nbins; j += EM_THREADS) {
    const unsigned c = s_hist[j];
    if (c) atomicAdd(hist + j, (unsigned long long)c);
  }
}

extern "C" int tzr_metric_update(const float* d_probs, const int64_t* d_labels, int64_t B, const float* d_thresholds, int T,
                                 uint64_t* d_hist, double* d_ne, void* stream) {
  if (B < 0 || (!d_hist && !d_ne)) return TZR_ERR_INVALID;
  if (d_hist && (T < 1 || !d_thresholds)) return TZR_ERR_INVALID;
  if (d_hist && T > TZR_METRIC_MAX_THRESHOLDS) return TZR_ERR_UNSUPPORTED;
  if (B >= ((int64_t)1 << 40)) return TZR_ERR_UNSUPPORTED;  // (32-bit LDS cells, see the kernel)
  if (B == 0) return TZR_OK;
  if (!d_probs || !d_labels) return TZR_ERR_INVALID;
  const bool vec = ((uintptr_t)d_probs % 16 == 0) && ((uintptr_t)d_labels % 16 == 0);
  const int64_t per = vec ? EM_THREADS * EM_VEC : EM_THREADS;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(EM_MAX_UPDATE_WGS, (B + per - 1) / per));
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(d_hist);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(tzr_metric_update_kernel<true>, dim3(grid), dim3(EM_THREADS), 0, s, d_probs, d_labels, B, d_thresholds, T, hist, d_ne);
  else
    hipLaunchKernelGGL(tzr_metric_update_kernel<false>, dim3(grid), dim3(EM_THREADS), 0, s, d_probs, d_labels, B, d_thresholds, T, hist, d_ne);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// ---- grouped AUC: append ----------------------------------------------------------------------------------------

// Every workgroup reads the cursor, then arrives at the launch's counter; the arrival that completes the count is behind
// every read, so it may move the cursor (and zero the counter for the next launch).  Row i of the batch always lands at
// cursor + i: the buffer's order does not depend on the schedule.
__global__ __launch_bounds__(EM_THREADS) void tzr_grouped_auc_append_kernel(
    const float* __restrict__ probs, const int64_t* __restrict__ labels, const int64_t* __restrict__ keys, int64_t B,
    float* __restrict__ row_probs, int32_t* __restrict__ row_labels, int64_t* __restrict__ row_keys, int64_t capacity,
    int64_t* state) {
  const int64_t base = *reinterpret_cast<volatile int64_t*>(state);
  const int64_t room = capacity > base ? capacity - base : 0;
  const int64_t take = B < room ? B : room;
  for (int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x; i < take; i += (int64_t)gridDim.x * EM_THREADS) {
    row_probs[base + i] = probs[i];
    row_labels[base + i] = labels[i] != 0 ? 1 : 0;
    row_keys[base + i] = keys[i];
  }
  __syncthreads();  // every lane of the workgroup holds `base` now
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned long long before = atomicAdd(reinterpret_cast<unsigned long long*>(state + 2), 1ull);
    if (before + 1 == gridDim.x) {
      state[0] = base + take;
      state[1] += B - take;
      state[2] = 0;
    }
  }
}

extern "C" int tzr_grouped_auc_append(const float* d_probs, const int64_t* d_labels, const int64_t* d_keys, int64_t B,
                                      float* d_row_probs, int32_t* d_row_labels, int64_t* d_row_keys, int64_t capacity,
                                      int64_t* d_state, void* stream) {
  if (B < 0 || capacity < 0 || !d_state) return TZR_ERR_INVALID;
  if (capacity > 0 && (!d_row_probs || !d_row_labels || !d_row_keys)) return TZR_ERR_INVALID;
  if (B == 0) return TZR_OK;
  if (!d_probs || !d_labels || !d_keys) return TZR_ERR_INVALID;
  const unsigned grid = (unsigned)std::min<int64_t>(1024, (B + EM_THREADS - 1) / EM_THREADS);
  hipLaunchKernelGGL(tzr_grouped_auc_append_kernel, dim3(grid), dim3(EM_THREADS), 0, static_cast<hipStream_t>(stream), d_probs,
                     d_labels, d_keys, B, d_row_probs, d_row_labels, d_row_keys, capacity, d_state);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}

// ---- grouped AUC: reduce ----------------------------------------------------------------------------------------
//
// Rows sorted by (key, prob).  cn[i] = negatives among rows [0, i) (exclusive prefix sum, n + 1 entries).  A positive row i
// of group [gs, ge) whose tie run is [rs, re) contributes 2 (cn[rs] - cn[gs]) + (cn[re] - cn[rs]) to the group's 2U; with
// cc = the prefix sum of the contributions, 2U of a group is cc[ge] - cc[gs], read by the group's first row.  Nothing
// walks a group: every row does three binary searches and four prefix reads.

struct EmRows {
  const int64_t* keys;
  const float* probs;
  int64_t n;
  // first row in [lo, hi) that is not before (key, prob) / is behind (key, prob) in the sorted order
  __device__ __forceinline__ int64_t lower(int64_t lo, int64_t hi, int64_t k, float p) const {
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      const int64_t km = keys[mid];
      if (km < k || (km == k && probs[mid] < p)) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
  __device__ __forceinline__ int64_t upper(int64_t lo, int64_t hi, int64_t k, float p) const {
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      const int64_t km = keys[mid];
      if (km < k || (km == k && probs[mid] <= p)) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
  __device__ __forceinline__ int64_t group_start(int64_t i, int64_t k) const {  // first row of key k, in [0, i]
    int64_t lo = 0, hi = i;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
  __device__ __forceinline__ int64_t group_end(int64_t i, int64_t k) const {  // one behind the last row of key k, in (i, n]
    int64_t lo = i + 1, hi = n;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
};

// x[i] = 1 for a negative row, x[n] = 0: scanned in place into cn
__global__ __launch_bounds__(EM_THREADS) void tzr_gauc_negatives_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  if (i <= n) x[i] = (i < n && labels[i] == 0) ? 1 : 0;
}

__global__ __launch_bounds__(EM_THREADS) void tzr_gauc_contrib_kernel(EmRows R, const int32_t* __restrict__ labels,
                                                                      const int64_t* __restrict__ cn, int64_t* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  if (i > R.n) return;
  int64_t c = 0;
  if (i < R.n && labels[i] != 0) {
    const int64_t k = R.keys[i];
    const float p = R.probs[i];
    const int64_t gs = R.group_start(i, k);
    const int64_t rs = R.lower(gs, i, k, p), re = R.upper(i + 1, R.n, k, p);
    const int64_t below = cn[rs] - cn[gs], tied = cn[re] - cn[rs];
    c = 2 * below + tied;
  }
  x[i] = c;
}

// In-place exclusive scan of int64 x[0, m) in three launches: per-workgroup sums, their scan by one workgroup, the
// workgroups' own scans on top of it.
__device__ __forceinline__ int64_t em_block_exclusive(int64_t v, int64_t* s_wave, int64_t* total) {
  const int lane = threadIdx.x % TZR_WAVE, wave = threadIdx.x / TZR_WAVE;
  int64_t inc = v;
  for (int d = 1; d < TZR_WAVE; d <<= 1) {
    const int64_t up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  if (lane == TZR_WAVE - 1) s_wave[wave] = inc;
  __syncthreads();
  int64_t before = 0, all = 0;
  for (int w = 0; w < EM_WAVES; ++w) {
    if (w < wave) before += s_wave[w];
    all += s_wave[w];
  }
  __syncthreads();  // (s_wave is reused by the caller's next round)
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(EM_THREADS) void tzr_scan_sums_kernel(const int64_t* __restrict__ x, int64_t m, int64_t* __restrict__ sums) {
  __shared__ int64_t s_wave[EM_WAVES];
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  int64_t total;
  em_block_exclusive(i < m ? x[i] : 0, s_wave, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(EM_THREADS) void tzr_scan_top_kernel(int64_t* __restrict__ sums, int64_t nb) {  // one workgroup
  __shared__ int64_t s_wave[EM_WAVES];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += EM_THREADS) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < nb ? sums[b] : 0;
    int64_t total;
    const int64_t ex = em_block_exclusive(v, s_wave, &total);
    if (b < nb) sums[b] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(EM_THREADS) void tzr_scan_apply_kernel(int64_t* __restrict__ x, int64_t m, const int64_t* __restrict__ sums) {
  __shared__ int64_t s_wave[EM_WAVES];
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  int64_t total;
  const int64_t ex = em_block_exclusive(i < m ? x[i] : 0, s_wave, &total);
  if (i < m) x[i] = sums[blockIdx.x] + ex;
}

// the first row of every group: its AUC when it holds both classes; per workgroup one partial (fixed order)
__global__ __launch_bounds__(EM_THREADS) void tzr_gauc_groups_kernel(EmRows R, const int64_t* __restrict__ cn, const int64_t* __restrict__ cc,
                                                                     double* __restrict__ part_sum, int64_t* __restrict__ part_cnt) {
  __shared__ double s_sum[EM_WAVES];
  __shared__ int64_t s_cnt[EM_WAVES];
  const int64_t i = (int64_t)blockIdx.x * EM_THREADS + threadIdx.x;
  double auc = 0.0;
  int64_t counted = 0;
  if (i < R.n) {
    const int64_t k = R.keys[i];
    if (i == 0 || R.keys[i - 1] != k) {
      const int64_t ge = R.group_end(i, k);
      const int64_t neg = cn[ge] - cn[i], pos = (ge - i) - neg;
      if (neg > 0 && pos > 0) {
        auc = (double)(cc[ge] - cc[i]) / (2.0 * (double)pos * (double)neg);
        counted = 1;
      }
    }
  }
  auc = em_wave_sum(auc);
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) counted += __shfl_down(counted, d);
  if (threadIdx.x % TZR_WAVE == 0) { s_sum[threadIdx.x / TZR_WAVE] = auc; s_cnt[threadIdx.x / TZR_WAVE] = counted; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int64_t c = 0;
    for (int w = 0; w < EM_WAVES; ++w) { s += s_sum[w]; c += s_cnt[w]; }
    part_sum[blockIdx.x] = s;
    part_cnt[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(EM_THREADS) void tzr_gauc_finish_kernel(const double* __restrict__ part_sum, const int64_t* __restrict__ part_cnt,
                                                                     int64_t nb, double* __restrict__ out_sum, int64_t* __restrict__ out_cnt) {  // one workgroup
  __shared__ double s_sum[EM_WAVES];
  __shared__ int64_t s_cnt[EM_WAVES];
  double s = 0.0;
  int64_t c = 0;
  for (int64_t b = threadIdx.x; b < nb; b += EM_THREADS) { s += part_sum[b]; c += part_cnt[b]; }
  s = em_wave_sum(s);
  for (int d = TZR_WAVE / 2; d > 0; d >>= 1) c += __shfl_down(c, d);
  if (threadIdx.x % TZR_WAVE == 0) { s_sum[threadIdx.x / TZR_WAVE] = s; s_cnt[threadIdx.x / TZR_WAVE] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = 0.0;
    c = 0;
    for (int w = 0; w < EM_WAVES; ++w) { s += s_sum[w]; c += s_cnt[w]; }
    *out_sum = s;
    *out_cnt = c;
  }
}

static inline int64_t em_blocks(int64_t m) { return (m + EM_THREADS - 1) / EM_THREADS; }

extern "C" size_t tzr_grouped_auc_reduce_workspace(int64_t n) {
  if (n < 0) return 0;
  const size_t m = (size_t)n + 1, nb = (size_t)em_blocks(n + 1);
  return 2 * tzr_align_up(m * 8) + tzr_align_up(nb * 8) + 2 * tzr_align_up(nb * 8);  // cn, cc | block sums | partial sums, counts
}

static void em_scan(int64_t* x, int64_t m, int64_t* sums, hipStream_t s) {
  const unsigned nb = (unsigned)em_blocks(m);
  hipLaunchKernelGGL(tzr_scan_sums_kernel, dim3(nb), dim3(EM_THREADS), 0, s, x, m, sums);
  hipLaunchKernelGGL(tzr_scan_top_kernel, dim3(1), dim3(EM_THREADS), 0, s, sums, (int64_t)nb);
  hipLaunchKernelGGL(tzr_scan_apply_kernel, dim3(nb), dim3(EM_THREADS), 0, s, x, m, sums);
}

extern "C" int tzr_grouped_auc_reduce(const int64_t* d_keys, const float* d_probs, const int32_t* d_labels, int64_t n,
                                      double* d_auc_sum, int64_t* d_groups, void* d_ws, size_t ws_bytes, void* stream) {
  if (n < 0 || !d_auc_sum || !d_groups) return TZR_ERR_INVALID;
  if (n >= ((int64_t)1 << 31) * EM_THREADS) return TZR_ERR_UNSUPPORTED;  // (one row per lane: the grid's x extent)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    hipLaunchKernelGGL(tzr_gauc_finish_kernel, dim3(1), dim3(EM_THREADS), 0, s, static_cast<const double*>(nullptr),
                       static_cast<const int64_t*>(nullptr), (int64_t)0, d_auc_sum, d_groups);
    TZR_CHECK_LAUNCH();
    return TZR_OK;
  }
  if (!d_keys || !d_probs || !d_labels) return TZR_ERR_INVALID;
  if (!d_ws || ((uintptr_t)d_ws % 256) || ws_bytes < tzr_grouped_auc_reduce_workspace(n)) return TZR_ERR_WORKSPACE;
  const int64_t m = n + 1, nb = em_blocks(m);
  TzrCarver carve(d_ws);
  int64_t* cn = carve.take<int64_t>((size_t)m);
  int64_t* cc = carve.take<int64_t>((size_t)m);
  int64_t* sums = carve.take<int64_t>((size_t)nb);
  double* part_sum = carve.take<double>((size_t)nb);
  int64_t* part_cnt = carve.take<int64_t>((size_t)nb);
  const EmRows R{d_keys, d_probs, n};
  hipLaunchKernelGGL(tzr_gauc_negatives_kernel, dim3((unsigned)nb), dim3(EM_THREADS), 0, s, d_labels, n, cn);
  em_scan(cn, m, sums, s);
  hipLaunchKernelGGL(tzr_gauc_contrib_kernel, dim3((unsigned)nb), dim3(EM_THREADS), 0, s, R, d_labels, cn, cc);
  em_scan(cc, m, sums, s);
  const int64_t nbg = em_blocks(n);
  hipLaunchKernelGGL(tzr_gauc_groups_kernel, dim3((unsigned)nbg), dim3(EM_THREADS), 0, s, R, cn, cc, part_sum, part_cnt);
  hipLaunchKernelGGL(tzr_gauc_finish_kernel, dim3(1), dim3(EM_THREADS), 0, s, part_sum, part_cnt, nbg, d_auc_sum, d_groups);
  TZR_CHECK_LAUNCH();
  return TZR_OK;
}
