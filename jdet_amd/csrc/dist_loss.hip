// Localization distillation for RetinaNet-OBB (include/jdet_hip.h): the regression branch predicts, per anchor,
// five distributions of reg_max + 1 logits instead of five numbers.
//
//   jdet_dist_integral          box_ops.integral / integral_angle: the expectation of each distribution
//   jdet_dist_bbox_loss_level   the integral + the weighted L1 / smooth-L1 of a level + d / d logits, one pass
//   jdet_kd_kl_div_level_*      knowledge_distillation_kl_div_loss of a level (LD term: rows of reg_max + 1 bins;
//                               class KD term: rows of cls_out_channels scores), forward and backward
//
// The reference composes each from about twenty tensor ops per level, every one a pass over (anchors, 45) maps, with a
// boolean row compaction (a host synchronisation) in the KL term.  Here each term reads its inputs once and writes its
// gradient once; the count of selected rows is summed, kept and used on the device.
//
// Every kernel walks tiles of kDistTileRows = 240 softmax rows (48 anchors), one row per thread, staged through LDS
// (dist_softmax.h).  Row arithmetic and sums are double and rounded once: the float64 references of tests/ld_ref.py are
// then met to the last float, whatever the summation order of the float32 composition happens to be.
#include "dist_softmax.h"
#include "jdet_hip.h"
#include "reduce.h"

namespace {

constexpr int kAnchorsPerTile = kDistTileRows / 5;
// the loss workspace (reduce.h: kJdetLossWorkspaceBytes = 4 KiB) holds the KL count's partials (int32) in front of the
// double partial sums of the loss
constexpr int kCountGridCap = 256;
constexpr int kSumGridCap = (int)((kJdetLossWorkspaceBytes - kCountGridCap * sizeof(int32_t)) / sizeof(double));
static_assert(kSumGridCap == 384, "1 KiB of counts + 3 KiB of sums");

__host__ __device__ inline double* sum_partials(void* ws) { return (double*)((char*)ws + kCountGridCap * sizeof(int32_t)); }

int sum_grid(long tiles) { return (int)(tiles < 1 ? 1 : (tiles > kSumGridCap ? kSumGridCap : tiles)); }

struct Ends {
  float lo, step, lo_angle, step_angle;   // e_k = lo + k * step, in fp32
};

// LOSS: the level loss (weights, targets, gradient, partial sums); otherwise the integral alone (deltas)
template <int KMAX, bool LOSS>
__global__ __launch_bounds__(256) void dist_bbox_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                        Blocked tb, const float* __restrict__ weight, Blocked wb,
                                                        long rows, int K, Ends ends, float beta,
                                                        float* __restrict__ grad, double* __restrict__ partial,
                                                        float* __restrict__ deltas) {
  __shared__ float s_tile[kDistTileRows * (KMAX + 1)];
  __shared__ float s_w[kDistTileRows];
  __shared__ int s_on[kAnchorsPerTile];
  __shared__ double s_part[4];
  const int t = threadIdx.x, kp = dist_pitch(K);
  const float inv_k = 1.f / (float)K;
  const long tile_el = (long)kDistTileRows * K;
  const long n_tiles = (rows + kAnchorsPerTile - 1) / kAnchorsPerTile;
  const bool vec = ((uintptr_t)logits & 15) == 0 && (!LOSS || ((uintptr_t)grad & 15) == 0);
  const int side = t % 5;
  double acc = 0.0;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long row0 = tile * kAnchorsPerTile;
    const int n_rows = (int)(rows - row0 < kAnchorsPerTile ? rows - row0 : kAnchorsPerTile);
    const int n_sm = n_rows * 5, n_el = n_sm * K;
    const bool mine = t < n_sm;
    float w = 1.f, tg = 0.f;
    if constexpr (LOSS) {
      if (mine) {
        const long r = row0 + t / 5;
        if (weight) w = weight[blocked_row(wb, r) * 5 + side];
        if (w != 0.f) tg = target[blocked_row(tb, r) * 5 + side];
      }
      if (t < kDistTileRows) s_w[t] = mine ? w : 0.f;
      __syncthreads();
      if (t < kAnchorsPerTile) {
        bool on = false;
#pragma unroll
        for (int s = 0; s < 5; s++) on = on || s_w[t * 5 + s] != 0.f;
        s_on[t] = on;
      }
      __syncthreads();
    }
    dist_tile_load(logits + tile * tile_el, n_el, K, inv_k, vec, s_tile, [&](int j) { return !LOSS || s_on[j / 5] != 0; });
    __syncthreads();
    if (mine) {
      float* row = s_tile + t * kp;
      if (!LOSS || w != 0.f) {
        DistSoftmax<KMAX> p;
        p.load(row, K, 1.0);
        const float e0 = side == 4 ? ends.lo_angle : ends.lo, step = side == 4 ? ends.step_angle : ends.step;
        double num = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; k++) num += p.e[k] * (double)(e0 + (float)k * step);
        const double rs = 1.0 / p.S, E = num / p.S;
        if constexpr (LOSS) {
          const double d = E - (double)tg, ad = fabs(d), b = (double)beta;
          double l, g;
          if (beta != 0.f && ad < b) {
            l = 0.5 * d * d / b;
            g = d / b;
          } else {
            l = beta != 0.f ? ad - 0.5 * b : ad;
            g = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
          }
          acc += l * (double)w;
          const double c = g * (double)w * rs;
#pragma unroll
          for (int k = 0; k < KMAX; k++)
            if (k < K) row[k] = (float)(c * p.e[k] * ((double)(e0 + (float)k * step) - E));
        } else {
          deltas[row0 * 5 + t] = (float)E;
        }
      } else {
        for (int k = 0; k < K; k++) row[k] = 0.f;
      }
    }
    __syncthreads();
    if constexpr (LOSS) {
      dist_tile_store(grad + tile * tile_el, n_el, K, inv_k, vec, s_tile);
      __syncthreads();
    }
  }
  if constexpr (LOSS) {
    const double sum = jdet_block_sum4(acc, s_part);
    if (t == 0) partial[blockIdx.x] = sum;
  }
}

// second stage of the level loss: thread t adds partial[t], partial[t + 256], ...; (sum / *avg_factor) * loss_weight
__global__ __launch_bounds__(256) void dist_bbox_finish_kernel(const double* __restrict__ partial, int n,
                                                               const float* __restrict__ avg_factor, float loss_weight,
                                                               float* __restrict__ out) {
  __shared__ double s_part[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const double total = jdet_block_sum4(acc, s_part);
  if (threadIdx.x == 0) out[0] = (float)((total / (double)avg_factor[0]) * (double)loss_weight);
}

// ---- KL divergence ----------------------------------------------------------------------------------------------------
// how many of the M weights are > 0: one int32 partial per workgroup (integers: any order gives the same sum)
__global__ __launch_bounds__(256) void kd_count_kernel(const float* __restrict__ weight, Blocked wb, long M,
                                                       int32_t* __restrict__ partial) {
  __shared__ int s_part[4];
  int acc = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long)gridDim.x * 256)
    acc += weight[blocked_row(wb, i)] > 0.f ? 1 : 0;
  const int sum = jdet_block_sum4(acc, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// the count every workgroup of the main kernels works with: all M rows when there is no weight or none is > 0
__device__ __forceinline__ long kd_effective_count(const int32_t* __restrict__ cnt_partial, int n_cnt, long M, int* s_ipart,
                                                   long* s_count) {
  int acc = 0;
  for (int i = threadIdx.x; i < n_cnt; i += 256) acc += cnt_partial[i];
  const int sum = jdet_block_sum4(acc, s_ipart);
  if (threadIdx.x == 0) *s_count = (n_cnt == 0 || sum == 0) ? M : (long)sum;
  __syncthreads();
  return *s_count;
}

// BACKWARD: writes grad_pred; otherwise the partial sums of sum_k t_k (log t_k - log p_k) over the selected rows.
// FORWARD reads the count's partials (n_cnt of them; 0 without a weight) and workgroup 0 publishes the count;
// BACKWARD reads the published count.
template <int KMAX, bool BACKWARD>
__global__ __launch_bounds__(256) void kd_kl_kernel(const float* __restrict__ pred, const float* __restrict__ soft,
                                                    const float* __restrict__ weight, Blocked wb, long M, int K,
                                                    float T, float loss_weight, const int32_t* __restrict__ cnt_partial,
                                                    int n_cnt, int32_t* __restrict__ count_out,
                                                    const int32_t* __restrict__ count_in,
                                                    const float* __restrict__ grad_out, double* __restrict__ partial,
                                                    float* __restrict__ grad) {
  __shared__ float s_tile[kDistTileRows * (KMAX + 1)];
  __shared__ int s_sel[kDistTileRows];
  __shared__ double s_part[4];
  __shared__ int s_ipart[4];
  __shared__ long s_count;
  const int t = threadIdx.x, kp = dist_pitch(K);
  const float inv_k = 1.f / (float)K;
  const double inv_t = 1.0 / (double)T;
  long count;
  if constexpr (BACKWARD) {
    count = count_in[0];
  } else {
    count = kd_effective_count(cnt_partial, n_cnt, M, s_ipart, &s_count);
    if (blockIdx.x == 0 && t == 0) count_out[0] = (int32_t)count;
  }
  const bool all = weight == nullptr || count == M;
  const long tile_el = (long)kDistTileRows * K;
  const long n_tiles = (M + kDistTileRows - 1) / kDistTileRows;
  const bool vec = (((uintptr_t)pred | (uintptr_t)soft) & 15) == 0 && (!BACKWARD || ((uintptr_t)grad & 15) == 0);
  double scale = 0.0;
  if constexpr (BACKWARD)
    scale = (double)grad_out[0] * (double)loss_weight * (double)T / (double)(float)(count * (long)K);
  double acc = 0.0;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long m0 = tile * kDistTileRows;
    const int n_sm = (int)(M - m0 < kDistTileRows ? M - m0 : kDistTileRows), n_el = n_sm * K;
    const bool mine = t < n_sm;
    const bool sel = mine && (all || weight[blocked_row(wb, m0 + t)] > 0.f);
    if (t < kDistTileRows) s_sel[t] = sel;
    __syncthreads();
    const auto need = [&](int j) { return s_sel[j] != 0; };
    float* row = s_tile + t * kp;
    DistSoftmax<KMAX> p, q;
    dist_tile_load(pred + tile * tile_el, n_el, K, inv_k, vec, s_tile, need);
    __syncthreads();
    if (sel) p.load(row, K, inv_t);
    __syncthreads();
    dist_tile_load(soft + tile * tile_el, n_el, K, inv_k, vec, s_tile, need);
    __syncthreads();
    if (sel) {
      q.load(row, K, inv_t);
      if constexpr (BACKWARD) {
        const double rp = scale / p.S, rq = scale / q.S;
#pragma unroll
        for (int k = 0; k < KMAX; k++)
          if (k < K) row[k] = (float)(p.e[k] * rp - q.e[k] * rq);
      } else {
        // sum_k t_k (log t_k - log p_k), t_k = e_k / S:  (sum_k e_k (xt_k - xp_k)) / S - (log S_t - log S_p)
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; k++)
          if (k < K) a += q.e[k] * (q.shifted(k, inv_t) - p.shifted(k, inv_t));
        acc += a / q.S - (log(q.S) - log(p.S));
      }
    } else if (BACKWARD && mine) {
      for (int k = 0; k < K; k++) row[k] = 0.f;
    }
    __syncthreads();
    if constexpr (BACKWARD) {
      dist_tile_store(grad + tile * tile_el, n_el, K, inv_k, vec, s_tile);
      __syncthreads();
    }
  }
  if constexpr (!BACKWARD) {
    const double sum = jdet_block_sum4(acc, s_part);
    if (t == 0) partial[blockIdx.x] = sum;
  }
}

// second stage: (sum / float(count * K)) * (T * T) * loss_weight
__global__ __launch_bounds__(256) void kd_finish_kernel(const double* __restrict__ partial, int n,
                                                        const int32_t* __restrict__ count, int K, float T,
                                                        float loss_weight, float* __restrict__ out) {
  __shared__ double s_part[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const double total = jdet_block_sum4(acc, s_part);
  if (threadIdx.x == 0)
    out[0] = (float)((total / (double)(float)((long)count[0] * K)) * ((double)T * (double)T) * (double)loss_weight);
}

bool bad_window(long rows_per_block, long block_stride) { return rows_per_block <= 0 || block_stride < 0; }
bool finite(float v) { return v == v && v - v == 0.f; }

// reg_max -> (status, e_k of both kinds of side)
int make_ends(int reg_max, float lo, float hi, float lo_angle, float hi_angle, Ends* out) {
  if (reg_max < 1 || !finite(lo) || !finite(hi) || !finite(lo_angle) || !finite(hi_angle)) return JDET_E_BADARG;
  if (reg_max + 1 > JDET_DIST_MAX_BINS) return JDET_E_UNSUPPORTED;
  *out = Ends{lo, (hi - lo) / (float)reg_max, lo_angle, (hi_angle - lo_angle) / (float)reg_max};
  return JDET_OK;
}

template <bool LOSS>
int launch_bbox(int K, int grid, hipStream_t st, const float* logits, const float* target, Blocked tb, const float* weight,
                Blocked wb, long rows, Ends ends, float beta, float* grad, double* partial, float* deltas) {
#define JDET_DIST_LAUNCH(KMAX)                                                                                          \
  hipLaunchKernelGGL((dist_bbox_kernel<KMAX, LOSS>), dim3(grid), dim3(256), 0, st, logits, target, tb, weight, wb, rows, \
                     K, ends, beta, grad, partial, deltas)
  if (K <= 8) JDET_DIST_LAUNCH(8);
  else if (K <= 16) JDET_DIST_LAUNCH(16);
  else JDET_DIST_LAUNCH(32);
#undef JDET_DIST_LAUNCH
  return jdet_launch_status();
}

template <bool BACKWARD>
int launch_kd(int grid, hipStream_t st, const float* pred, const float* soft, const float* weight, Blocked wb, long M,
              int K, float T, float loss_weight, const int32_t* cnt_partial, int n_cnt, int32_t* count_out,
              const int32_t* count_in, const float* grad_out, double* partial, float* grad) {
#define JDET_KD_LAUNCH(KMAX)                                                                                          \
  hipLaunchKernelGGL((kd_kl_kernel<KMAX, BACKWARD>), dim3(grid), dim3(256), 0, st, pred, soft, weight, wb, M, K, T,    \
                     loss_weight, cnt_partial, n_cnt, count_out, count_in, grad_out, partial, grad)
  if (K <= 8) JDET_KD_LAUNCH(8);
  else if (K <= 16) JDET_KD_LAUNCH(16);
  else JDET_KD_LAUNCH(32);
#undef JDET_KD_LAUNCH
  return jdet_launch_status();
}

int kd_check(long M, int K, float T, const float* weight, long wr, long ws) {
  if (M < 0 || K < 1 || !finite(T) || !(T >= 1.f)) return JDET_E_BADARG;
  if (weight && bad_window(wr, ws)) return JDET_E_BADARG;
  if (K > JDET_DIST_MAX_BINS || M > 2147483647L) return JDET_E_UNSUPPORTED;
  return JDET_OK;
}

}  // namespace

JDET_API int jdet_dist_integral(const float* logits, long rows, int reg_max, float lo, float hi, float lo_angle,
                                float hi_angle, float* deltas, jdet_stream_t stream) {
  Ends ends;
  if (rows < 0) return JDET_E_BADARG;
  if (int e = make_ends(reg_max, lo, hi, lo_angle, hi_angle, &ends)) return e;
  if (rows == 0) return JDET_OK;
  if (!logits || !deltas) return JDET_E_BADARG;
  const long tiles = (rows + kAnchorsPerTile - 1) / kAnchorsPerTile;
  const int grid = (int)(tiles > 4096 ? 4096 : tiles);
  return launch_bbox<false>(reg_max + 1, grid, (hipStream_t)stream, logits, nullptr, Blocked{1, 0}, nullptr, Blocked{1, 0},
                            rows, ends, 0.f, nullptr, nullptr, deltas);
}

JDET_API int jdet_dist_bbox_loss_level(const float* logits, const float* target, long target_rows_per_block,
                                       long target_block_stride, const float* weight, long weight_rows_per_block,
                                       long weight_block_stride, long rows, int reg_max, float lo, float hi,
                                       float lo_angle, float hi_angle, float beta, const float* avg_factor,
                                       float loss_weight, float* loss, float* grad_logits, void* workspace,
                                       size_t workspace_bytes, jdet_stream_t stream) {
  Ends ends;
  if (rows < 0 || !finite(beta) || beta < 0.f || !loss) return JDET_E_BADARG;
  if (int e = make_ends(reg_max, lo, hi, lo_angle, hi_angle, &ends)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) return jdet_zero_async(loss, sizeof(float), st);
  if (!logits || !target || !avg_factor || !grad_logits || !workspace) return JDET_E_BADARG;
  if (bad_window(target_rows_per_block, target_block_stride) ||
      (weight && bad_window(weight_rows_per_block, weight_block_stride)))
    return JDET_E_BADARG;
  if (workspace_bytes < kJdetLossWorkspaceBytes) return JDET_E_WORKSPACE;
  const int grid = sum_grid((rows + kAnchorsPerTile - 1) / kAnchorsPerTile);
  double* partial = sum_partials(workspace);
  if (int e = launch_bbox<true>(reg_max + 1, grid, st, logits, target, Blocked{target_rows_per_block, target_block_stride},
                                weight, Blocked{weight ? weight_rows_per_block : 1, weight ? weight_block_stride : 0}, rows,
                                ends, beta, grad_logits, partial, nullptr))
    return e;
  hipLaunchKernelGGL(dist_bbox_finish_kernel, dim3(1), dim3(256), 0, st, partial, grid, avg_factor, loss_weight, loss);
  return jdet_launch_status();
}

JDET_API int jdet_kd_kl_div_level_forward(const float* pred, const float* soft, const float* weight,
                                          long weight_rows_per_block, long weight_block_stride, long M, int K, float T,
                                          float loss_weight, float* loss, int32_t* count, void* workspace,
                                          size_t workspace_bytes, jdet_stream_t stream) {
  if (!loss || !count) return JDET_E_BADARG;
  if (int e = kd_check(M, K, T, weight, weight_rows_per_block, weight_block_stride)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {
    if (int e = jdet_zero_async(loss, sizeof(float), st)) return e;
    return jdet_zero_async(count, sizeof(int32_t), st);
  }
  if (!pred || !soft || !workspace) return JDET_E_BADARG;
  if (workspace_bytes < kJdetLossWorkspaceBytes) return JDET_E_WORKSPACE;
  const Blocked wb{weight ? weight_rows_per_block : 1, weight ? weight_block_stride : 0};
  int32_t* cnt_partial = (int32_t*)workspace;
  int n_cnt = 0;
  if (weight) {
    const long want = (M + 1023) / 1024;
    n_cnt = (int)(want > kCountGridCap ? kCountGridCap : want);
    hipLaunchKernelGGL(kd_count_kernel, dim3(n_cnt), dim3(256), 0, st, weight, wb, M, cnt_partial);
    if (int e = jdet_launch_status()) return e;
  }
  const int grid = sum_grid((M + kDistTileRows - 1) / kDistTileRows);
  double* partial = sum_partials(workspace);
  if (int e = launch_kd<false>(grid, st, pred, soft, weight, wb, M, K, T, loss_weight, cnt_partial, n_cnt, count, nullptr,
                               nullptr, partial, nullptr))
    return e;
  hipLaunchKernelGGL(kd_finish_kernel, dim3(1), dim3(256), 0, st, partial, grid, count, K, T, loss_weight, loss);
  return jdet_launch_status();
}

JDET_API int jdet_kd_kl_div_level_backward(const float* pred, const float* soft, const float* weight,
                                           long weight_rows_per_block, long weight_block_stride, long M, int K, float T,
                                           float loss_weight, const int32_t* count, const float* grad_out,
                                           float* grad_pred, jdet_stream_t stream) {
  if (!count || !grad_out) return JDET_E_BADARG;
  if (int e = kd_check(M, K, T, weight, weight_rows_per_block, weight_block_stride)) return e;
  if (M == 0) return JDET_OK;
  if (!pred || !soft || !grad_pred) return JDET_E_BADARG;
  const Blocked wb{weight ? weight_rows_per_block : 1, weight ? weight_block_stride : 0};
  const long tiles = (M + kDistTileRows - 1) / kDistTileRows;
  const int grid = (int)(tiles > 4096 ? 4096 : tiles);
  return launch_kd<true>(grid, (hipStream_t)stream, pred, soft, weight, wb, M, K, T, loss_weight, nullptr, 0, nullptr,
                         count, grad_out, nullptr, grad_pred);
}
