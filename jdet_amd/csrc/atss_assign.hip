// ATSS assignment of rotated anchors for gfx950 (MI355X): ATSSAssignerRbbox.assign.
//
// Reference semantics (a Jittor tensor program):
//   python/jdet/models/boxes/assigner.py:L314-391   (A, K) IoU + distance + inside matrices, one topk per level,
//                                                   a Python loop over gts, a second (K * A) "-INF" matrix
//   python/jdet/models/boxes/box_ops.py:L725-741    points_in_rotated_boxes (atan2 / cos / sin per pair)
// The rules the reference leaves open (tie order, the clamp to the level size, the algebraic inside test) are stated
// in include/jdet_hip.h.
//
// MI355X design (not a translation).  Only K x C pairs (C = sum over levels of min(topk, n_level), 45 at config size)
// decide anything, so nothing of size (A, K) is computed or stored; the cost is launch latency, three launches:
//   1. atss_topk_kernel   one workgroup per (gt, level).  Rank r of the level is the smallest packed key
//                         (distance bits << 32 | anchor index) above rank r - 1's: k block-wide minima over
//                         recomputed distances (a level is at most a few thousand L2-resident rows; no sorted
//                         per-lane lists, so no scratch).  A key is unique, and a smaller one means a smaller
//                         distance, then a lower index: the tie rule costs nothing.  All workgroups together also
//                         clear the per-anchor claim keys, grid-stride.
//   2. atss_claim_kernel  one wavefront per gt, lane c = candidate c: its IoU (the pair function of
//                         box_iou_rotated.hip, or the caller's matrix), lane 0 sums mean / variance serially,
//                         every lane tests threshold + inside and claims its anchor with a 64-bit atomicMax.
//   3. atss_write_kernel  one lane per anchor unpacks its key into gt_inds / max_overlaps / labels.
// No host synchronisation, no allocation, fixed shapes: the step captures into a HIP graph.
#include "jdet_hip.h"
#include "rotated_iou.h"

namespace {

constexpr int kMaxCand = JDET_ATSS_MAX_CANDIDATES;   // >= L * topk, so also the most levels
constexpr int kTopkBlock = 256;

struct AtssLevels {
  int32_t off[kMaxCand + 1];    // anchor rows of level l: [off[l], off[l+1])
  int32_t coff[kMaxCand + 1];   // candidate slots of level l: [coff[l], coff[l+1]), coff[L] = C
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(kTopkBlock) void atss_topk_kernel(const float* __restrict__ anchors, int A, int stride,
                                                               const float* __restrict__ gt, AtssLevels lv, int topk,
                                                               int C, unsigned long long* __restrict__ keys,
                                                               int32_t* __restrict__ cand) {
  __shared__ unsigned long long s_min[kTopkBlock / 64];
  const int g = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  {
    const size_t nthreads = (size_t)gridDim.x * gridDim.y * kTopkBlock;
    for (size_t i = ((size_t)l * gridDim.x + g) * kTopkBlock + tid; i < (size_t)A; i += nthreads) keys[i] = 0ull;
  }
  const int lo = lv.off[l], hi = lv.off[l + 1];
  const int k = min(topk, hi - lo);
  if (k <= 0) return;
  const float gx = gt[(size_t)g * 5], gy = gt[(size_t)g * 5 + 1];
  unsigned long long prev = 0ull;
  for (int r = 0; r < k; r++) {
    unsigned long long best = ~0ull;
    for (int j = lo + tid; j < hi; j += kTopkBlock) {
      const float dx = anchors[(size_t)j * stride] - gx, dy = anchors[(size_t)j * stride + 1] - gy;
      const float d = sqrtf(dx * dx + dy * dy);
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
      if ((r == 0 || key > prev) && key < best) best = key;
    }
    best = wave_min_u64(best);
    if ((tid & 63) == 0) s_min[tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kTopkBlock / 64; w++) best = s_min[w] < best ? s_min[w] : best;
    __syncthreads();
    // k <= n_level distinct keys exist, so a rank is always found; the guard keeps the index a row of the level
    if (tid == 0) cand[(size_t)g * C + lv.coff[l] + r] = best == ~0ull ? lo : (int32_t)(unsigned)best;
    prev = best;
  }
}

__global__ __launch_bounds__(64) void atss_claim_kernel(const float* __restrict__ anchors, int stride,
                                                        const float* __restrict__ gt, int K,
                                                        const float* __restrict__ overlaps, int C,
                                                        const int32_t* __restrict__ cand,
                                                        unsigned long long* __restrict__ keys) {
  __shared__ float s_x[24 * 64];
  __shared__ float s_y[24 * 64];
  __shared__ float s_iou[64];
  __shared__ float s_thr;
  const int g = blockIdx.x, lane = threadIdx.x;
  LanePts<64> q;
  q.x = s_x + lane;
  q.y = s_y + lane;
  float b[5];
#pragma unroll
  for (int k = 0; k < 5; k++) b[k] = gt[(size_t)g * 5 + k];
  int idx = 0;
  float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float iou = 0.f;
  if (lane < C) {
    idx = cand[(size_t)g * C + lane];
#pragma unroll
    for (int k = 0; k < 5; k++) a[k] = anchors[(size_t)idx * stride + k];
    iou = overlaps ? overlaps[(size_t)idx * K + g] : iou_dispatch<64>(a, b, 0, 0, q);
  }
  s_iou[lane] = iou;
  __syncthreads();
  if (lane == 0) {
    float s = 0.f;
    for (int c = 0; c < C; c++) s += s_iou[c];
    const float mean = s / (float)C;
    float v = 0.f;
    for (int c = 0; c < C; c++) {
      const float d = s_iou[c] - mean;
      v += d * d;
    }
    const float var = v / (float)(C - 1);
    s_thr = mean + sqrtf(fmaxf(var, 1e-6f));
  }
  __syncthreads();
  if (lane >= C) return;
  const float thr = s_thr;
  float sn, cs;
  sincosf(b[4], &sn, &cs);
  const float dx = a[0] - b[0], dy = a[1] - b[1];
  const bool inside = fabsf(dx * cs + dy * sn) < b[2] / 2 && fabsf(-dx * sn + dy * cs) < b[3] / 2;
  if (iou >= thr && inside && iou > 0.f)
    atomicMax(&keys[idx], ((unsigned long long)__float_as_uint(iou) << 32) | (0xFFFFFFFFu - (unsigned)g));
}

__global__ __launch_bounds__(256) void atss_write_kernel(const unsigned long long* __restrict__ keys, int A,
                                                         const int32_t* __restrict__ gt_labels, int labels_filled,
                                                         int32_t* __restrict__ gt_inds,
                                                         float* __restrict__ max_overlaps,
                                                         int32_t* __restrict__ labels) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= A) return;
  const unsigned long long key = keys[j];
  const int g = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
  gt_inds[j] = g + 1;
  max_overlaps[j] = key ? __uint_as_float((unsigned)(key >> 32)) : -1e8f;
  if (labels) labels[j] = key ? gt_labels[g] : labels_filled;
}

inline size_t keys_bytes(int A) { return (size_t)A * sizeof(unsigned long long); }

}  // namespace

JDET_API size_t jdet_atss_assign_workspace(int A, int K, int L, int topk) {
  if (A <= 0 || K <= 0 || L <= 0 || topk <= 0 || (long)L * topk > kMaxCand) return 0;
  // the claim keys, then K rows of at most L * topk candidate indices
  return keys_bytes(A) + (((size_t)K * L * topk * sizeof(int32_t) + 7) & ~(size_t)7);
}

JDET_API int jdet_atss_assign(const float* anchors, int A, int anchor_stride, const int32_t* level_offsets, int L,
                              const float* gt, int K, const int32_t* gt_labels, const float* overlaps, int topk,
                              int labels_filled, int32_t* gt_inds, float* max_overlaps, int32_t* labels,
                              void* workspace, size_t workspace_bytes, jdet_stream_t stream) {
  if (A <= 0 || K <= 0 || L <= 0 || topk <= 0 || anchor_stride < 5) return JDET_E_BADARG;
  if (!anchors || !level_offsets || !gt || !gt_inds || !max_overlaps || !workspace || (labels && !gt_labels) ||
      ((uintptr_t)workspace & 7))
    return JDET_E_BADARG;
  if ((long)L * topk > kMaxCand) return JDET_E_UNSUPPORTED;
  AtssLevels lv;
  if (level_offsets[0] != 0 || level_offsets[L] != A) return JDET_E_BADARG;
  lv.coff[0] = 0;
  for (int l = 0; l < L; l++) {
    if (level_offsets[l + 1] < level_offsets[l]) return JDET_E_BADARG;
    lv.off[l] = level_offsets[l];
    const int n = level_offsets[l + 1] - level_offsets[l];
    lv.coff[l + 1] = lv.coff[l] + (n < topk ? n : topk);
  }
  lv.off[L] = A;
  for (int l = L + 1; l <= kMaxCand; l++) lv.off[l] = A, lv.coff[l] = lv.coff[L];
  const int C = lv.coff[L];
  if (C < 2) return JDET_E_UNSUPPORTED;
  if (workspace_bytes < jdet_atss_assign_workspace(A, K, L, topk)) return JDET_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  int32_t* cand = (int32_t*)((char*)workspace + keys_bytes(A));
  hipLaunchKernelGGL(atss_topk_kernel, dim3(K, L), dim3(kTopkBlock), 0, st, anchors, A, anchor_stride, gt, lv, topk, C,
                     keys, cand);
  int e = jdet_launch_status();
  if (e) return e;
  hipLaunchKernelGGL(atss_claim_kernel, dim3(K), dim3(64), 0, st, anchors, anchor_stride, gt, K, overlaps, C, cand,
                     keys);
  e = jdet_launch_status();
  if (e) return e;
  hipLaunchKernelGGL(atss_write_kernel, dim3(jdet_cdiv(A, 256)), dim3(256), 0, st, (const unsigned long long*)keys, A,
                     gt_labels, labels_filled, gt_inds, max_overlaps, labels);
  return jdet_launch_status();
}
