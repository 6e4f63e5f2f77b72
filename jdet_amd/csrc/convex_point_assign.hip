// RepPoints init-stage point assignment for gfx950 (MI355X): ConvexAssigner.assign for a whole batch.
//
// Reference semantics (a Jittor tensor program driven by a host loop):
//   python/jdet/models/boxes/assigner.py:L433-548   per gt: a boolean mask over all points, a gather, a distance
//                                                   tensor, a topk, two scatter writes -- ~8 launches and several
//                                                   host syncs per gt, for at most pos_num positives per gt
// The rules (level of a gt, distance, tie order, the clamp to the level size, conflicts) are stated in
// include/jdet_hip.h.
//
// MI355X design (not a translation).  The work is a few hundred KB of reads; the cost is launches and syncs, so the
// whole batch is three launches and no sync:
//   1. convex_clear_kernel   the per-(image, point) claim keys := ~0 (a plain kernel: no memset node in a graph).
//   2. convex_claim_kernel   one wavefront per (image, gt).  Every lane derives the gt's box and level; lanes stride
//                            over the level's points; rank r is the smallest packed key (distance bits << 32 | point
//                            index) above rank r - 1's, by a wave-wide 64-bit minimum over recomputed distances (a
//                            level is at most a few thousand L2-resident rows; no per-lane sorted lists, no scratch).
//                            A key is unique and a smaller one means a smaller distance, then a lower index: the tie
//                            rule costs nothing.  Lane 0 claims the point with a 64-bit atomicMin on
//                            (distance bits << 32 | g): order-independent, hence deterministic.
//   3. convex_write_kernel   one lane per (image, point) unpacks its key into gt_inds / labels.
#include "common.h"
#include "jdet_hip.h"

#include <math.h>

namespace {

constexpr int kMaxLevels = JDET_CONVEX_ASSIGN_MAX_LEVELS;
constexpr unsigned long long kUnclaimed = ~0ull;

struct ConvexLevels {
  int32_t off[kMaxLevels + 1];   // point rows of level l: [off[l], off[l+1])
  int32_t id[kMaxLevels];        // log2(stride) of level l
  int32_t n, id_min, id_max;
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

// log2f, exact on exact powers of two (the header says why)
__device__ __forceinline__ float lg(float x) {
  int e;
  const float m = frexpf(x, &e);
  return m == 0.5f ? (float)(e - 1) : log2f(x);
}

__global__ __launch_bounds__(256) void convex_clear_kernel(unsigned long long* __restrict__ keys, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = kUnclaimed;
}

__global__ __launch_bounds__(64) void convex_claim_kernel(const float* __restrict__ points, int N, int stride,
                                                          ConvexLevels lv, const float* __restrict__ gt,
                                                          const int32_t* __restrict__ gt_count, int Kmax, float scale,
                                                          int pos_num, unsigned long long* __restrict__ keys) {
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  int cnt = gt_count[b];
  cnt = cnt < 0 ? 0 : (cnt > Kmax ? Kmax : cnt);
  if (g >= cnt) return;                                  // (uniform over the wavefront)
  const float* p = gt + ((size_t)b * Kmax + g) * 8;
  float xmin = p[0], xmax = p[0], ymin = p[1], ymax = p[1];
#pragma unroll
  for (int k = 1; k < 4; k++) {
    xmin = fminf(xmin, p[2 * k]), xmax = fmaxf(xmax, p[2 * k]);
    ymin = fminf(ymin, p[2 * k + 1]), ymax = fmaxf(ymax, p[2 * k + 1]);
  }
  const float cx = (xmin + xmax) / 2, cy = (ymin + ymax) / 2;
  const float w = fmaxf(xmax - xmin, 1e-6f), h = fmaxf(ymax - ymin, 1e-6f);
  int lvl = (int)((lg(w / scale) + lg(h / scale)) / 2);
  lvl = lvl < lv.id_min ? lv.id_min : (lvl > lv.id_max ? lv.id_max : lvl);
  int lo = 0, hi = 0;
#pragma unroll
  for (int l = 0; l < kMaxLevels; l++)
    if (l < lv.n && lv.id[l] == lvl) lo = lv.off[l], hi = lv.off[l + 1];
  const int k = min(pos_num, hi - lo);                   // <= 0: no such level, or an empty one
  unsigned long long* kb = keys + (size_t)b * N;
  unsigned long long prev = 0ull;
  for (int r = 0; r < k; r++) {
    unsigned long long best = kUnclaimed;
    for (int j = lo + lane; j < hi; j += 64) {
      const float dx = (points[(size_t)j * stride] - cx) / w, dy = (points[(size_t)j * stride + 1] - cy) / h;
      const float d = sqrtf(dx * dx + dy * dy);
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
      if ((r == 0 || key > prev) && key < best) best = key;
    }
    best = wave_min_u64(best);
    // k <= n_level distinct keys exist, so a rank is always found; the guard keeps the index a row of the level
    if (best == kUnclaimed) break;
    if (lane == 0) atomicMin(&kb[(unsigned)best], (best & 0xFFFFFFFF00000000ull) | (unsigned)g);
    prev = best;
  }
}

__global__ __launch_bounds__(256) void convex_write_kernel(const unsigned long long* __restrict__ keys, int N,
                                                           const int32_t* __restrict__ gt_labels, int Kmax,
                                                           int labels_filled, int32_t* __restrict__ gt_inds,
                                                           int32_t* __restrict__ labels) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= N) return;
  const size_t i = (size_t)b * N + j;
  const unsigned long long key = keys[i];
  const bool claimed = key != kUnclaimed;
  const int g = (int)(unsigned)key;
  gt_inds[i] = claimed ? g + 1 : 0;
  if (labels) labels[i] = claimed ? gt_labels[(size_t)b * Kmax + g] : labels_filled;
}

}  // namespace

JDET_API size_t jdet_convex_point_assign_workspace(int B, int N) {
  if (B <= 0 || N <= 0) return 0;
  return (size_t)B * N * sizeof(unsigned long long);
}

JDET_API int jdet_convex_point_assign(const float* points, int N, int point_stride, const int32_t* level_offsets,
                                      const int32_t* level_ids, int L, const float* gt, const int32_t* gt_labels,
                                      const int32_t* gt_count, int B, int Kmax, float scale, int pos_num,
                                      int labels_filled, int32_t* gt_inds, int32_t* labels, void* workspace,
                                      size_t workspace_bytes, jdet_stream_t stream) {
  if (N <= 0 || B <= 0 || Kmax < 0 || L <= 0 || point_stride < 2 || pos_num <= 0) return JDET_E_BADARG;
  if (!(scale > 0.f) || !isfinite(scale)) return JDET_E_BADARG;
  if (!points || !level_offsets || !level_ids || !gt_count || !gt_inds || !workspace || (Kmax > 0 && !gt) ||
      (labels && !gt_labels) || ((uintptr_t)workspace & 7))
    return JDET_E_BADARG;
  if (L > kMaxLevels || pos_num > JDET_CONVEX_ASSIGN_MAX_POS) return JDET_E_UNSUPPORTED;
  if ((long)B * N > 0x7FFFFFFFL || (long)B * Kmax > 0x7FFFFFFFL || B > 65535) return JDET_E_UNSUPPORTED;
  ConvexLevels lv;
  if (level_offsets[0] != 0 || level_offsets[L] != N) return JDET_E_BADARG;
  lv.n = L;
  lv.id_min = lv.id_max = level_ids[0];
  for (int l = 0; l < L; l++) {
    if (level_offsets[l + 1] < level_offsets[l]) return JDET_E_BADARG;
    for (int m = 0; m < l; m++)
      if (level_ids[m] == level_ids[l]) return JDET_E_BADARG;
    lv.off[l] = level_offsets[l];
    lv.id[l] = level_ids[l];
    lv.id_min = level_ids[l] < lv.id_min ? level_ids[l] : lv.id_min;
    lv.id_max = level_ids[l] > lv.id_max ? level_ids[l] : lv.id_max;
  }
  lv.off[L] = N;
  for (int l = L; l < kMaxLevels; l++) lv.off[l + 1] = N, lv.id[l] = 0;
  if (workspace_bytes < jdet_convex_point_assign_workspace(B, N)) return JDET_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  const long total = (long)B * N;
  hipLaunchKernelGGL(convex_clear_kernel, dim3(jdet_cdiv(total, 256)), dim3(256), 0, st, keys, total);
  int e = jdet_launch_status();
  if (e) return e;
  if (Kmax > 0) {
    hipLaunchKernelGGL(convex_claim_kernel, dim3(Kmax, B), dim3(64), 0, st, points, N, point_stride, lv, gt, gt_count,
                       Kmax, scale, pos_num, keys);
    e = jdet_launch_status();
    if (e) return e;
  }
  hipLaunchKernelGGL(convex_write_kernel, dim3(jdet_cdiv(N, 256), B), dim3(256), 0, st,
                     (const unsigned long long*)keys, N, gt_labels, Kmax, labels_filled, gt_inds, labels);
  return jdet_launch_status();
}
