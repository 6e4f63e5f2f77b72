// FCOS point targets for rotated boxes on gfx950 (MI355X): FCOSHead.get_targets / _get_target_single.
//
// Reference semantics (a Jittor tensor program, per image in a Python loop):
//   python/jdet/models/roi_heads/fcos_head.py:L535-670   (points x gts) areas, ranges, offsets, 2x2 matrices, four
//                                                        distances, two masks, an argmin and two gathers
//   python/jdet/models/boxes/box_ops.py:L679-692         mintheta_obb
// The rules (matrix, inside, range, tie, background, empty image) are stated in include/jdet_hip.h.
//
// MI355X design (not a translation).  Nothing of size (points x gts) exists: one thread owns one (image, point), computes
// its coordinates from its index and keeps the running winner in registers.  The image's gts are walked in chunks of
// JDET_FCOS_GT_CHUNK staged in LDS; the staging thread prepares its gt once (mintheta_obb, one sincosf, the area, the
// label), so the inner loop is LDS broadcasts and a dozen flops.  The gt count is read from the device, so the call
// needs no host sync; one launch covers all images and levels.  Bandwidth is 8 output words per point: latency-bound.
#include "common.h"
#include "jdet_hip.h"

namespace {

constexpr int kChunk = JDET_FCOS_GT_CHUNK;
constexpr int kMaxLevels = JDET_FCOS_MAX_LEVELS;
constexpr int kBlock = 256;

struct FcosLevels {
  int32_t W[kMaxLevels], stride[kMaxLevels];
  int32_t off[kMaxLevels + 1];    // points of level l: [off[l], off[l+1]); levels beyond L are empty
  float lo[kMaxLevels], hi[kMaxLevels];
  float rad[kMaxLevels];          // stride * radius
};

// torch.remainder (floor-mod) of a by b > 0
__device__ __forceinline__ float floor_mod(float a, float b) {
  float r = fmodf(a, b);
  if (r != 0.f && r < 0.f) r += b;
  return r;
}

// regular_theta(theta, "180", -pi/2) of ops/bbox_transforms.py in fp32
__device__ __forceinline__ float regular_theta(float th) {
  const float half_pi = 1.5707963267948966f, pi = 3.141592653589793f;
  return floor_mod(th - (-half_pi), pi) + (-half_pi);
}

__global__ __launch_bounds__(kBlock) void fcos_targets_kernel(FcosLevels lv, int L, int N, const float* __restrict__ gt,
                                                             const int32_t* __restrict__ gt_labels,
                                                             const int32_t* __restrict__ gt_count, int Kmax,
                                                             int num_classes, int norm_on_bbox, int center_sampling,
                                                             int32_t* __restrict__ labels,
                                                             float* __restrict__ bbox_targets,
                                                             float* __restrict__ centerness,
                                                             int32_t* __restrict__ gt_inds) {
  __shared__ float s_cx[kChunk], s_cy[kChunk], s_w[kChunk], s_h[kChunk], s_th[kChunk], s_cos[kChunk], s_sin[kChunk],
      s_area[kChunk];
  __shared__ int32_t s_lab[kChunk];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int p = blockIdx.x * kBlock + tid;
  const bool live = p < N;
  int l = 0;
  while (l + 1 < L && p >= lv.off[l + 1]) l++;
  const int q = live ? p - lv.off[l] : 0;
  const int stride = lv.stride[l];
  const float px = (float)((q % lv.W[l]) * stride + stride / 2), py = (float)((q / lv.W[l]) * stride + stride / 2);
  const float lo = lv.lo[l], hi = lv.hi[l], rad = lv.rad[l];
  int K = gt_count[b];
  K = K < 0 ? 0 : (K > Kmax ? Kmax : K);

  int win = -1, win_lab = num_classes;
  float best = 0.f, bl = 0.f, bt = 0.f, br = 0.f, bb = 0.f, bth = 0.f;
  for (int base = 0; base < K; base += kChunk) {          // K is uniform over the block: so are the barriers
    const int n = min(kChunk, K - base);
    __syncthreads();
    if (tid < n) {
      const size_t g = (size_t)b * Kmax + base + tid;
      const float w = gt[g * 5 + 2], h = gt[g * 5 + 3], th = gt[g * 5 + 4];
      const float th1 = regular_theta(th), th2 = regular_theta(th + (float)(3.141592 / 2));
      const bool first = fabsf(th1) < fabsf(th2);
      const float a = first ? th1 : th2;
      s_cx[tid] = gt[g * 5];
      s_cy[tid] = gt[g * 5 + 1];
      s_w[tid] = first ? w : h;
      s_h[tid] = first ? h : w;
      s_th[tid] = a;
      sincosf(a, &s_sin[tid], &s_cos[tid]);
      s_area[tid] = w * h;
      s_lab[tid] = gt_labels[g] - 1;
    }
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < n; k++) {
      const float ox = px - s_cx[k], oy = py - s_cy[k];
      const float cs = s_cos[k], sn = s_sin[k];
      const float rx = cs * ox + (-sn) * oy, ry = sn * ox + cs * oy;
      const float hw = s_w[k] / 2, hh = s_h[k] / 2;
      const float dl = hw + rx, dr = hw - rx, dt = hh + ry, db = hh - ry;
      bool ok = fminf(fminf(dl, dt), fminf(dr, db)) > 0.f;
      if (center_sampling) ok = ok && fabsf(rx) < rad && fabsf(ry) < rad;
      const float mx = fmaxf(fmaxf(dl, dt), fmaxf(dr, db));
      ok = ok && mx >= lo && mx <= hi;
      const float area = s_area[k];
      if (ok && (win < 0 || area < best)) {               // strict: equal areas keep the lower index
        win = base + k;
        best = area;
        win_lab = s_lab[k];
        bl = dl; bt = dt; br = dr; bb = db; bth = s_th[k];
      }
    }
  }
  if (!live) return;
  float ctr = 0.f;
  if (win >= 0) {
    if (norm_on_bbox) {
      const float s = (float)stride;
      bl = bl / s; bt = bt / s; br = br / s; bb = bb / s;
    }
    ctr = sqrtf((fminf(bl, br) / fmaxf(bl, br)) * (fminf(bt, bb) / fmaxf(bt, bb)));
  }
  const size_t o = (size_t)b * N + p;
  labels[o] = win_lab;
  float* t = bbox_targets + o * 5;
  t[0] = bl; t[1] = bt; t[2] = br; t[3] = bb; t[4] = bth;
  centerness[o] = ctr;
  if (gt_inds) gt_inds[o] = win;
}

}  // namespace

JDET_API int jdet_fcos_targets(const int32_t* levels, const float* regress_ranges, int L, const float* gt,
                               const int32_t* gt_labels, const int32_t* gt_count, int B, int Kmax, int num_classes,
                               int norm_on_bbox, int center_sampling, float radius, int32_t* labels,
                               float* bbox_targets, float* centerness, int32_t* gt_inds, jdet_stream_t stream) {
  if (B <= 0 || Kmax < 0 || L <= 0 || num_classes <= 0) return JDET_E_BADARG;
  if (!levels || !regress_ranges || !gt_count || !labels || !bbox_targets || !centerness) return JDET_E_BADARG;
  if (Kmax > 0 && (!gt || !gt_labels)) return JDET_E_BADARG;
  if (center_sampling && !(radius > 0.f && radius < 3.0e38f)) return JDET_E_BADARG;
  if (L > kMaxLevels || B > 65535) return JDET_E_UNSUPPORTED;     // (B is the grid's y extent)
  FcosLevels lv;
  long N = 0;
  for (int l = 0; l < kMaxLevels; l++) {
    lv.off[l] = (int32_t)N;
    if (l < L) {
      const int H = levels[l * 3], W = levels[l * 3 + 1], s = levels[l * 3 + 2];
      if (H <= 0 || W <= 0 || s <= 0) return JDET_E_BADARG;
      if ((long)H * W > 0x7FFFFFFFL || (long)W * s > 0x7FFFFFFFL || (long)H * s > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;
      N += (long)H * W;
      if (N * B > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;
      lv.W[l] = W;
      lv.stride[l] = s;
      lv.lo[l] = regress_ranges[l * 2];
      lv.hi[l] = regress_ranges[l * 2 + 1];
      lv.rad[l] = center_sampling ? (float)s * radius : 0.f;
    } else {
      lv.W[l] = 1;
      lv.stride[l] = 1;
      lv.lo[l] = lv.hi[l] = lv.rad[l] = 0.f;
    }
  }
  lv.off[kMaxLevels] = (int32_t)N;
  hipLaunchKernelGGL(fcos_targets_kernel, dim3(jdet_cdiv(N, kBlock), B), dim3(kBlock), 0, (hipStream_t)stream, lv, L,
                     (int)N, gt, gt_labels, gt_count, Kmax, num_classes, norm_on_bbox ? 1 : 0, center_sampling ? 1 : 0,
                     labels, bbox_targets, centerness, gt_inds);
  return jdet_launch_status();
}
