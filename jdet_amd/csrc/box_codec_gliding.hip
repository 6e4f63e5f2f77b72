// Box codecs of the Gliding Vertex detector for gfx950, one fused launch each.
//
// Reference semantics (Jittor tensor programs, fp32; 60-80 elementwise launches per image and stage):
//   GVFixCoder.encode / decode            python/jdet/models/boxes/coder.py:L148-205
//   GVRatioCoder.encode                   python/jdet/models/boxes/coder.py:L213-228
//   GVDeltaXYWHBBoxCoder.encode / decode  python/jdet/models/boxes/coder.py:L242-320
//   poly2hbb / hbb2poly                   python/jdet/ops/bbox_transforms.py:L600-607, L649-651
//   the head's target pass and decode     python/jdet/models/roi_heads/gliding_head.py:L287-325, L355-379
// These passes are tiny (<= 1024 rows per training step, <= 2000 x 15 (row, class) pairs per image at inference):
// their cost is the launch, not the traffic.  One lane per row (per (row, class) for the class-wise decodes),
// grid-stride; the algebra above is inlined in the reference's order of operations.
//
// Extreme-vertex ties (GVFixCoder.encode takes argmax / argmin over the four x and the four y): the LOWEST vertex
// index wins.  Jittor's argmax tie order is not part of the reference tree, so this rule is this project's own; the
// torch composition in models/boxes/coder.py follows the same rule (torch.argmax returns the first extreme).
#include "common.h"

namespace {

struct Vec4 {
  float v[4];
};

// GVDeltaXYWHBBoxCoder.encode of one (box, gt) pair of horizontal boxes (L248-268)
__device__ __forceinline__ void gv_delta_encode(const float* a, float g0, float g1, float g2, float g3,
                                                const Vec4& means, const Vec4& stds, float* o) {
  const float px = (a[0] + a[2]) * 0.5f, py = (a[1] + a[3]) * 0.5f;
  const float pw = a[2] - a[0], ph = a[3] - a[1];
  const float gx = (g0 + g2) * 0.5f, gy = (g1 + g3) * 0.5f;
  const float gw = g2 - g0, gh = g3 - g1;
  const float d[4] = {(gx - px) / pw, (gy - py) / ph, logf(gw / pw), logf(gh / ph)};
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = (d[k] - means.v[k]) / stds.v[k];
}

// GVDeltaXYWHBBoxCoder.decode of one (box, delta) pair (L282-316); max_h / max_w <= 0: no clamp
__device__ __forceinline__ void gv_delta_decode(const float* a, const float* d, const Vec4& means, const Vec4& stds,
                                                float max_ratio, float max_h, float max_w, float* b) {
  float dd[4];
#pragma unroll
  for (int k = 0; k < 4; k++) dd[k] = d[k] * stds.v[k] + means.v[k];
  const float dw = fminf(fmaxf(dd[2], -max_ratio), max_ratio);
  const float dh = fminf(fmaxf(dd[3], -max_ratio), max_ratio);
  const float px = (a[0] + a[2]) * 0.5f, py = (a[1] + a[3]) * 0.5f;
  const float pw = a[2] - a[0], ph = a[3] - a[1];
  const float gw = pw * expf(dw), gh = ph * expf(dh);
  const float gx = px + pw * dd[0], gy = py + ph * dd[1];
  b[0] = gx - gw * 0.5f;
  b[1] = gy - gh * 0.5f;
  b[2] = gx + gw * 0.5f;
  b[3] = gy + gh * 0.5f;
  if (max_h > 0.f && max_w > 0.f) {
    b[0] = fminf(fmaxf(b[0], 0.f), max_w);
    b[1] = fminf(fmaxf(b[1], 0.f), max_h);
    b[2] = fminf(fmaxf(b[2], 0.f), max_w);
    b[3] = fminf(fmaxf(b[3], 0.f), max_h);
  }
}

__global__ __launch_bounds__(256) void gliding_targets_kernel(const float* __restrict__ rois,
                                                             const float* __restrict__ polys, long n, Vec4 means,
                                                             Vec4 stds, float* __restrict__ bbox_t,
                                                             float* __restrict__ fix_t, float* __restrict__ ratio_t) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float* p = polys + i * 8;
    float x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      x[k] = p[2 * k];
      y[k] = p[2 * k + 1];
    }
    // extreme vertices; strict comparisons in ascending index: the lowest index wins a tie
    float min_x = x[0], max_x = x[0], min_y = y[0], max_y = y[0];
    // coordinates of the extreme vertices the fix targets read: the top-most vertex's x, the right-most's (x, y), the
    // bottom-most's x, the left-most's y
    float top_x = x[0], top_y = y[0], right_x = x[0], right_y = y[0], bottom_x = x[0], left_y = y[0];
#pragma unroll
    for (int k = 1; k < 4; k++) {
      if (x[k] > max_x) { max_x = x[k]; right_x = x[k]; right_y = y[k]; }
      if (x[k] < min_x) { min_x = x[k]; left_y = y[k]; }
      if (y[k] > max_y) { max_y = y[k]; bottom_x = x[k]; }
      if (y[k] < min_y) { min_y = y[k]; top_x = x[k]; top_y = y[k]; }
    }
    gv_delta_encode(rois + i * 4, min_x, min_y, max_x, max_y, means, stds, bbox_t + i * 4);
    // GVFixCoder.encode (L176-184)
    const float w = max_x - min_x, h = max_y - min_y;
    const bool h_mask = (top_y - right_y == 0.f) || (right_x - bottom_x == 0.f);
    float* f = fix_t + i * 4;
    f[0] = h_mask ? 1.f : (top_x - min_x) / w;
    f[1] = h_mask ? 1.f : (right_y - min_y) / h;
    f[2] = h_mask ? 1.f : (max_x - bottom_x) / w;
    f[3] = h_mask ? 1.f : (max_y - left_y) / h;
    // GVRatioCoder.encode (L216-227): shoelace over the absolute coordinates, the reference's term order
    const float h_area = (max_x - min_x) * (max_y - min_y);
    float area = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int k1 = (k + 1) & 3;
      area += 0.5f * (x[k] * y[k1] - x[k1] * y[k]);
    }
    ratio_t[i] = fabsf(area) / h_area;
  }
}

__global__ __launch_bounds__(256) void gliding_decode_kernel(const float* __restrict__ rois,
                                                            const float* __restrict__ bbox_pred,
                                                            const float* __restrict__ fix_pred,
                                                            const float* __restrict__ ratio_pred, long n, int ncls,
                                                            Vec4 means, Vec4 stds, float max_ratio, float max_h,
                                                            float max_w, float ratio_thr, Vec4 scale,
                                                            float* __restrict__ out) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n * ncls; idx += (long)gridDim.x * 256) {
    float b[4];
    gv_delta_decode(rois + (idx / ncls) * 4, bbox_pred + idx * 4, means, stds, max_ratio, max_h, max_w, b);
    const float* f = fix_pred + idx * 4;
    // GVFixCoder.decode (L188-203): top, right, bottom, left vertex
    const float w = b[2] - b[0], h = b[3] - b[1];
    float q[8] = {b[0] + w * f[0], b[1], b[2], b[1] + h * f[1], b[2] - w * f[2], b[3], b[0], b[3] - h * f[3]};
    if (ratio_pred[idx] > ratio_thr) {     // nearly horizontal: the box itself, hbb2poly (gliding_head.py:L367)
      q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; q[3] = b[1];
      q[4] = b[2]; q[5] = b[3]; q[6] = b[0]; q[7] = b[3];
    }
    float* o = out + idx * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = q[k] / scale.v[k & 3];     // scale_factor.repeat(2) (L373)
  }
}

__global__ __launch_bounds__(256) void gv_delta_encode_kernel(const float* __restrict__ rois,
                                                             const float* __restrict__ gt, long n, Vec4 means,
                                                             Vec4 stds, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float* g = gt + i * 4;
    gv_delta_encode(rois + i * 4, g[0], g[1], g[2], g[3], means, stds, out + i * 4);
  }
}

__global__ __launch_bounds__(256) void gv_delta_decode_kernel(const float* __restrict__ rois,
                                                             const float* __restrict__ deltas, long n, int ncls,
                                                             Vec4 means, Vec4 stds, float max_ratio, float max_h,
                                                             float max_w, float* __restrict__ out) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n * ncls; idx += (long)gridDim.x * 256) {
    float b[4];
    gv_delta_decode(rois + (idx / ncls) * 4, deltas + idx * 4, means, stds, max_ratio, max_h, max_w, b);
    float* o = out + idx * 4;
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = b[k];
  }
}

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// |log(wh_ratio_clip)| in double, rounded once, as the reference's np.abs(np.log(wh_ratio_clip)) (coder.py:L289)
inline float max_ratio_of(float wh_ratio_clip) { return (float)fabs(log((double)wh_ratio_clip)); }

inline Vec4 vec_of(const float* p) {
  Vec4 v;
  for (int i = 0; i < 4; i++) v.v[i] = p[i];
  return v;
}

}  // namespace

JDET_API int jdet_gliding_targets(const float* rois_hbb, const float* gt_polys, long n, const float* means4,
                                  const float* stds4, float* bbox_targets, float* fix_targets, float* ratio_targets,
                                  jdet_stream_t stream) {
  if (n < 0 || !means4 || !stds4) return JDET_E_BADARG;
  if (n == 0) return JDET_OK;
  if (!rois_hbb || !gt_polys || !bbox_targets || !fix_targets || !ratio_targets) return JDET_E_BADARG;
  hipLaunchKernelGGL(gliding_targets_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, rois_hbb, gt_polys,
                     n, vec_of(means4), vec_of(stds4), bbox_targets, fix_targets, ratio_targets);
  return jdet_launch_status();
}

JDET_API int jdet_gliding_decode(const float* rois_hbb, const float* bbox_pred, const float* fix_pred,
                                 const float* ratio_pred, long n, int ncls, const float* means4, const float* stds4,
                                 float wh_ratio_clip, float max_h, float max_w, float ratio_thr, const float* scale4,
                                 float* out_polys, jdet_stream_t stream) {
  if (n < 0 || ncls <= 0 || !means4 || !stds4 || !scale4 || !(wh_ratio_clip > 0.f)) return JDET_E_BADARG;
  if (n == 0) return JDET_OK;
  if (!rois_hbb || !bbox_pred || !fix_pred || !ratio_pred || !out_polys) return JDET_E_BADARG;
  hipLaunchKernelGGL(gliding_decode_kernel, dim3(grid_for(n * ncls)), dim3(256), 0, (hipStream_t)stream, rois_hbb,
                     bbox_pred, fix_pred, ratio_pred, n, ncls, vec_of(means4), vec_of(stds4),
                     max_ratio_of(wh_ratio_clip), max_h, max_w, ratio_thr, vec_of(scale4), out_polys);
  return jdet_launch_status();
}

JDET_API int jdet_gv_delta_encode(const float* rois_hbb, const float* gt_hbb, long n, const float* means4,
                                  const float* stds4, float* out4, jdet_stream_t stream) {
  if (n < 0 || !means4 || !stds4) return JDET_E_BADARG;
  if (n == 0) return JDET_OK;
  if (!rois_hbb || !gt_hbb || !out4) return JDET_E_BADARG;
  hipLaunchKernelGGL(gv_delta_encode_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, rois_hbb, gt_hbb, n,
                     vec_of(means4), vec_of(stds4), out4);
  return jdet_launch_status();
}

JDET_API int jdet_gv_delta_decode(const float* rois_hbb, const float* deltas, long n, int ncls, const float* means4,
                                  const float* stds4, float wh_ratio_clip, float max_h, float max_w, float* out,
                                  jdet_stream_t stream) {
  if (n < 0 || ncls <= 0 || !means4 || !stds4 || !(wh_ratio_clip > 0.f)) return JDET_E_BADARG;
  if (n == 0) return JDET_OK;
  if (!rois_hbb || !deltas || !out) return JDET_E_BADARG;
  hipLaunchKernelGGL(gv_delta_decode_kernel, dim3(grid_for(n * ncls)), dim3(256), 0, (hipStream_t)stream, rois_hbb,
                     deltas, n, ncls, vec_of(means4), vec_of(stds4), max_ratio_of(wh_ratio_clip), max_h, max_w, out);
  return jdet_launch_status();
}
