// Gaussian box-regression losses of the rotated RetinaNet variants as ONE fused forward + gradient pass per pyramid
// level (round 7).  Replaces the tensor programs of the reference's
//   models/losses/gaussian_dist_loss.py:L48-276     GDLoss    (gwd, kld, jd, kld_symmax, kld_symmin; postprocess)
//   models/losses/gaussian_dist_loss_v1.py:L48-156  GDLoss_v1 (gwd, kld, bcd)
//   models/losses/kf_iou_loss.py:L48-99             KFLoss    (smooth-L1 on the xy deltas + the KF-IoU term)
// and the decode in front of them (`reg_decoded_bbox=True`; KFIoURRetinaHead always decodes both sides).  There every
// call starts with `jt.any(weight > 0)` (a host sync), compacts with `pred[mask]` (a dynamic shape) and composes
// dozens of small ops (2x2 bmm / det / inv) plus their autograd.  Here one thread owns one row: it decodes in
// registers (box_codec.h: the arithmetic of jdet_delta2bbox_rotated), builds both Gaussians, evaluates the distance
// and its post-processing and -- through forward-mode dual numbers over the row's 5 deltas -- the gradient, and adds
// the row when weight.mean(-1) > 0 (the weight is a mask only, as in the reference).  Per-workgroup partials, one
// finishing workgroup: (sum / *avg_factor) * loss_weight.  Deterministic, no atomics, no allocation, no host sync.
#include "box_codec.h"
#include "reduce.h"

namespace {

// ---- forward-mode dual numbers over the 5 delta inputs of a row ------------------------------------------------------
// v: value, g[k]: d v / d pred[k].  The value part is the very float operation of the plain code, so a decode through
// D5 rounds exactly like jdet_delta2bbox_rotated.  Clamps follow torch: the gradient passes where lo <= x <= hi.
struct D5 {
  float v;
  float g[5];
};

__device__ __forceinline__ D5 dconst(float c) {
  D5 r;
  r.v = c;
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = 0.f;
  return r;
}
__device__ __forceinline__ D5 dvar(float x, int i) {
  D5 r = dconst(x);
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = k == i ? 1.f : 0.f;
  return r;
}
__device__ __forceinline__ D5 dscale(const D5& a, float v, float s) {  // value v, gradient s * a.g
  D5 r;
  r.v = v;
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = a.g[k] * s;
  return r;
}
__device__ __forceinline__ D5 operator+(const D5& a, const D5& b) {
  D5 r;
  r.v = a.v + b.v;
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = a.g[k] + b.g[k];
  return r;
}
__device__ __forceinline__ D5 operator-(const D5& a, const D5& b) {
  D5 r;
  r.v = a.v - b.v;
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = a.g[k] - b.g[k];
  return r;
}
__device__ __forceinline__ D5 operator-(const D5& a) { return dscale(a, -a.v, -1.f); }
__device__ __forceinline__ D5 operator+(const D5& a, float b) { return dscale(a, a.v + b, 1.f); }
__device__ __forceinline__ D5 operator+(float a, const D5& b) { return dscale(b, a + b.v, 1.f); }
__device__ __forceinline__ D5 operator-(const D5& a, float b) { return dscale(a, a.v - b, 1.f); }
__device__ __forceinline__ D5 operator-(float a, const D5& b) { return dscale(b, a - b.v, -1.f); }
__device__ __forceinline__ D5 operator*(const D5& a, float b) { return dscale(a, a.v * b, b); }
__device__ __forceinline__ D5 operator*(float a, const D5& b) { return dscale(b, a * b.v, a); }
__device__ __forceinline__ D5 operator/(const D5& a, float b) { return dscale(a, a.v / b, 1.f / b); }
__device__ __forceinline__ D5 operator*(const D5& a, const D5& b) {
  D5 r;
  r.v = a.v * b.v;
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = a.g[k] * b.v + a.v * b.g[k];
  return r;
}
__device__ __forceinline__ D5 operator/(const D5& a, const D5& b) {
  D5 r;
  r.v = a.v / b.v;
#pragma unroll
  for (int k = 0; k < 5; k++) r.g[k] = (a.g[k] - r.v * b.g[k]) / b.v;
  return r;
}
__device__ __forceinline__ D5 operator/(float a, const D5& b) {
  const float v = a / b.v;
  return dscale(b, v, -v / b.v);
}
__device__ __forceinline__ D5 dsqrt(const D5& a) {
  const float v = sqrtf(a.v);
  return dscale(a, v, 0.5f / v);
}
__device__ __forceinline__ D5 dlog(const D5& a) { return dscale(a, logf(a.v), 1.f / a.v); }
__device__ __forceinline__ D5 dexp(const D5& a) {
  const float v = expf(a.v);
  return dscale(a, v, v);
}
__device__ __forceinline__ D5 dcos(const D5& a) { return dscale(a, cosf(a.v), -sinf(a.v)); }
__device__ __forceinline__ D5 dsin(const D5& a) { return dscale(a, sinf(a.v), cosf(a.v)); }
__device__ __forceinline__ D5 dabs(const D5& a) {
  return dscale(a, fabsf(a.v), a.v > 0.f ? 1.f : (a.v < 0.f ? -1.f : 0.f));
}
__device__ __forceinline__ D5 dclamp_min(const D5& a, float lo) { return dscale(a, fmaxf(a.v, lo), a.v >= lo ? 1.f : 0.f); }
__device__ __forceinline__ D5 dmax(const D5& a, const D5& b) { return a.v >= b.v ? a : b; }
__device__ __forceinline__ D5 dmin(const D5& a, const D5& b) { return a.v <= b.v ? a : b; }

// the decoder's hooks (box_codec.h), found by argument-dependent lookup
__device__ __forceinline__ float codec_val(const D5& x) { return x.v; }
__device__ __forceinline__ D5 codec_exp(const D5& x) { return dexp(x); }
__device__ __forceinline__ D5 codec_clamp(const D5& x, float lo, float hi) {
  return dscale(x, fminf(fmaxf(x.v, lo), hi), (x.v >= lo && x.v <= hi) ? 1.f : 0.f);
}

// ---- 2-D Gaussians ---------------------------------------------------------------------------------------------------
// xy_wh_r_2_xy_sigma: mean (x, y), Sigma = R diag((w/2)^2, (h/2)^2) R^T = [[a, b], [b, d]], wh clamped to [1e-7, 1e7]
struct Gauss {
  D5 x, y, a, b, d;
};

__device__ __forceinline__ Gauss to_gauss(const D5* box) {
  const D5 w = codec_clamp(box[2], 1e-7f, 1e7f), h = codec_clamp(box[3], 1e-7f, 1e7f);
  const D5 c = dcos(box[4]), s = dsin(box[4]);
  const D5 sw = 0.5f * w, sh = 0.5f * h;
  const D5 sw2 = sw * sw, sh2 = sh * sh;
  Gauss g;
  g.x = box[0];
  g.y = box[1];
  g.a = c * sw2 * c + s * sh2 * s;
  g.b = c * sw2 * s - s * sh2 * c;
  g.d = s * sw2 * s + c * sh2 * c;
  return g;
}
__device__ __forceinline__ D5 det2(const Gauss& p) { return p.a * p.d - p.b * p.b; }
__device__ __forceinline__ D5 trace2(const Gauss& p) { return p.a + p.d; }
__device__ __forceinline__ D5 trace_prod(const Gauss& p, const Gauss& t) {  // tr(Sp St)
  return p.a * t.a + 2.f * (p.b * t.b) + p.d * t.d;
}
// v^T M v with M = [[m00, m01], [m01, m11]]
__device__ __forceinline__ D5 quad(const D5& m00, const D5& m01, const D5& m11, const D5& dx, const D5& dy) {
  return m00 * dx * dx + 2.f * (m01 * dx * dy) + m11 * dy * dy;
}

// GDLoss postprocess: fun, then 1 - 1/(tau + d) when tau >= 1
__device__ __forceinline__ D5 post_v0(D5 d, int fun, float tau) {
  if (fun == JDET_GD_FUN_LOG1P) d = dlog(1.f + d);
  else if (fun == JDET_GD_FUN_SQRT) d = dsqrt(dclamp_min(d, 1e-7f));
  if (tau >= 1.f) return 1.f - 1.f / (tau + d);
  return d;
}

// GDLoss gwd_loss
__device__ D5 gwd_v0(const Gauss& p, const Gauss& t, const jdet_gaussian_loss_params_t& q) {
  const D5 dx = p.x - t.x, dy = p.y - t.y;
  const D5 xy = dx * dx + dy * dy;
  D5 whr = trace2(p) + trace2(t);
  const D5 t_tr = trace_prod(p, t);
  const D5 t_det_sqrt = dsqrt(dclamp_min(det2(p) * det2(t), 0.f));
  whr = whr + (-2.f) * dsqrt(dclamp_min(t_tr + 2.f * t_det_sqrt, 1e-7f));
  D5 dist = dsqrt(dclamp_min(xy + q.alpha * q.alpha * whr, 1e-7f));
  if (q.normalize) {
    const D5 scale = 2.f * dclamp_min(dsqrt(dclamp_min(dsqrt(dclamp_min(t_det_sqrt, 1e-7f)), 1e-7f)), 1e-7f);
    dist = dist / scale;
  }
  return post_v0(dist, q.fun, q.tau);
}

// GDLoss kld_loss before its postprocess (fun='none', tau=0 as jd / kld_symmax / kld_symmin call it).  As written there:
// inv(Sigma_p) is divided by det(Sigma_p) a second time.
__device__ D5 kld_v0_raw(const Gauss& p, const Gauss& t, float alpha, bool take_sqrt) {
  const D5 detp = det2(p);
  const D5 i00 = p.d / detp / detp, i01 = -p.b / detp / detp, i11 = p.a / detp / detp;
  const D5 dx = p.x - t.x, dy = p.y - t.y;
  const D5 xy = 0.5f * quad(i00, i01, i11, dx, dy);
  D5 whr = 0.5f * (i00 * t.a + 2.f * (i01 * t.b) + i11 * t.d);
  whr = whr + 0.5f * (dlog(detp) - dlog(det2(t)));
  whr = whr - 1.f;
  D5 dist = xy / (alpha * alpha) + whr;
  if (take_sqrt) dist = dsqrt(dclamp_min(dist, 1e-7f));
  return dist;
}

// GDLoss_v1 gwd_loss
__device__ D5 gwd_v1(const Gauss& p, const Gauss& t, const jdet_gaussian_loss_params_t& q) {
  const D5 dx = p.x - t.x, dy = p.y - t.y;
  const D5 xy = dx * dx + dy * dy;
  D5 whr = trace2(p) + trace2(t);
  const D5 t_tr = trace_prod(p, t);
  const D5 t_det_sqrt = dsqrt(dclamp_min(det2(p) * det2(t), 0.f));
  whr = whr + (-2.f) * dsqrt(dclamp_min(t_tr + 2.f * t_det_sqrt, 0.f));
  const D5 g = dclamp_min(xy + whr, 1e-6f);
  if (q.fun == JDET_GD_FUN_SQRT) return 1.f - 1.f / (q.tau + dsqrt(g));
  if (q.fun == JDET_GD_FUN_LOG1P) return 1.f - 1.f / (q.tau + dlog(1.f + g));
  const D5 scale = 2.f * dclamp_min(dsqrt(dsqrt(t_det_sqrt)), 1e-7f);
  return dlog(1.f + dsqrt(g) / scale);
}

// GDLoss_v1 bcd_loss
__device__ D5 bcd_v1(const Gauss& p, const Gauss& t, const jdet_gaussian_loss_params_t& q) {
  Gauss m;
  m.a = 0.5f * (p.a + t.a);
  m.b = 0.5f * (p.b + t.b);
  m.d = 0.5f * (p.d + t.d);
  const D5 detm = det2(m);
  const D5 dx = p.x - t.x, dy = p.y - t.y;
  const D5 term1 = dlog(detm / dsqrt(det2(t) * det2(p)));
  const D5 term2 = quad(m.d / detm, -m.b / detm, m.a / detm, dx, dy);
  const D5 b = dclamp_min(0.5f * term1 + 0.125f * term2, 1e-6f);
  if (q.fun == JDET_GD_FUN_SQRT) return 1.f - 1.f / (q.tau + dsqrt(b));
  if (q.fun == JDET_GD_FUN_LOG1P) return 1.f - 1.f / (q.tau + dlog(1.f + b));
  return 1.f - 1.f / (q.tau + b);
}

// GDLoss_v1 kld_loss: inverts Sigma_t (not Sigma_p), no 0.5 factors, clamp at 1e-6
__device__ D5 kld_v1(const Gauss& p, const Gauss& t, const jdet_gaussian_loss_params_t& q) {
  const D5 dett = det2(t);
  const D5 t00 = t.d / dett, t01 = -t.b / dett, t11 = t.a / dett;
  const D5 dx = p.x - t.x, dy = p.y - t.y;
  const D5 term1 = quad(t00, t01, t11, dx, dy);
  const D5 term2 = (t00 * p.a + 2.f * (t01 * p.b) + t11 * p.d) + dlog(dett / det2(p));
  const D5 kl = dclamp_min(term1 + term2 - 2.f, 1e-6f);
  if (q.fun == JDET_GD_FUN_SQRT) return 1.f - 1.f / (q.tau + dsqrt(kl));
  return 1.f - 1.f / (q.tau + dlog(1.f + kl));
}

// KFLoss kfiou_loss: smooth-L1 on the xy DELTAS + the KF-IoU term of the decoded boxes.  Vb = where(isnan(Vb), 0, Vb)
// of the reference: det(Sigma) <= 0 (rounding) gives Vb = 0 with a ZERO gradient here (the torch composition would
// back-propagate NaN through the square root of a negative number).
__device__ D5 kfiou(const D5* dp, const float* dt, const Gauss& p, const Gauss& t, const jdet_gaussian_loss_params_t& q) {
  D5 xy_loss = dconst(0.f);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const D5 diff = dabs(dp[k] - dt[k]);
    xy_loss = xy_loss + (diff.v < q.beta ? 0.5f * diff * diff / q.beta : diff - 0.5f * q.beta);
  }
  const D5 vb_p = 4.f * dsqrt(det2(p));
  const D5 vb_t = 4.f * dsqrt(det2(t));
  // K = Sp inv(Sp + St); Sigma = Sp - K Sp
  Gauss m;
  m.a = p.a + t.a;
  m.b = p.b + t.b;
  m.d = p.d + t.d;
  const D5 detm = det2(m);
  const D5 n00 = m.d / detm, n01 = -m.b / detm, n11 = m.a / detm;
  const D5 k00 = p.a * n00 + p.b * n01, k01 = p.a * n01 + p.b * n11;
  const D5 k10 = p.b * n00 + p.d * n01, k11 = p.b * n01 + p.d * n11;
  // Sigma = Sp - K Sp = K St (Sp - Sp M^-1 Sp = Sp M^-1 (M - Sp)): the same matrix, without the fp32 cancellation of the
  // subtraction when Sp >> St (which there costs the gradient most of its digits)
  const D5 s00 = k00 * t.a + k01 * t.b, s01 = k00 * t.b + k01 * t.d;
  const D5 s10 = k10 * t.a + k11 * t.b, s11 = k10 * t.b + k11 * t.d;
  const D5 dets = s00 * s11 - s01 * s10;
  const D5 vb = dets.v > 0.f ? 4.f * dsqrt(dets) : dconst(0.f);
  const D5 kf = vb / (vb_p + vb_t - vb + q.eps);
  D5 kf_loss;
  if (q.fun == JDET_GD_FUN_LN) kf_loss = -dlog(kf + q.eps);
  else if (q.fun == JDET_GD_FUN_EXP) kf_loss = dexp(1.f - kf) - 1.f;
  else kf_loss = 1.f - kf;
  return dclamp_min(xy_loss + kf_loss, 0.f);
}

// one thread per row; rows with weight.mean(-1) <= 0 contribute 0 and a zero gradient
__global__ __launch_bounds__(256) void gaussian_loss_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ target, Blocked tb,
                                                            const float* __restrict__ weight, Blocked wb,
                                                            const float* __restrict__ anchors, long anchor_rows,
                                                            long rows, jdet_gaussian_loss_params_t q, Vec5 means,
                                                            Vec5 stds, float max_ratio, float* __restrict__ grad,
                                                            float* __restrict__ partial) {
  __shared__ float s_part[4];
  float acc = 0.f;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
    bool on = true;
    if (weight) {
      const float* w = weight + blocked_row(wb, r) * 5;
      on = ((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) / 5.f > 0.f;
    }
    float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
      D5 d[5];
#pragma unroll
      for (int k = 0; k < 5; k++) d[k] = dvar(pred[r * 5 + k], k);
      const float* tr = target + blocked_row(tb, r) * 5;
      float t[5];
#pragma unroll
      for (int k = 0; k < 5; k++) t[k] = tr[k];
      const float* a = anchors ? anchors + (r % anchor_rows) * 5 : nullptr;
      D5 pb[5];
      if (q.decode_pred) {
        delta2bbox_one<D5>(a, d, means, stds, max_ratio, pb);
      } else {
#pragma unroll
        for (int k = 0; k < 5; k++) pb[k] = d[k];
      }
      float tbx[5];
      if (q.decode_target) {
        delta2bbox_one<float>(a, t, means, stds, max_ratio, tbx);
      } else {
#pragma unroll
        for (int k = 0; k < 5; k++) tbx[k] = t[k];
      }
      D5 tbd[5];
#pragma unroll
      for (int k = 0; k < 5; k++) tbd[k] = dconst(tbx[k]);
      const Gauss gp = to_gauss(pb), gt = to_gauss(tbd);
      D5 l;
      switch (q.kind) {
        case JDET_GD_GWD: l = gwd_v0(gp, gt, q); break;
        case JDET_GD_KLD: l = post_v0(kld_v0_raw(gp, gt, q.alpha, q.sqrt_dist != 0), q.fun, q.tau); break;
        case JDET_GD_JD: {
          D5 j = (kld_v0_raw(gp, gt, q.alpha, false) + kld_v0_raw(gt, gp, q.alpha, false)) * 0.5f;
          if (q.sqrt_dist) j = dsqrt(dclamp_min(j, 1e-7f));
          l = post_v0(j, q.fun, q.tau);
          break;
        }
        case JDET_GD_KLD_SYMMAX:
          l = post_v0(dmax(kld_v0_raw(gp, gt, q.alpha, q.sqrt_dist != 0), kld_v0_raw(gt, gp, q.alpha, q.sqrt_dist != 0)), q.fun,
                      q.tau);
          break;
        case JDET_GD_KLD_SYMMIN:
          l = post_v0(dmin(kld_v0_raw(gp, gt, q.alpha, q.sqrt_dist != 0), kld_v0_raw(gt, gp, q.alpha, q.sqrt_dist != 0)), q.fun,
                      q.tau);
          break;
        case JDET_GD1_GWD: l = gwd_v1(gp, gt, q); break;
        case JDET_GD1_KLD: l = kld_v1(gp, gt, q); break;
        case JDET_GD1_BCD: l = bcd_v1(gp, gt, q); break;
        default: l = kfiou(d, t, gp, gt, q); break;  // JDET_KFIOU
      }
      acc += l.v;
#pragma unroll
      for (int k = 0; k < 5; k++) g[k] = l.g[k];
    }
#pragma unroll
    for (int k = 0; k < 5; k++) grad[r * 5 + k] = g[k];
  }
  const float sum = jdet_block_sum4(acc, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

}  // namespace

JDET_API int jdet_gaussian_loss_level(const float* pred, const float* target, long target_rows_per_block,
                                      long target_block_stride, const float* weight, long weight_rows_per_block,
                                      long weight_block_stride, const float* anchors, long anchor_rows, long rows,
                                      const jdet_gaussian_loss_params_t* params, const float* avg_factor,
                                      float loss_weight, float* loss, float* grad_pred, void* workspace,
                                      size_t workspace_bytes, jdet_stream_t stream) {
  if (rows <= 0 || !params || !loss || !avg_factor || !pred || !target || !grad_pred || !workspace)
    return JDET_E_BADARG;
  const jdet_gaussian_loss_params_t q = *params;
  if (q.kind < JDET_GD_GWD || q.kind > JDET_KFIOU || q.fun < JDET_GD_FUN_NONE || q.fun > JDET_GD_FUN_EXP)
    return JDET_E_BADARG;
  if ((q.decode_pred || q.decode_target) && (!anchors || anchor_rows <= 0 || !(q.wh_ratio_clip > 0.f)))
    return JDET_E_BADARG;
  if (target_rows_per_block <= 0 || target_block_stride < 0 ||
      (weight && (weight_rows_per_block <= 0 || weight_block_stride < 0)))
    return JDET_E_BADARG;
  if (workspace_bytes < jdet_sigmoid_focal_loss_workspace()) return JDET_E_WORKSPACE;
  Vec5 m, s;
  for (int k = 0; k < 5; k++) {
    m.v[k] = q.means[k];
    s.v[k] = q.stds[k];
  }
  const float max_ratio = (q.decode_pred || q.decode_target) ? fabsf(logf(q.wh_ratio_clip)) : 0.f;
  hipStream_t st = (hipStream_t)stream;
  const int grid = jdet_loss_grid(rows, 256);
  hipLaunchKernelGGL(gaussian_loss_kernel, dim3(grid), dim3(256), 0, st, pred, target,
                     Blocked{target_rows_per_block, target_block_stride}, weight,
                     Blocked{weight ? weight_rows_per_block : 1, weight ? weight_block_stride : 0},
                     (q.decode_pred || q.decode_target) ? anchors : nullptr, anchor_rows > 0 ? anchor_rows : 1, rows,
                     q, m, s, max_ratio, grad_pred, (float*)workspace);
  if (int e = jdet_launch_status()) return e;
  return jdet_sum_partials<true>((const float*)workspace, grid, avg_factor, loss_weight, loss, st);
}
