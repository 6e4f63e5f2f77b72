// Polygon IoU loss of rotated box pairs for gfx950 (MI355X): forward and gradient in one launch.
//
// Reference semantics (a differentiable Jittor tensor program of ~60 small ops over (P, 24, 2) point sets + a scan):
//   python/jdet/models/losses/poly_iou_loss.py:L11-36    shoelace, convex_areas (convex_sort + gather)
//   python/jdet/models/losses/poly_iou_loss.py:L39-86    poly_intersection (16 edge pairs, two inside masks)
//   python/jdet/models/losses/poly_iou_loss.py:L97-123   iou, clamp, -log / 1 - iou, weight
// The operations, their order and the gradient rules are stated in include/jdet_hip.h.
//
// MI355X design.  One thread per row; a row is a few hundred flops on 24 points.  The 24 points and masks of a lane live
// in LDS at [k * 64 + lane] (conflict-free, dynamic indexing without scratch); the scan's sort keys and the hull indices
// are thread-private.  The backward pass needs nothing stored: it walks the hull indices once more, recomputing the
// four numbers of an intersection point from the eight vertices kept in registers.  A row of weight 0 leaves at once:
// FCOS positives are spatially clustered, so in the dense call over all points most wavefronts leave whole, and the
// step has no nonzero() host round trip.  Measured at 10 % positives: 2.26 ms against the gathered route's 2.84 ms,
// forward + backward with the decoding ops around it (profiles/fcos.md).
#include "common.h"
#include "graham_scan.h"
#include "jdet_hip.h"

namespace {

constexpr int kPts = 24;     // 16 intersections, 4 pred vertices, 4 target vertices
constexpr int kLanes = 64;

__device__ __forceinline__ void obb_corners(const float* b, float* x, float* y) {
  float sn, cs;
  sincosf(b[4], &sn, &cs);
  const float v1x = b[2] / 2 * cs, v1y = -b[2] / 2 * sn;
  const float v2x = -b[3] / 2 * sn, v2y = -b[3] / 2 * cs;
  x[0] = b[0] + v1x + v2x; y[0] = b[1] + v1y + v2y;
  x[1] = b[0] + v1x - v2x; y[1] = b[1] + v1y - v2y;
  x[2] = b[0] - v1x - v2x; y[2] = b[1] - v1y - v2y;
  x[3] = b[0] - v1x + v2x; y[3] = b[1] - v1y + v2y;
}

__global__ __launch_bounds__(kLanes) void poly_iou_loss_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ target,
                                                              const float* __restrict__ weight, long P, int linear,
                                                              float eps, float* __restrict__ loss,
                                                              float* __restrict__ grad) {
  __shared__ float s_x[kPts * kLanes], s_y[kPts * kLanes], s_m[kPts * kLanes];
  const int lane = threadIdx.x;
  const long r = (long)blockIdx.x * kLanes + lane;
  if (r >= P) return;                                      // (no barrier below: a lane only touches its own column)
  const float wt = weight ? weight[r] : 1.f;
  float* g = grad + r * 5;
  if (wt == 0.f) {
    loss[r] = 0.f;
#pragma unroll
    for (int k = 0; k < 5; k++) g[k] = 0.f;
    return;
  }
  float a[5], b[5];
#pragma unroll
  for (int k = 0; k < 5; k++) a[k] = pred[r * 5 + k], b[k] = target[r * 5 + k];
  const float area1 = a[2] * a[3], area2 = b[2] * b[3];
  float ax[4], ay[4], bx[4], by[4];
  obb_corners(a, ax, ay);
  obb_corners(b, bx, by);
  float* X = s_x + lane;
  float* Y = s_y + lane;
  float* M = s_m + lane;

  float in1[4] = {0.f, 0.f, 0.f, 0.f}, in2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float x1 = ax[i], y1 = ay[i], x2 = ax[(i + 1) & 3], y2 = ay[(i + 1) & 3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float x3 = bx[j], y3 = by[j], x4 = bx[(j + 1) & 3], y4 = by[(j + 1) & 3];
      const float num = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4);
      const float den_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4);
      const float den_u = (x2 - x1) * (y1 - y3) - (y2 - y1) * (x1 - x3);
      const float t = den_t / num, u = den_u / num;
      const bool hit = t > 0.f && t < 1.f && u > 0.f && u < 1.f;
      const float te = den_t / (num + eps);
      X[(i * 4 + j) * kLanes] = x1 + te * (x2 - x1);
      Y[(i * 4 + j) * kLanes] = y1 + te * (y2 - y1);
      M[(i * 4 + j) * kLanes] = hit ? 1.f : 0.f;
      in1[i] += 0.5f * fabsf((x3 - x1) * (y4 - y1) - (y3 - y1) * (x4 - x1));
      in2[j] += 0.5f * fabsf((x1 - x3) * (y2 - y3) - (x2 - x3) * (y1 - y3));
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    X[(16 + i) * kLanes] = ax[i];
    Y[(16 + i) * kLanes] = ay[i];
    M[(16 + i) * kLanes] = fabsf(in1[i] - area2) < 1e-3f * area2 ? 1.f : 0.f;
    X[(20 + i) * kLanes] = bx[i];
    Y[(20 + i) * kLanes] = by[i];
    M[(20 + i) * kLanes] = fabsf(in2[i] - area1) < 1e-3f * area1 ? 1.f : 0.f;
  }

  int idx[kPts + 1];
  const int m = jdet_graham_scan<kPts>([&](int i) { return X[i * kLanes]; }, [&](int i) { return Y[i * kLanes]; },
                                       [&](int i) { return M[i * kLanes]; }, kPts, 1,
                                       [&](int i) -> int& { return idx[i]; });
  // shoelace over the closed hull; the -1 slots gather the origin and add exact zeros (poly_iou_loss.py:L19-36)
  float S = 0.f;
  for (int k = 0; k < m; k++) {
    const int p = idx[k], q = idx[k + 1];
    S += X[p * kLanes] * Y[q * kLanes] - Y[p * kLanes] * X[q * kLanes];
  }
  const float overlap = 0.5f * fabsf(S);
  const float uni = area1 + area2 - overlap + eps;
  const float raw = overlap / uni;
  const float iou = fmaxf(raw, eps);
  loss[r] = (linear ? 1.f - iou : -logf(iou)) * wt;

  // ---- gradient
  float g_iou = (linear ? -1.f : -1.f / iou) * wt;
  if (!(raw >= eps)) g_iou = 0.f;                          // the clamp is active
  const float g_ov = g_iou * (1.f / uni + overlap / (uni * uni));
  const float g_a1 = -g_iou * overlap / (uni * uni);
  const float sgn = S > 0.f ? 1.f : (S < 0.f ? -1.f : 0.f);
  const float g_S = g_ov * 0.5f * sgn;
  float gx[4] = {0.f, 0.f, 0.f, 0.f}, gy[4] = {0.f, 0.f, 0.f, 0.f};   // on the pred vertices
  if (g_S != 0.f) {
    for (int k = 0; k < m; k++) {
      const int p = idx[k];
      if (p >= 20) continue;                               // a target vertex
      const int pv = idx[k == 0 ? m - 1 : k - 1], nx = idx[k + 1 == m ? 0 : k + 1];
      const float gX = g_S * (Y[nx * kLanes] - Y[pv * kLanes]), gY = g_S * (X[pv * kLanes] - X[nx * kLanes]);
      if (p >= 16) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
          gx[v] += v == p - 16 ? gX : 0.f;
          gy[v] += v == p - 16 ? gY : 0.f;
        }
        continue;
      }
      const int i = p >> 2, j = p & 3, i2 = (i + 1) & 3, j2 = (j + 1) & 3;
      float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, x3 = 0.f, y3 = 0.f, x4 = 0.f, y4 = 0.f;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        x1 = v == i ? ax[v] : x1; y1 = v == i ? ay[v] : y1;
        x2 = v == i2 ? ax[v] : x2; y2 = v == i2 ? ay[v] : y2;
        x3 = v == j ? bx[v] : x3; y3 = v == j ? by[v] : y3;
        x4 = v == j2 ? bx[v] : x4; y4 = v == j2 ? by[v] : y4;
      }
      const float ca = y3 - y4, cb = x3 - x4;
      const float num = (x1 - x2) * ca - (y1 - y2) * cb;
      const float den_t = (x1 - x3) * ca - (y1 - y3) * cb;
      const float ne = num + eps;
      const float te = den_t / ne;
      // point = v1 + te * (v2 - v1);  d te / d v = (d den_t / d v - te * d num / d v) / ne
      const float g_t = gX * (x2 - x1) + gY * (y2 - y1);
      const float gx1 = gX * (1.f - te) + g_t * (ca - te * ca) / ne;
      const float gy1 = gY * (1.f - te) + g_t * (te * cb - cb) / ne;
      const float gx2 = gX * te + g_t * (te * ca) / ne;
      const float gy2 = gY * te - g_t * (te * cb) / ne;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        gx[v] += (v == i ? gx1 : 0.f) + (v == i2 ? gx2 : 0.f);
        gy[v] += (v == i ? gy1 : 0.f) + (v == i2 ? gy2 : 0.f);
      }
    }
  }
  // vertices -> (xc, yc, w, h, theta): P0 = c + v1 + v2, P1 = c + v1 - v2, P2 = c - v1 - v2, P3 = c - v1 + v2 with
  // v1 = (w/2 cos, -w/2 sin), v2 = (-h/2 sin, -h/2 cos)
  float sn, cs;
  sincosf(a[4], &sn, &cs);
  const float g1x = gx[0] + gx[1] - gx[2] - gx[3], g1y = gy[0] + gy[1] - gy[2] - gy[3];
  const float g2x = gx[0] - gx[1] - gx[2] + gx[3], g2y = gy[0] - gy[1] - gy[2] + gy[3];
  g[0] = gx[0] + gx[1] + gx[2] + gx[3];
  g[1] = gy[0] + gy[1] + gy[2] + gy[3];
  g[2] = 0.5f * (g1x * cs - g1y * sn) + g_a1 * a[3];
  g[3] = 0.5f * (-g2x * sn - g2y * cs) + g_a1 * a[2];
  g[4] = 0.5f * (a[2] * (-g1x * sn - g1y * cs) + a[3] * (-g2x * cs + g2y * sn));
}

}  // namespace

JDET_API int jdet_poly_iou_loss(const float* pred, const float* target, const float* weight, long P, int linear,
                                float eps, float* loss, float* grad_pred, jdet_stream_t stream) {
  if (P < 0 || !(eps > 0.f)) return JDET_E_BADARG;
  if (P == 0) return JDET_OK;
  if (!pred || !target || !loss || !grad_pred) return JDET_E_BADARG;
  if ((P + kLanes - 1) / kLanes > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;
  hipLaunchKernelGGL(poly_iou_loss_kernel, dim3((unsigned)((P + kLanes - 1) / kLanes)), dim3(kLanes), 0,
                     (hipStream_t)stream, pred, target, weight, P, linear ? 1 : 0, eps, loss, grad_pred);
  return jdet_launch_status();
}
