// RepPoints convex GIoU with the gradient w.r.t. the 9 points, for gfx950.
//
// Reference (CUDA only): ops/reppoints_convex_iou/convex_giou.py:L29-47 (`reppoints_convex_giou`: aligned pairs,
// output (N, 19) = 18 point gradients + the GIoU) and convex_giou_kernel.cu:L725-821 (`devrIoU`): hull of the 9 points
// (Jarvis, L613-723), intersection area with the quadrilateral and its gradient through the clipping (L117-447),
// hull area and its gradient (L68-115), area of the hull of both polygons' vertices and its gradient (L539-610), then
//     giou = I/U - (C - U)/C,   U = |A| + |B| - I,
//     d giou = (U + I)/U^2 dI - I/U^2 dA - (dI - dA)/C - U/C^2 dC                            (L782-790)
// with the gradient of a point that is not a hull vertex zero.  The reference derives the ~40 partial derivatives by
// hand, one CUDA thread per pair with 100-point local arrays.
//
// MI355X design (not a translation): the value is a composition of differentiable pieces selected by discrete decisions
// (which points are hull vertices, which edges cross), so the gradient is taken by FORWARD-MODE DUAL NUMBERS: half a
// wave (32 lanes) per pair, lane j < 18 carries the dual seed d/d(coordinate j), every lane runs the SAME control flow
// (decisions look at the value parts only, which are identical across the lanes of a pair), and the dual part of the
// final GIoU in lane j IS the j-th partial derivative -- 18 derivatives in the time of one evaluation, no hand-written
// derivative code to get wrong.  Geometry: Andrew monotone-chain hulls (the 9 points; the union of both polygons'
// vertices), Sutherland-Hodgman clipping of the convex hull by the convex quadrilateral, shoelace areas; all in double
// like the reference.  Collinear / duplicate hull candidates are dropped (they change neither the areas nor, almost
// everywhere, the derivatives).
#include "convex_giou.h"

namespace {

// 32 lanes per pair: lane j < 18 differentiates w.r.t. coordinate j of the point set; lane 18 stores the value
__global__ __launch_bounds__(64) void convex_giou_kernel(const float* __restrict__ pointsets,
                                                        const float* __restrict__ polygons, int N,
                                                        float* __restrict__ out) {
  const int pair = blockIdx.x * 2 + (threadIdx.x >> 5);
  const int j = threadIdx.x & 31;
  if (pair >= N || j > 18) return;
  const float* ps = pointsets + (size_t)pair * 18;
  const float* q = polygons + (size_t)pair * 8;
  const Dual giou = jdet_convex_giou_dual([&](int i) { return ps[i]; }, [&](int i) { return q[i]; }, j);
  float* o = out + (size_t)pair * 19;
  if (j < 18) o[j] = (float)giou.d;
  else o[18] = (float)giou.v;
}

}  // namespace

JDET_API int jdet_convex_giou(const float* pointsets, const float* polygons, int N, float* out, jdet_stream_t stream) {
  if (N < 0) return JDET_E_BADARG;
  if (N == 0) return JDET_OK;
  if (!pointsets || !polygons || !out) return JDET_E_BADARG;
  hipLaunchKernelGGL(convex_giou_kernel, dim3((unsigned)((N + 1) / 2)), dim3(64), 0, (hipStream_t)stream, pointsets,
                     polygons, N, out);
  return jdet_launch_status();
}
