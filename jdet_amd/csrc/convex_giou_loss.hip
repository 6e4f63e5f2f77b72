// Dense convex GIoU loss of RepPoints point sets for gfx950 (MI355X): forward and gradient of all rows in one launch.
//
// Reference semantics: python/jdet/models/losses/convex_giou_loss.py:L10-53 (ConvexGIoULossFunction.execute) on the
// rows that python/jdet/models/roi_heads/rotated_reppoints_head.py:L612-634 gathers with nonzero() and divides by
// normalize_term.  The operations and their order are stated in include/jdet_hip.h.
//
// MI355X design.  The head's nonzero() is one host round trip per (level, stage), ten per step; here every row of a
// stage goes through one launch and a row of weight 0 leaves at once.  Half a wavefront per row, as in
// csrc/convex_giou.hip: lane j < 18 carries the dual seed of coordinate j, lane 18 the value, all through the shared
// jdet_convex_giou_dual.  The "any component > 1" rule of a row is one ballot over its half of the wavefront.
#include "convex_giou.h"
#include "jdet_hip.h"

namespace {

__global__ __launch_bounds__(64) void convex_giou_loss_kernel(const float* __restrict__ pred,
                                                             const float* __restrict__ target,
                                                             const float* __restrict__ weight,
                                                             const float* __restrict__ norm, long P,
                                                             float* __restrict__ loss, float* __restrict__ grad) {
  const long row = (long)blockIdx.x * 2 + (threadIdx.x >> 5);
  const int j = threadIdx.x & 31;
  if (row >= P || j > 18) return;
  const float wt = weight[row];
  if (wt == 0.f) {
    if (j < 18) grad[row * 18 + j] = 0.f;
    else loss[row] = 0.f;
    return;
  }
  const float nm = norm[row];
  const float* ps = pred + row * 18;
  const float* q = target + row * 8;
  const Dual giou = jdet_convex_giou_dual([&](int i) { return ps[i] / nm; }, [&](int i) { return q[i] / nm; }, j);
  float g = (float)giou.d * wt;
  // the live lanes of this row's half: j <= 18; lane 18 holds no gradient component
  const unsigned long long over = __ballot(j < 18 && g > 1.f);
  const bool invalid = ((over >> (threadIdx.x & 32)) & 0x3FFFFull) != 0ull;
  if (j < 18) {
    if (invalid) g = 1e-6f;
    grad[row * 18 + j] = -g / nm;
  } else {
    loss[row] = (1.f - (float)giou.v) * wt;
  }
}

}  // namespace

JDET_API int jdet_convex_giou_loss(const float* pred, const float* target, const float* weight, const float* norm,
                                   long P, float* loss, float* grad_pred, jdet_stream_t stream) {
  if (P < 0) return JDET_E_BADARG;
  if (P == 0) return JDET_OK;
  if (!pred || !target || !weight || !norm || !loss || !grad_pred) return JDET_E_BADARG;
  if ((P + 1) / 2 > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;
  hipLaunchKernelGGL(convex_giou_loss_kernel, dim3((unsigned)((P + 1) / 2)), dim3(64), 0, (hipStream_t)stream, pred,
                     target, weight, norm, P, loss, grad_pred);
  return jdet_launch_status();
}
