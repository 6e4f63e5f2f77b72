// The profiling build of the conv_bn kernel (../conv_bn_kernel.h with STAMPS = true), outside the product library: every
// workgroup writes wall_clock64() at its start, when it enters / leaves the K loop and at its end, plus HW_ID / XCC_ID /
// blockIdx, over the first 16 words of its tile's first output row (those words are garbage afterwards).
// scripts/r6_conv_stamps.py reads them; the prologue / epilogue finding of DESIGN.md 3.6 came from it.
#include "conv_bn_kernel.h"

#include "jdet_experimental.h"

// Always conv_bn_kernel<64, 32, 1, 2, true>: the 64 x 64 tile, 32-deep K steps, one wave group, operand tiles two steps
// ahead; no workspace, no plan.  JDET_E_UNSUPPORTED unless Cin % 32 == 0 and the product's own limits hold.
JDET_API int jdet_conv_bn_forward_stamps(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout,
                                         int R, int stride, const jdet_conv_epilogue_t* epilogue, float* y_nhwc,
                                         jdet_stream_t stream) {
  CbArgs a{};
  const int bad = cb_check_args(x_nhwc, N, H, W, Cin, w_krsc, Cout, R, stride, epilogue, y_nhwc, a);
  if (bad) return bad;
  if (Cin % 32 != 0) return JDET_E_UNSUPPORTED;
  if (N == 0) return JDET_OK;
  const long M = (long)N * a.Ho * a.Wo;
  const long tiles = ((M + 63) / 64) * ((Cout + 63) / 64);
  hipLaunchKernelGGL((conv_bn_kernel<64, 32, 1, 2, true>), dim3((unsigned)tiles, 1), dim3(256), 0, (hipStream_t)stream, a);
  return jdet_launch_status();
}
