/* jdet_hip_strip.h -- the strip-convolution entry point of libjdet_hip.so (csrc/strip_conv.hip): the 1 x K and K x 1
 * depthwise layers of the StripNet backbones (models/backbones/stripnet.py).  Conventions, error codes and jdet_stream_t
 * are those of jdet_hip.h: nothing is launched on an argument error, inputs are never written, every output element is
 * written, the entry point neither synchronises nor allocates.  It is deterministic: no atomics, every sum in a fixed
 * order, two runs agree bit for bit.
 *
 * LAYOUT.  fp32 and channels-last: activations (N, H, W, C) in memory, the strip's weights packed (K, C) -- what
 * jdet_hip_lsk.h calls (KH, KW, C) with KH or KW equal to 1.  x, w, bias (unless null) and y must be 16-byte aligned
 * (JDET_E_BADARG otherwise): all accesses along C are 16 bytes wide.  y must not overlap x.
 *
 * ARGUMENTS.  axis 0: a K x 1 kernel along H; axis 1: a 1 x K kernel along W.  Stride 1, dilation 1, padding
 * (K - 1) / 2 on the strip axis and none on the other.  Dimensions below 1, K < 1, an axis outside {0, 1} and a null x, w
 * or y are JDET_E_BADARG.  C % 4 != 0, an even K, K > 1023 and an activation of 2^31 elements or more (N * H * W * C:
 * indexing is 32-bit) are JDET_E_UNSUPPORTED.  Maps of any size are correct, a strip axis shorter than K and of length 1
 * included: every window position is bounds-checked.
 *
 * THE ORDER (the library is built with -ffp-contract=off), for the output at position o of the strip axis:
 *   acc = bias[c], or 0.f without a bias;
 *   for k = 0 .. K - 1:
 *     i = o + k - (K - 1) / 2; a tap outside the map is SKIPPED (not added as a zero);
 *     acc = acc + (w[k, c] * x[.., i, .., c])             -- a float32 multiply, then a float32 add
 *   y = acc.
 * That is the order of jdet_dwconv_nhwc_forward (jdet_hip_lsk.h) with (KH, KW) = (K, 1) on axis 0 or (1, K) on axis 1,
 * pad (K - 1) / 2 on that axis, dilation 1 and act 0: THE TWO ENTRY POINTS ARE BIT-IDENTICAL (tests/lsk_ref.py restates
 * the order in float32).  They differ in the memory traffic: a thread here owns 4 consecutive outputs of the strip axis and
 * walks their shared window of K + 3 inputs once, so it loads K + 3 values of x where the generic kernel loads 4 K.
 * The data gradient of a strip convolution is this same entry point on the weights flipped along K, without a bias; its
 * weight and bias gradients are jdet_dwconv_nhwc_wgrad with KH x KW = K x 1 or 1 x K.
 */
#ifndef JDET_HIP_STRIP_H_
#define JDET_HIP_STRIP_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y (N, H, W, C) = stripconv(x (N, H, W, C), w (K, C)) + bias (C) | NULL; axis 0: a K x 1 kernel along H, axis 1: 1 x K along W;
 * stride 1, dilation 1, pad (K - 1) / 2 on the strip axis. */
int jdet_strip_conv_forward(const float* x, const float* w, const float* bias, int N, int H, int W, int C, int K,
                            int axis, float* y, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_STRIP_H_ */
