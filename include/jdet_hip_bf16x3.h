/* jdet_hip_bf16x3.h -- the 3x3 convolution forward of libjdet_hip.so that runs fp32 data on the bf16 matrix pipe through
 * an exact three-way split (csrc/conv_bf16x3.hip).
 *
 * Why a header of its own: the names of jdet_hip.h are pinned as a set by the buffer-contract table (tests/abi_cases.py),
 * as jdet_hip_rows_fwd.h explains for itself.  These entry points are exported by the same library, follow every
 * convention stated at the top of jdet_hip.h (status codes, no synchronisation, no allocation, inputs never written, the
 * stream last) and are checked against BF16X3_SIGNATURES of jdet_amd/_lib.py by tests/test_conv_bf16x3_cpu.py.
 *
 * Numerics: every fp32 input and weight x is split by truncation into three bf16 values a1 + a2 + a3 == x (exactly);
 * six bf16 products per operand pair (a3b1, a1b3, a2b2, a2b1, a1b2, a1b1, small terms first within a 16-deep K block)
 * go into one fp32 accumulator per output.  The result is as close to the exact sum as an fp32 fma chain's (the bound of
 * jdet_conv3x3_igemm_forward's tests holds with the same headroom), but not bit-equal to that kernel's.  Non-finite
 * inputs give non-finite outputs, possibly NaN where jdet_conv3x3_igemm_forward gives Inf (Inf splits into Inf, NaN, NaN).
 */
#ifndef JDET_HIP_BF16X3_H_
#define JDET_HIP_BF16X3_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cin % 32 == 0, any Cout > 0: what the entry point below takes (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_bf16x3_supported(int Cin, int Cout);

/* y[m, co] = [relu](sum over taps and ci of x[nbr(m, tap), ci] * w[co, tap, ci] + bias[co]) * rowmask[m]: 3x3 / stride 1 /
 * pad 1, channels last, neighbours outside the image contribute zero.  The plain form of jdet_conv3x3_igemm_forward
 * with that entry point's arguments: x (N,H,W,Cin), w (Cout,3,3,Cin), bias (Cout) or null, rowmask (N*H*W) or null, y
 * (N,H,W,Cout), every element written.  One launch of 128 x 128 output tiles, no workspace, nothing read back, no launch
 * shape taken from device data.  N == 0 is a no-op.  x and w 16-byte aligned, y 4-byte aligned (else JDET_E_BADARG);
 * N*H*W * max(Cin, Cout) < 2^30 and Cout * 9 * Cin < 2^30 (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_bf16x3_forward(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout,
                                const float* bias, int relu, const float* rowmask, float* y_nhwc, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_BF16X3_H_ */
