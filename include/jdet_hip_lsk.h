/* jdet_hip_lsk.h -- the depthwise-convolution and kernel-selection entry points of libjdet_hip.so (csrc/dwconv.hip,
 * csrc/lsk_select.hip): the hot path of the LSKNet backbones (models/backbones/lsknet.py).  Conventions, error codes and
 * jdet_stream_t are those of jdet_hip.h: nothing is launched on an argument error, inputs are never written, every output
 * element is written (the one accumulating entry point says so), no entry point synchronises or allocates.  All of them
 * are deterministic: no atomics, every sum in a fixed order, two runs agree bit for bit.
 *
 * LAYOUT.  Everything is fp32 and channels-last: activations (N, H, W, C) in memory, depthwise weights packed (KH, KW, C)
 * (the host layer packs -- and, for the data gradient, flips -- a tensor of at most KH * KW * C floats with torch ops).
 * Every tensor pointer of the dwconv entry points must be 16-byte aligned (JDET_E_BADARG otherwise): all accesses along C
 * are 16 bytes wide.  The selection entry points take any Ch >= 1; they use 16-byte accesses when Ch % 4 == 0 and every
 * pointer is 16-byte aligned, 4-byte accesses otherwise (same arithmetic, same order).
 *
 * INDEXING IS 32-BIT.  An activation of 2^31 elements or more (N * H * W * C, for the selection N * H * W * 2 * Ch) is
 * JDET_E_UNSUPPORTED, and so is a selection map of 2^25 pixels or more.
 *
 * GEOMETRY.  Stride 1 and "same" padding only: 2 * pad == dil * (K - 1) on both axes, anything else is
 * JDET_E_UNSUPPORTED, as are C % 4 != 0 and K or dil above 1024.  (Rectangular kernels are taken: 1 x 19 and 19 x 1
 * strips.)  Dimensions below 1, pad < 0, dil < 1, an unknown act and null pointers are JDET_E_BADARG.  Maps of any size
 * are correct, H or W of 1 and maps smaller than the dilated footprint included: every tap is bounds-checked.
 *
 * THE ORDER OF THE CONVOLUTION (restated in float32 by tests/lsk_ref.py; the library is built with -ffp-contract=off):
 *   acc = bias[c], or 0.f without a bias;
 *   for kh = 0 .. KH - 1 (outer), for kw = 0 .. KW - 1 (inner):
 *     ih = h + kh * dil_h - pad_h, iw = w + kw * dil_w - pad_w; a tap outside the map is SKIPPED (not added as a zero);
 *     acc = acc + (w[kh, kw, c] * x[n, ih, iw, c])        -- a float32 multiply, then a float32 add
 *   y = acc (act 0) or gelu(acc) = 0.5 * acc * (1 + erf(acc / sqrt(2))) (act 1, float32, the device library's erff).
 * The data gradient of such a convolution is this same entry point on the weights flipped along KH and KW, without a bias.
 *
 * THE ORDER OF THE WEIGHT GRADIENT.  R = N * H image rows, S = min(R, 512) slabs of L = ceil(R / S) consecutive rows
 * (slab s: rows s * L .. min(R, (s + 1) * L) - 1; a slab may be empty).  First stage: the partial sum of (slab, tap, c)
 * starts at 0.f and adds g[n, h, w, c] * x[n, h + kh * dil_h - pad_h, w + kw * dil_w - pad_w, c] (a multiply, then an add)
 * over the slab's rows in increasing order and, inside a row, over w in increasing order, positions whose tap is outside
 * the map skipped; the bias partial adds g[n, h, w, c] in the same order.  Second stage, per (tap, c): lane l of one
 * 64-lane wave starts at 0.f and adds the partials of slabs l, l + 64, l + 128, ...; the 64 lane sums are then combined by
 * the xor butterfly v = v + v(lane ^ off), off = 32, 16, 8, 4, 2, 1.  (Longest chain of additions: W * L + 8 + 6.)
 *
 * SELECTION.  a1, a2: (N, H, W, Ch); concat(a1, a2) has 2 Ch channels, channel j < Ch from a1, else a2[j - Ch].
 * A pixel is worked by a group of G lanes (G = 4, 16 or 64: the smallest that covers the pixel's accesses, else 64): lane l
 * of the group takes the access units l, l + G, ... (a unit is 4 consecutive channels on the 16-byte route, 1 on the other)
 * in increasing order -- a sum starts at 0.f and adds the unit's channels in increasing order -- and the G lane results
 * are combined by the xor butterfly off = G / 2, ..., 1.  The maximum is exact in any order; its index is the FIRST
 * channel attaining it (what torch.max(dim=1) returns and differentiates through).  Inputs with NaN give an unspecified
 * maximum.
 */
#ifndef JDET_HIP_LSK_H_
#define JDET_HIP_LSK_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JDET_DWCONV_ACT_NONE 0
#define JDET_DWCONV_ACT_GELU 1
#define JDET_DWCONV_MAX_SLABS 512

/* y (N, H, W, C) = act(dwconv(x (N, H, W, C), w (KH, KW, C)) + bias (C) | NULL), in the order above. */
int jdet_dwconv_nhwc_forward(const float* x, const float* w, const float* bias, int N, int H, int W, int C, int KH,
                             int KW, int pad_h, int pad_w, int dil_h, int dil_w, int act, float* y,
                             jdet_stream_t stream);

/* bytes of the weight gradient's workspace: S * (KH * KW + 1) * C floats; 0 for arguments the entry point refuses */
size_t jdet_dwconv_nhwc_wgrad_workspace(int N, int H, int W, int C, int KH, int KW);

/* gw (KH, KW, C) and, unless null, gb (C): the gradients of the packed weights and of the bias, given x and the gradient g
 * (N, H, W, C) of the convolution's output, in the two-stage order above.  workspace: 16-byte aligned, any content.
 * A workspace_bytes below the query is JDET_E_WORKSPACE and leaves gw and gb untouched. */
int jdet_dwconv_nhwc_wgrad(const float* x, const float* g, int N, int H, int W, int C, int KH, int KW, int pad_h,
                           int pad_w, int dil_h, int dil_w, float* gw, float* gb, void* workspace,
                           size_t workspace_bytes, jdet_stream_t stream);

/* g_z (N, H, W, C) = g_y * gelu'(z), gelu'(z) = Phi(z) + z * phi(z) = 0.5 * (1 + erf(z / sqrt(2))) + z * exp(-z^2 / 2) /
 * sqrt(2 pi), with z = dwconv(x) + bias recomputed from x in the forward's order (the fused forward never stores it).
 * bias may be null. */
int jdet_dwconv_gelu_backward(const float* x, const float* w, const float* bias, const float* g_y, int N, int H, int W,
                              int C, int KH, int KW, int pad_h, int pad_w, int dil_h, int dil_w, float* g_z,
                              jdet_stream_t stream);

/* agg (N, H, W, 2): [..., 0] = (sum over the 2 Ch channels of concat(a1, a2)) / (2 Ch), [..., 1] = their maximum;
 * argmax (N * H * W) int32: the first channel of the concatenation attaining it. */
int jdet_lsk_squeeze_forward(const float* a1, const float* a2, int N, int H, int W, int Ch, float* agg, int* argmax,
                             jdet_stream_t stream);

/* ACCUMULATES onto the contents of g_a1, g_a2 (N, H, W, Ch): every channel gains g_agg[..., 0] / (2 Ch), the argmax
 * channel then g_agg[..., 1] (two separate additions, in that order).  An argmax outside [0, 2 Ch) adds no maximum. */
int jdet_lsk_squeeze_backward(const float* g_agg, const int* argmax, int N, int H, int W, int Ch, float* g_a1,
                              float* g_a2, jdet_stream_t stream);

/* out (N, H, W, Ch) = (a1 * sig[..., 0]) + (a2 * sig[..., 1]): two multiplies and one add; sig (N, H, W, 2). */
int jdet_lsk_select_forward(const float* a1, const float* a2, const float* sig, int N, int H, int W, int Ch, float* out,
                            jdet_stream_t stream);

/* g_a1 = g * sig[..., 0], g_a2 = g * sig[..., 1]; g_sig (N, H, W, 2): [..., k] = sum over the pixel's Ch channels of
 * g * a_k, in the group order above. */
int jdet_lsk_select_backward(const float* g, const float* a1, const float* a2, const float* sig, int N, int H, int W,
                             int Ch, float* g_a1, float* g_a2, float* g_sig, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_LSK_H_ */
