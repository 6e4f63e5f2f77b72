/* jdet_hip_rows_fwd.h -- the row-sparse convolution FORWARD of libjdet_hip.so (csrc/conv_rows.hip).
 *
 * Why a header of its own: the names of include/jdet_hip_rows.h are pinned as a set by tests/test_conv_rows_cpu.py, as
 * the names of jdet_hip.h are by the buffer-contract table (tests/abi_cases.py).  These entry points arrived later: they
 * are exported by the same library, follow every convention stated at the top of jdet_hip.h (status codes, no
 * synchronisation, no allocation, inputs never written, the stream last) and have their contract rows in
 * tests/test_gpu_conv_rows_fwd_abi.py.  When the contract table is next revised, fold this file into jdet_hip.h together
 * with jdet_hip_rows.h (and ROWS_FWD_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 *
 * What they are for: in training, the output of the S2ANet head's ODM regression tower (models/roi_heads/
 * s2anet_head.py:L127-205, odm_reg_convs -> odm_reg) is read by the smooth-L1 loss only, and that loss weighs every
 * anchor that is not positive with 0 (L300-340).  With S0 the positive position rows, the 3x3 prediction layer needs its
 * input on the 3x3 dilation of S0 and the tower layer before it on the dilation of that: the two entry points below
 * make those lists from a flag byte per position and compute conv + bias + ReLU on the listed rows only.  No value is
 * read back to the host and no launch shape depends on device data: every list has capacity P = N*H*W rows, so there is
 * no overflow path, and a dense list is computed correctly (only slower than by the dense kernel).
 */
#ifndef JDET_HIP_ROWS_FWD_H_
#define JDET_HIP_ROWS_FWD_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Three ascending row lists from one flag byte per position (non-zero = listed), in four launches (the dilation and
 * list kernels of jdet_rows_nonzero).  Comes in place of nothing the reference has.
 *   flags          (P) bytes, read only
 *   rows           (P) int32: the flagged positions, ascending, in [0, counts[0]); -1 in the rest
 *   rows_dilated   (P) int32: the positions whose 3x3 neighbourhood (n, y + dy, x + dx), taken inside the same image --
 *                  never across a row end or an image boundary -- holds a flagged one, in [0, counts[1]); -1 in the rest
 *   rows_dilated2  (P) int32: the same dilation applied to rows_dilated's set, in [0, counts[2]); -1 in the rest
 *   counts         3 int32: the three list lengths
 * P < 2^30, else JDET_E_UNSUPPORTED.  workspace: jdet_rows_from_flags_workspace(N, H, W) bytes, 4-byte aligned, may
 * hold anything; fewer bytes: JDET_E_WORKSPACE. */
size_t jdet_rows_from_flags_workspace(int N, int H, int W);
int jdet_rows_from_flags(const uint8_t* flags, int N, int H, int W, int32_t* rows, int32_t* rows_dilated,
                         int32_t* rows_dilated2, int32_t* counts, void* workspace, size_t workspace_bytes,
                         jdet_stream_t stream);

/* Cin % 16 == 0 and Cout % 16 == 0: what the entry point below takes (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_rows_forward_supported(int Cin, int Cout);

/* y[r, co] = [relu](sum over taps and ci of x[nbr(r, tap), ci] * w[co, tap, ci] + bias[co]) * rowmask[r] for every r
 * of the list: 3x3 / stride 1 / pad 1, neighbours outside the image contribute zero.  Replaces
 * jdet_conv3x3_igemm_forward (plain form) where only the listed rows of y are read: w (Cout,3,3,Cin), bias (Cout) or
 * null, rowmask (P) or null with that entry point's meaning (a listed row whose mask is 0 is written as 0).  Rows of y
 * that are not listed are left alone, or -- zero_first != 0 -- zero-filled by a launch of this call, so that y
 * (N,H,W,Cout) is fully written.  rows / count: device pointers (a list of jdet_rows_from_flags and its count);
 * entries past *count are not read; *count == 0 computes nothing.  The grid is fixed by P (P / 64 row tiles); tiles past
 * *count leave at once.  It is the tile of jdet_conv3x3_dgrad_rows with conv_igemm.hip's epilogue.
 * P * max(Cin, Cout) < 2^30, 16-byte aligned x / w, else JDET_E_UNSUPPORTED / JDET_E_BADARG. */
int jdet_conv3x3_rows_forward(const float* x_nhwc, const float* w_krsc, const float* bias, int relu,
                              const float* rowmask, const int32_t* rows, const int32_t* count, int N, int H, int W,
                              int Cin, int Cout, int zero_first, float* y_nhwc, jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_ROWS_FWD_H_ */
