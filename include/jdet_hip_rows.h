/* jdet_hip_rows.h -- the row-sparse convolution gradients of libjdet_hip.so (csrc/conv_rows.hip).
 *
 * Why a header of its own: every name of include/jdet_hip.h has a row in the buffer-contract table
 * (tests/abi_cases.py), and that table is revised as a whole (see jdet_hip_atss.h).  These entry points arrived
 * between two revisions: they are exported by the same library, follow every convention stated at the top of
 * jdet_hip.h (status codes, no synchronisation, no allocation, inputs never written, the stream last) and have their
 * contract rows in tests/test_gpu_conv_rows_abi.py.  When the contract table is next revised, fold this file into
 * jdet_hip.h together with those rows (and ROWS_SIGNATURES of jdet_amd/_lib.py into SIGNATURES).
 *
 * What they are for: the regression towers of the S2ANet head (models/roi_heads/s2anet_head.py:L127-205) are trained by
 * a smooth-L1 loss whose weight is zero for every anchor that is not positive, so the gradient entering their 3x3
 * convolutions is exactly zero on almost every position row.  The three entry points below compute the same data and
 * weight gradients as the dense kernels from the non-zero rows only.  No value is read back to the host and no launch
 * shape depends on device data: the capacity of every list is P = N*H*W rows, so there is no overflow path, and a
 * fully dense gradient is computed correctly (only slower than by the dense kernels).
 */
#ifndef JDET_HIP_ROWS_H_
#define JDET_HIP_ROWS_H_

#include "jdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The non-zero rows of a channels-last gradient g (N,H,W,C) = (P, C), in three launches.  Comes before the two
 * entry points below in place of nothing the reference has: Jittor's autograd runs the dense gradients.
 *   flags         (P) bytes, every one written: 1 where any element of the row has (bits & 0x7fffffff) != 0 -- rows
 *                 holding a NaN or an Inf are kept, rows of +0 / -0 are dropped -- else 0
 *   rows          (P) int32: the flagged positions in ASCENDING order in the entries [0, counts[0]), -1 in the rest
 *   rows_dilated  (P) int32: ascending positions whose 3x3 neighbourhood (n, y + dy, x + dx), taken inside the same
 *                 image -- never across a row end or an image boundary -- holds a flagged row, in the entries
 *                 [0, counts[1]), -1 in the rest
 *   counts        2 int32: the two list lengths
 * C % 4 == 0, P * C < 2^30, g 16-byte aligned, else JDET_E_UNSUPPORTED / JDET_E_BADARG.  workspace:
 * jdet_rows_nonzero_workspace(N, H, W) bytes, 4-byte aligned, may hold anything; fewer bytes: JDET_E_WORKSPACE. */
size_t jdet_rows_nonzero_workspace(int N, int H, int W);
int jdet_rows_nonzero(const float* g_nhwc, int N, int H, int W, int C, uint8_t* flags, int32_t* rows,
                      int32_t* rows_dilated, int32_t* counts, void* workspace, size_t workspace_bytes,
                      jdet_stream_t stream);

/* Cin % 4 == 0 and Cout % 16 == 0: what both gradient entry points below take (else JDET_E_UNSUPPORTED). */
int jdet_conv3x3_rows_supported(int Cin, int Cout);

/* gw (Cout,3,3,Cin) += sum over the listed positions r of gy[r, co] * x[nbr(r, tap), ci]; neighbours outside the
 * image contribute zero.  Replaces jdet_conv3x3_wgrad (plain form) where gy is zero outside rows[0 .. *count): the
 * same tiles, fragments and float atomics with the K index taken from the list, so several calls may target one
 * buffer exactly as there.  rows / count: device pointers (jdet_rows_nonzero's `rows` and `counts`); entries past
 * *count are not read; *count == 0 adds nothing.  The grid is fixed by the channel counts; (P + 16) * max(Cin, Cout)
 * < 2^30 and 16-byte aligned x / gy, else JDET_E_UNSUPPORTED / JDET_E_BADARG. */
int jdet_conv3x3_wgrad_rows_workers(int Cin, int Cout); /* K workers per tile: at most this many partial sums are added
                                                           to one element of gw per call (0: unsupported channels) */
int jdet_conv3x3_wgrad_rows(const float* x_nhwc, const float* gy_nhwc, const int32_t* rows, const int32_t* count,
                            int N, int H, int W, int Cin, int Cout, float* gw_krsc, jdet_stream_t stream);

/* gx[r, ci] = sum over taps and co of gy[nbr(r, tap), co] * wd[ci, tap, co] for every r of the list; rows of gx that
 * are not listed are left alone, or -- zero_first != 0 -- zero-filled by a launch of this call, so that gx
 * (N,H,W,Cin) is fully written.  Replaces the library's dense data gradient (convolution_backward, igemm_bwd_*) where
 * gy is zero outside the rows whose dilation the list is (jdet_rows_nonzero's `rows_dilated`, `counts + 1`).  wd
 * (Cin,3,3,Cout): the flipped weights jdet_conv_dgrad_weights writes.  The grid is fixed by P (P / 64 row tiles);
 * tiles past *count leave at once.  P * max(Cin, Cout) < 2^30, 16-byte aligned gy / wd, else JDET_E_UNSUPPORTED /
 * JDET_E_BADARG. */
int jdet_conv3x3_dgrad_rows(const float* gy_nhwc, const float* wd_crsk, const int32_t* rows, const int32_t* count,
                            int N, int H, int W, int Cin, int Cout, int zero_first, float* gx_nhwc,
                            jdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JDET_HIP_ROWS_H_ */
