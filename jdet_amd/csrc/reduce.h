// The fixed-order reductions of the two-stage sum kernels.  The ORDER of every addition here is a contract.
// Device code, included by loss_offset.hip, gaussian_loss.hip, graph_safe.hip and frozen_bn.hip.
//
// Not here on purpose, because their orders differ from the ones below (merging any of them moves result bits):
//   frozen_bn.hip  sums_finish_kernel (eight partial rows in flight, a tree) and bn_sums_finish_kernel (four in flight,
//                  a loop): two second stages, two orders
//   conv_bn_kernel.h  writes [rows][2][C] partial rows too, but straight from registers: the two half waves of a column
//                  are combined with one __shfl_xor(., 32) and every (M tile, wave row) stores its own row -- no LDS
//                  combine over t, t + cpt, ...; conv_rows.hip forms no per-channel sums (its wave_sum counts integers)
#pragma once
#include "common.h"

// the xor butterfly off = 32, 16, ..., 1 over the 64 lanes of a wave: every lane ends with the same bits
template <typename T>
__device__ __forceinline__ T jdet_wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// 256-thread workgroups: wave sums s0..s3 through s_part[4], then (s0 + s1) + (s2 + s3).  Thread 0 alone gets the sum.
template <typename T>
__device__ __forceinline__ T jdet_block_sum4(T acc, T* s_part) {
  acc = jdet_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  return threadIdx.x == 0 ? (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]) : T(0);
}

// A level's targets / weights are a column window [:, s:e] of the per-image arrays: logical row r lives in block
// r / rows_per_block (one image's window) at element r % rows_per_block.
struct Blocked {
  long rows_per_block;   // rows of one block; >= total rows when the array is contiguous
  long block_stride;     // distance between two blocks, in rows
};
__device__ __forceinline__ long blocked_row(const Blocked& b, long r) {
  const long blk = r / b.rows_per_block;
  return blk * b.block_stride + (r - blk * b.rows_per_block);
}

// First stage of a loss sum: 256-thread workgroups, one partial sum each, at most kJdetLossGridCap of them -- the rows
// of the workspace every loss entry point asks for (jdet_sigmoid_focal_loss_workspace).
constexpr int kJdetLossGridCap = 1024;
constexpr size_t kJdetLossWorkspaceBytes = sizeof(float) * kJdetLossGridCap;

static inline int jdet_loss_grid(long n_items, long items_per_group) {
  const long want = (n_items + items_per_group - 1) / items_per_group;
  return (int)(want < 1 ? 1 : (want > kJdetLossGridCap ? kJdetLossGridCap : want));
}

namespace {

// Second stage: one workgroup, thread t adds partial[t], partial[t + 256], ...; SCALED: (sum / *avg_factor) * loss_weight,
// the operations of `loss_weight * (sum / avg_factor)` in the composition's order.
template <bool SCALED>
__global__ __launch_bounds__(256) void jdet_sum_partials_kernel(const float* __restrict__ partial, int n,
                                                                const float* __restrict__ avg_factor,
                                                                float loss_weight, float* __restrict__ out) {
  __shared__ float s_part[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const float total = jdet_block_sum4(acc, s_part);
  if (threadIdx.x == 0) out[0] = SCALED ? (total / avg_factor[0]) * loss_weight : total;
}

template <bool SCALED>
int jdet_sum_partials(const float* partial, int n, const float* avg_factor, float loss_weight, float* out,
                      hipStream_t st) {
  hipLaunchKernelGGL((jdet_sum_partials_kernel<SCALED>), dim3(1), dim3(256), 0, st, partial, n, avg_factor, loss_weight, out);
  return jdet_launch_status();
}

}  // namespace

// Epilogue of the frozen-BN family's first stages.  Every thread holds N per-channel-quad sums (N = 8: dbeta and dgamma
// quads, N = 4: dbeta alone); blockDim is a multiple of cpt, so the threads t, t + cpt, ... of a workgroup hold the same
// quad, and (blockIdx * blockDim + t) % cpt == t.  s_red: [blockDim][N] floats.  Threads t < cpt add the LDS rows t,
// t + cpt, ... in that order and store one partial row [2][cpt * 4] (N = 4: its first half only).
template <int N>
__device__ __forceinline__ void jdet_quad_partials(float* s_red, const float (&vals)[N], int cpt,
                                                   float* __restrict__ partial_row) {
  static_assert(N == 4 || N == 8, "one or two channel quads");
  float* mine = s_red + (size_t)threadIdx.x * N;
#pragma unroll
  for (int k = 0; k < N; k++) mine[k] = vals[k];
  __syncthreads();
  if ((int)threadIdx.x < cpt) {
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; k++) acc[k] = 0.f;
    for (int t = threadIdx.x; t < (int)blockDim.x; t += cpt)
#pragma unroll
      for (int k = 0; k < N; k++) acc[k] += s_red[(size_t)t * N + k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      partial_row[threadIdx.x * 4 + k] = acc[k];
      if constexpr (N == 8) partial_row[cpt * 4 + threadIdx.x * 4 + k] = acc[4 + k];
    }
  }
}
