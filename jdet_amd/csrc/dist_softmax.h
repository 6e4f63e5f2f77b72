// What the distribution and distillation kernels of dist_loss.hip share: a tile of softmax rows staged through LDS so
// that every global access of a wave covers contiguous memory, and the softmax of one row in registers.
//
// A softmax row is K <= 32 floats (36 bytes at K = 9: not 16-byte aligned), one row per thread.  Read straight from
// memory that is a stride-K access; instead the kDistTileRows rows of a tile -- kDistTileRows * K contiguous floats,
// a multiple of 16 bytes for every K -- are copied with 16-byte accesses, element i of the tile by lane i / 4, into LDS
// rows of K | 1 floats (an odd pitch: the row-per-thread reads and writes that follow hit 32 distinct banks).
#pragma once
#include "common.h"

constexpr int kDistTileRows = 240;   // softmax rows of one tile: 48 anchors x 5 sides; 240 of a workgroup's 256 threads

__device__ __forceinline__ int dist_pitch(int K) { return K | 1; }

// element i of a tile (i < 240 * 32) -> its row, exactly: (i + 0.5) / K is at least 0.5 / K >= 1 / 64 away from an
// integer and the fp32 product is off by less than 1e-3
__device__ __forceinline__ int dist_row_of(int i, float inv_k) { return (int)(((float)i + 0.5f) * inv_k); }

// global -> LDS.  g: the tile's first float, n_el = its rows * K; vec: g is 16-byte aligned; need(j): row j's values
// are wanted.  A 16-byte piece none of whose rows is wanted is not read (its LDS words are left as they are).
template <typename Need>
__device__ __forceinline__ void dist_tile_load(const float* __restrict__ g, int n_el, int K, float inv_k, bool vec,
                                               float* __restrict__ s, Need need) {
  const int kp = dist_pitch(K);
  const int n4 = vec ? n_el >> 2 : 0;
  for (int q = threadIdx.x; q < n4; q += 256) {
    const int i = q * 4;
    int j = dist_row_of(i, inv_k), k = i - j * K;
    const int j3 = dist_row_of(i + 3, inv_k);
    bool any = false;
    for (int jj = j; jj <= j3; jj++) any = any || need(jj);
    if (!any) continue;
    const float4 v = *reinterpret_cast<const float4*>(g + i);
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; u++) {
      s[j * kp + k] = x[u];
      if (++k == K) { k = 0; j++; }
    }
  }
  for (int i = n4 * 4 + threadIdx.x; i < n_el; i += 256) {
    const int j = dist_row_of(i, inv_k);
    if (need(j)) s[j * kp + (i - j * K)] = g[i];
  }
}

// LDS -> global, every one of the n_el elements
__device__ __forceinline__ void dist_tile_store(float* __restrict__ g, int n_el, int K, float inv_k, bool vec,
                                                const float* __restrict__ s) {
  const int kp = dist_pitch(K);
  const int n4 = vec ? n_el >> 2 : 0;
  for (int q = threadIdx.x; q < n4; q += 256) {
    const int i = q * 4;
    int j = dist_row_of(i, inv_k), k = i - j * K;
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      x[u] = s[j * kp + k];
      if (++k == K) { k = 0; j++; }
    }
    *reinterpret_cast<float4*>(g + i) = make_float4(x[0], x[1], x[2], x[3]);
  }
  for (int i = n4 * 4 + threadIdx.x; i < n_el; i += 256) {
    const int j = dist_row_of(i, inv_k);
    g[i] = s[j * kp + (i - j * K)];
  }
}

// Softmax of one row of K <= KMAX values x_k = z_k * inv_t, in double, max-subtracted:
//   e[k] = exp(x_k - m), S = sum e, so p_k = e[k] / S and log p_k = (x_k - m) - log S  (the log-softmax form: no
//   log of a probability that underflowed).  e[k] = 0 for k >= K.
template <int KMAX>
struct DistSoftmax {
  float z[KMAX];
  double m, S, e[KMAX];

  __device__ __forceinline__ void load(const float* __restrict__ row, int K, double inv_t) {
#pragma unroll
    for (int k = 0; k < KMAX; k++) z[k] = k < K ? row[k] : row[0];
    float zm = z[0];
#pragma unroll
    for (int k = 1; k < KMAX; k++) zm = fmaxf(zm, z[k]);
    m = (double)zm * inv_t;      // inv_t > 0: the largest x_k up to one rounding, which the subtraction only has to bound
    S = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      e[k] = k < K ? exp((double)z[k] * inv_t - m) : 0.0;
      S += e[k];
    }
  }
  // x_k - m
  __device__ __forceinline__ double shifted(int k, double inv_t) const { return (double)z[k] * inv_t - m; }
};
