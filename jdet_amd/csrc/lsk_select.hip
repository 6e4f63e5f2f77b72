// The kernel-selection step of an LSK block (include/jdet_hip_lsk.h) around the library's 2 -> 2 7x7 convolution:
//
//   jdet_lsk_squeeze_forward / _backward   channel mean and max (first argmax) of concat(a1, a2), never materialised
//   jdet_lsk_select_forward / _backward    a1 * sig0 + a2 * sig1 and its three gradients
//
// Streaming kernels over channels-last maps.  A pixel is worked by a group of G lanes of one wave (G = 4, 16 or 64): lane l
// takes the access units l, l + G, ... of the pixel's channels -- 16 bytes each when Ch % 4 == 0 and the pointers allow
// it, 4 bytes otherwise -- and the per-pixel reductions finish with an xor butterfly inside the group.  The order of every
// addition is the header's contract; no atomics, no second stage.
#include "jdet_hip_lsk.h"
#include <initializer_list>

#include "common.h"

namespace {

template <int V>
struct Unit;
template <>
struct Unit<4> {
  typedef float4 T;
  static __device__ __forceinline__ void get(const T& v, float* e) { e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w; }
  static __device__ __forceinline__ T make(const float* e) { return make_float4(e[0], e[1], e[2], e[3]); }
};
template <>
struct Unit<1> {
  typedef float T;
  static __device__ __forceinline__ void get(const T& v, float* e) { e[0] = v; }
  static __device__ __forceinline__ T make(const float* e) { return e[0]; }
};

// pixels: P; units per branch: U = Ch / V.  Groups are aligned to G lanes, so the butterfly never leaves a group; lanes of
// a group beyond the last pixel load and store nothing but take part in the shuffles.
template <int G, int V>
__global__ __launch_bounds__(256) void squeeze_fwd_kernel(const float* __restrict__ a1, const float* __restrict__ a2, int P,
                                                          int U, float* __restrict__ agg, int* __restrict__ argmax) {
  typedef typename Unit<V>::T T;
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int pix = tid / G, l = tid % G;
  const bool live = pix < P;
  const T* p1 = reinterpret_cast<const T*>(a1) + (size_t)(live ? pix : 0) * U;
  const T* p2 = reinterpret_cast<const T*>(a2) + (size_t)(live ? pix : 0) * U;
  float sum = 0.f, best = -INFINITY;
  int at = 0x7fffffff;
  if (live) {
    for (int u = l; u < 2 * U; u += G) {
      float e[V];
      Unit<V>::get(u < U ? p1[u] : p2[u - U], e);
#pragma unroll
      for (int k = 0; k < V; k++) {
        sum = sum + e[k];
        if (e[k] > best) best = e[k], at = u * V + k;     // strict: the first of equal values stays
      }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    sum = sum + __shfl_xor(sum, off, 64);
    const float ob = __shfl_xor(best, off, 64);
    const int oa = __shfl_xor(at, off, 64);
    if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
  }
  if (live && l == 0) {
    agg[(size_t)pix * 2] = sum / (float)(2 * U * V);
    agg[(size_t)pix * 2 + 1] = best;
    argmax[pix] = at == 0x7fffffff ? 0 : at;              // a pixel of -inf / NaN only
  }
}

// thread = one access unit of concat(g_a1, g_a2) of one pixel
template <int V>
__global__ __launch_bounds__(256) void squeeze_bwd_kernel(const float* __restrict__ g_agg, const int* __restrict__ argmax,
                                                          int P, int U, float* __restrict__ g_a1, float* __restrict__ g_a2) {
  typedef typename Unit<V>::T T;
  const int tid = blockIdx.x * 256 + threadIdx.x;        // < P * 2 U < 2^31
  const int pix = tid / (2 * U), u = tid % (2 * U);
  if (pix >= P) return;
  const float gm = g_agg[(size_t)pix * 2] / (float)(2 * U * V), gx = g_agg[(size_t)pix * 2 + 1];
  const int am = argmax[pix];
  T* dst = reinterpret_cast<T*>(u < U ? g_a1 : g_a2) + (size_t)pix * U + (u < U ? u : u - U);
  float e[V];
  Unit<V>::get(*dst, e);
#pragma unroll
  for (int k = 0; k < V; k++) {
    e[k] = e[k] + gm;
    if (u * V + k == am) e[k] = e[k] + gx;
  }
  *dst = Unit<V>::make(e);
}

template <int V>
__global__ __launch_bounds__(256) void select_fwd_kernel(const float* __restrict__ a1, const float* __restrict__ a2,
                                                         const float* __restrict__ sig, int P, int U,
                                                         float* __restrict__ out) {
  typedef typename Unit<V>::T T;
  const int tid = blockIdx.x * 256 + threadIdx.x;        // < P * U
  const int pix = tid / U;
  if (pix >= P) return;
  const float s0 = sig[(size_t)pix * 2], s1 = sig[(size_t)pix * 2 + 1];
  float x[V], y[V], o[V];
  Unit<V>::get(reinterpret_cast<const T*>(a1)[tid], x);
  Unit<V>::get(reinterpret_cast<const T*>(a2)[tid], y);
#pragma unroll
  for (int k = 0; k < V; k++) o[k] = (x[k] * s0) + (y[k] * s1);
  reinterpret_cast<T*>(out)[tid] = Unit<V>::make(o);
}

template <int G, int V>
__global__ __launch_bounds__(256) void select_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a1,
                                                         const float* __restrict__ a2, const float* __restrict__ sig, int P,
                                                         int U, float* __restrict__ g_a1, float* __restrict__ g_a2,
                                                         float* __restrict__ g_sig) {
  typedef typename Unit<V>::T T;
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int pix = tid / G, l = tid % G;
  const bool live = pix < P;
  const size_t base = (size_t)(live ? pix : 0) * U;
  float d0 = 0.f, d1 = 0.f;
  if (live) {
    const float s0 = sig[(size_t)pix * 2], s1 = sig[(size_t)pix * 2 + 1];
    for (int u = l; u < U; u += G) {
      float gv[V], x[V], y[V], o1[V], o2[V];
      Unit<V>::get(reinterpret_cast<const T*>(g)[base + u], gv);
      Unit<V>::get(reinterpret_cast<const T*>(a1)[base + u], x);
      Unit<V>::get(reinterpret_cast<const T*>(a2)[base + u], y);
#pragma unroll
      for (int k = 0; k < V; k++) {
        o1[k] = gv[k] * s0;
        o2[k] = gv[k] * s1;
        d0 = d0 + (gv[k] * x[k]);
        d1 = d1 + (gv[k] * y[k]);
      }
      reinterpret_cast<T*>(g_a1)[base + u] = Unit<V>::make(o1);
      reinterpret_cast<T*>(g_a2)[base + u] = Unit<V>::make(o2);
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    d0 = d0 + __shfl_xor(d0, off, 64);
    d1 = d1 + __shfl_xor(d1, off, 64);
  }
  if (live && l == 0) {
    g_sig[(size_t)pix * 2] = d0;
    g_sig[(size_t)pix * 2 + 1] = d1;
  }
}

struct Shape {
  int P, Ch;
};

// -> status; dims below 1 are bad arguments; 2^31 elements or more of concat(a1, a2), or 2^25 pixels or more (64 lanes
// each under a 32-bit thread index), unsupported
int make_shape(int N, int H, int W, int Ch, Shape* out) {
  if (N < 1 || H < 1 || W < 1 || Ch < 1) return JDET_E_BADARG;
  if ((long)N * H * W * 2 * Ch >= 2147483648L || (long)N * H * W >= (1L << 25)) return JDET_E_UNSUPPORTED;
  *out = Shape{N * H * W, Ch};
  return JDET_OK;
}

bool all_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;
  return true;
}

int group_of(int units) { return units <= 4 ? 4 : (units <= 16 ? 16 : 64); }

#define LSK_GROUPED(KERNEL, G, V, P, ...)                                                                              \
  hipLaunchKernelGGL((KERNEL<G, V>), dim3(jdet_cdiv((long)(P) * (G), 256)), dim3(256), 0, st, __VA_ARGS__)

#define LSK_DISPATCH(KERNEL, units, vec, P, ...)                                                                       \
  do {                                                                                                                 \
    const int G_ = group_of(units);                                                                                    \
    if (vec) {                                                                                                         \
      if (G_ == 4) LSK_GROUPED(KERNEL, 4, 4, P, __VA_ARGS__);                                                          \
      else if (G_ == 16) LSK_GROUPED(KERNEL, 16, 4, P, __VA_ARGS__);                                                   \
      else LSK_GROUPED(KERNEL, 64, 4, P, __VA_ARGS__);                                                                 \
    } else {                                                                                                           \
      if (G_ == 4) LSK_GROUPED(KERNEL, 4, 1, P, __VA_ARGS__);                                                          \
      else if (G_ == 16) LSK_GROUPED(KERNEL, 16, 1, P, __VA_ARGS__);                                                   \
      else LSK_GROUPED(KERNEL, 64, 1, P, __VA_ARGS__);                                                                 \
    }                                                                                                                  \
  } while (0)

}  // namespace

JDET_API int jdet_lsk_squeeze_forward(const float* a1, const float* a2, int N, int H, int W, int Ch, float* agg,
                                      int* argmax, jdet_stream_t stream) {
  Shape s;
  if (!a1 || !a2 || !agg || !argmax) return JDET_E_BADARG;
  if (int e = make_shape(N, H, W, Ch, &s)) return e;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = Ch % 4 == 0 && all_aligned16({a1, a2});
  const int U = vec ? Ch / 4 : Ch;
  LSK_DISPATCH(squeeze_fwd_kernel, 2 * U, vec, s.P, a1, a2, s.P, U, agg, argmax);
  return jdet_launch_status();
}

JDET_API int jdet_lsk_squeeze_backward(const float* g_agg, const int* argmax, int N, int H, int W, int Ch, float* g_a1,
                                       float* g_a2, jdet_stream_t stream) {
  Shape s;
  if (!g_agg || !argmax || !g_a1 || !g_a2) return JDET_E_BADARG;
  if (int e = make_shape(N, H, W, Ch, &s)) return e;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = Ch % 4 == 0 && all_aligned16({g_a1, g_a2});
  const int U = vec ? Ch / 4 : Ch;
  const int grid = jdet_cdiv((long)s.P * 2 * U, 256);
  if (vec)
    hipLaunchKernelGGL(squeeze_bwd_kernel<4>, dim3(grid), dim3(256), 0, st, g_agg, argmax, s.P, U, g_a1, g_a2);
  else
    hipLaunchKernelGGL(squeeze_bwd_kernel<1>, dim3(grid), dim3(256), 0, st, g_agg, argmax, s.P, U, g_a1, g_a2);
  return jdet_launch_status();
}

JDET_API int jdet_lsk_select_forward(const float* a1, const float* a2, const float* sig, int N, int H, int W, int Ch,
                                     float* out, jdet_stream_t stream) {
  Shape s;
  if (!a1 || !a2 || !sig || !out) return JDET_E_BADARG;
  if (int e = make_shape(N, H, W, Ch, &s)) return e;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = Ch % 4 == 0 && all_aligned16({a1, a2, out});
  const int U = vec ? Ch / 4 : Ch;
  const int grid = jdet_cdiv((long)s.P * U, 256);
  if (vec)
    hipLaunchKernelGGL(select_fwd_kernel<4>, dim3(grid), dim3(256), 0, st, a1, a2, sig, s.P, U, out);
  else
    hipLaunchKernelGGL(select_fwd_kernel<1>, dim3(grid), dim3(256), 0, st, a1, a2, sig, s.P, U, out);
  return jdet_launch_status();
}

JDET_API int jdet_lsk_select_backward(const float* g, const float* a1, const float* a2, const float* sig, int N, int H,
                                      int W, int Ch, float* g_a1, float* g_a2, float* g_sig, jdet_stream_t stream) {
  Shape s;
  if (!g || !a1 || !a2 || !sig || !g_a1 || !g_a2 || !g_sig) return JDET_E_BADARG;
  if (int e = make_shape(N, H, W, Ch, &s)) return e;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = Ch % 4 == 0 && all_aligned16({g, a1, a2, g_a1, g_a2});
  const int U = vec ? Ch / 4 : Ch;
  LSK_DISPATCH(select_bwd_kernel, U, vec, s.P, g, a1, a2, sig, s.P, U, g_a1, g_a2, g_sig);
  return jdet_launch_status();
}
