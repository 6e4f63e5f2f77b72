// Strip convolution on channels-last fp32 maps (include/jdet_hip_strip.h): a depthwise 1 x K or K x 1 kernel, stride 1,
// "same" padding -- the conv_spatial1 / conv_spatial2 layers of a StripNet block.
//
//   jdet_strip_conv_forward    y = stripconv(x) + bias; on flipped weights it is the data gradient
//
// A rolling-window kernel.  A thread owns four consecutive channels (one 16-byte access) of kOut consecutive outputs
// along the strip axis; consecutive threads own consecutive channel quads (and then, on axis 0, consecutive w), so a
// wave's accesses at every window position are whole contiguous spans.  The kOut outputs share a window of K + kOut - 1
// inputs: the thread walks it once, loads every x value and every weight quad once, and feeds the value at window
// position j to output p through tap j - p -- the last kOut weight quads are kept in a rolling set of named registers.
// Each output therefore still adds its taps in increasing tap index, a multiply then an add, and a window position
// outside the map is skipped for all of them: the order of jdet_dwconv_nhwc_forward, bit for bit, with K + 3 loads of x
// per thread where that kernel issues 4 K.  The window is walked kUnroll positions at a time, all of a chunk's loads
// issued before its first use; loads of positions outside the map or past the window go to a clamped (valid) address
// and are dropped.
#include "jdet_hip_strip.h"
#include "common.h"

namespace {

constexpr int kOut = 4;       // outputs along the strip axis per thread
constexpr int kUnroll = 8;    // window positions whose loads are in flight together
constexpr int kMaxK = 1023;

struct Geom {
  int C4;                    // C / 4
  int L, LT;                 // length of the strip axis, ceil(L / kOut)
  int S;                     // float4 stride between neighbours on the strip axis: C4 (axis 1) or W * C4 (axis 0)
  int W;                     // axis 0 only: the threads after the channel quads walk w
  int K, pad;
};

__device__ __forceinline__ float4 mul_add(float4 acc, float4 w, float4 x) {   // acc + (w * x), uncontracted
  const float4 p = make_float4(w.x * x.x, w.y * x.y, w.z * x.z, w.w * x.w);
  return make_float4(acc.x + p.x, acc.y + p.y, acc.z + p.z, acc.w + p.w);
}

// AXIS 1: id = ((n * H + h) * LT + t) * C4 + cq, the strip runs along W.
// AXIS 0: id = ((n * LT + t) * W + w) * C4 + cq, the strip runs along H.
template <int AXIS>
__global__ __launch_bounds__(256) void strip_conv_kernel(const float4* __restrict__ x, const float4* __restrict__ w,
                                                         const float4* __restrict__ bias, Geom g, int total,
                                                         float4* __restrict__ y) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int cq = id % g.C4;
  int r = id / g.C4;
  int t, base;                                 // base: float4 index of strip position 0, channel quad 0
  if (AXIS == 1) {
    t = r % g.LT;
    base = (r / g.LT) * g.L * g.C4;
  } else {
    const int wi = r % g.W;
    r /= g.W;
    t = r % g.LT;
    base = ((r / g.LT) * g.L * g.W + wi) * g.C4;
  }
  const int o0 = t * kOut;
  const float4* xp = x + base + cq;
  const float4* wp = w + cq;
  const int i0 = o0 - g.pad;                   // the map index of window position 0
  const int J = g.K + kOut - 1;                // window positions
  const float4 b = bias ? bias[cq] : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc0 = b, acc1 = b, acc2 = b, acc3 = b;
  float4 w1 = b, w2 = b, w3 = b;               // the weights of taps j - 1, j - 2, j - 3; read only where those exist
  for (int j0 = 0; j0 < J; j0 += kUnroll) {
    float4 xv[kUnroll], wv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      int i = i0 + j0 + u;
      i = i < 0 ? 0 : (i >= g.L ? g.L - 1 : i);
      int k = j0 + u;
      k = k >= g.K ? g.K - 1 : k;
      xv[u] = xp[i * g.S];
      wv[u] = wp[k * g.C4];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const int j = j0 + u;
      if (j >= J) break;
      const int i = i0 + j;
      const float4 w0 = wv[u];
      if (i >= 0 && i < g.L) {
        if (j < g.K) acc0 = mul_add(acc0, w0, xv[u]);
        if (j >= 1 && j - 1 < g.K) acc1 = mul_add(acc1, w1, xv[u]);
        if (j >= 2 && j - 2 < g.K) acc2 = mul_add(acc2, w2, xv[u]);
        if (j >= 3 && j - 3 < g.K) acc3 = mul_add(acc3, w3, xv[u]);
      }
      w3 = w2;
      w2 = w1;
      w1 = w0;
    }
  }
  float4* yp = y + base + cq;
  yp[o0 * g.S] = acc0;
  if (o0 + 1 < g.L) yp[(o0 + 1) * g.S] = acc1;
  if (o0 + 2 < g.L) yp[(o0 + 2) * g.S] = acc2;
  if (o0 + 3 < g.L) yp[(o0 + 3) * g.S] = acc3;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

JDET_API int jdet_strip_conv_forward(const float* x, const float* w, const float* bias, int N, int H, int W, int C, int K,
                                     int axis, float* y, jdet_stream_t stream) {
  if (!x || !w || !y) return JDET_E_BADARG;
  if (N < 1 || H < 1 || W < 1 || C < 1 || K < 1 || (axis != 0 && axis != 1)) return JDET_E_BADARG;
  if (C % 4 != 0 || K % 2 == 0 || K > kMaxK) return JDET_E_UNSUPPORTED;
  if ((long)N * H * W * C >= 2147483648L) return JDET_E_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y)) return JDET_E_BADARG;
  const int C4 = C / 4;
  const int L = axis == 1 ? W : H;
  const int LT = (L + kOut - 1) / kOut;
  const Geom g{C4, L, LT, axis == 1 ? C4 : W * C4, W, K, (K - 1) / 2};
  const long total = (long)N * (axis == 1 ? H : W) * LT * C4;   // < 2^31 / 4
  hipStream_t st = (hipStream_t)stream;
  if (axis == 1) {
    hipLaunchKernelGGL((strip_conv_kernel<1>), dim3(jdet_cdiv(total, 256)), dim3(256), 0, st, (const float4*)x,
                       (const float4*)w, (const float4*)bias, g, (int)total, (float4*)y);
  } else {
    hipLaunchKernelGGL((strip_conv_kernel<0>), dim3(jdet_cdiv(total, 256)), dim3(256), 0, st, (const float4*)x,
                       (const float4*)w, (const float4*)bias, g, (int)total, (float4*)y);
  }
  return jdet_launch_status();
}
