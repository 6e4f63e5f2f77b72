// Depthwise convolution on channels-last fp32 maps (include/jdet_hip_lsk.h): stride 1, "same" padding, any dilation,
// rectangular kernels -- the 5x5, the 7x7 dilation-3 and the 3x3 + bias + GELU layers of an LSKNet block.
//
//   jdet_dwconv_nhwc_forward    y = act(dwconv(x) + bias); on flipped weights it is the data gradient
//   jdet_dwconv_gelu_backward   g_z = g_y * gelu'(dwconv(x) + bias), the pre-activation recomputed
//   jdet_dwconv_nhwc_wgrad      weight and bias gradients, two stages in a fixed order, no atomics
//
// These are streaming kernels: a thread owns four consecutive channels (one 16-byte access) of kPixels consecutive
// output pixels of an image row; consecutive threads own consecutive channel quads, so a wave reads and writes whole
// 1 KiB spans.  A tap's weights are read once per thread and used for its kPixels pixels -- one tap at a time, never the
// whole tap set in registers; the taps' re-reads of x are served by the caches.  The order of every addition is the
// header's contract: per output kh outer, kw inner, multiply then add, taps outside the map skipped.
#include "jdet_hip_lsk.h"
#include "common.h"

namespace {

constexpr int kPixels = 4;   // output pixels of one row per thread
constexpr int kMaxK = 1024;

struct Geom {
  int N, H, W, C4;           // C4 = C / 4
  int KH, KW, pad_h, pad_w, dil_h, dil_w;
  int WT;                    // ceil(W / kPixels)
};

__device__ __forceinline__ float4 mul_add(float4 acc, float4 w, float4 x) {   // acc + (w * x), uncontracted
  const float4 p = make_float4(w.x * x.x, w.y * x.y, w.z * x.z, w.w * x.w);
  return make_float4(acc.x + p.x, acc.y + p.y, acc.z + p.z, acc.w + p.w);
}

__device__ __forceinline__ float gelu_f(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752f)); }

// Phi(z) + z phi(z)
__device__ __forceinline__ float gelu_grad_f(float z) {
  const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752f));
  const float pdf = expf(-0.5f * z * z) * 0.39894228040143268f;
  return cdf + z * pdf;
}

// MODE 0: y = z; 1: y = gelu(z); 2: y = gy * gelu'(z)
template <int MODE>
__global__ __launch_bounds__(256) void dwconv_kernel(const float4* __restrict__ x, const float4* __restrict__ w,
                                                     const float4* __restrict__ bias, const float4* __restrict__ gy,
                                                     Geom g, int total, float4* __restrict__ y) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int cq = id % g.C4;
  int r = id / g.C4;
  const int wt = r % g.WT;
  r /= g.WT;                                   // n * H + h
  const int h = r % g.H;
  const int w0 = wt * kPixels;
  const int row0 = (r - h) * g.W;              // first pixel of image n
  float4 acc[kPixels];
  const float4 b = bias ? bias[cq] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int p = 0; p < kPixels; p++) acc[p] = b;
  for (int kh = 0; kh < g.KH; kh++) {
    const int ih = h + kh * g.dil_h - g.pad_h;
    if (ih < 0 || ih >= g.H) continue;
    const float4* xr = x + (size_t)(row0 + ih * g.W) * g.C4 + cq;
    const float4* wr = w + (size_t)kh * g.KW * g.C4 + cq;
    for (int kw = 0; kw < g.KW; kw++) {
      const float4 wv = wr[(size_t)kw * g.C4];
      const int iw0 = w0 + kw * g.dil_w - g.pad_w;
#pragma unroll
      for (int p = 0; p < kPixels; p++) {
        const int iw = iw0 + p;
        if (iw >= 0 && iw < g.W) acc[p] = mul_add(acc[p], wv, xr[iw * g.C4]);
      }
    }
  }
  const size_t o = (size_t)(r * g.W + w0) * g.C4 + cq;
#pragma unroll
  for (int p = 0; p < kPixels; p++) {
    if (w0 + p >= g.W) break;
    float4 v = acc[p];
    if (MODE == 1) v = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
    if (MODE == 2) {
      const float4 q = gy[o + (size_t)p * g.C4];
      v = make_float4(q.x * gelu_grad_f(v.x), q.y * gelu_grad_f(v.y), q.z * gelu_grad_f(v.z), q.w * gelu_grad_f(v.w));
    }
    y[o + (size_t)p * g.C4] = v;
  }
}

// ---- weight gradient, first stage: thread = (tap or bias, channel quad) of one slab of image rows
__global__ __launch_bounds__(256) void dwconv_wgrad_partial_kernel(const float4* __restrict__ x,
                                                                   const float4* __restrict__ gr, Geom g, int rows_per_slab,
                                                                   float4* __restrict__ partial) {
  const int taps = g.KH * g.KW;
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= (taps + 1) * g.C4) return;
  const int cq = id % g.C4, t = id / g.C4;
  const int s = blockIdx.y;
  const int R = g.N * g.H;
  const int r0 = s * rows_per_slab;
  const int r1 = r0 + rows_per_slab < R ? r0 + rows_per_slab : R;
  const bool is_bias = t == taps;
  const int kh = is_bias ? 0 : t / g.KW, kw = is_bias ? 0 : t - (t / g.KW) * g.KW;
  const int dh = is_bias ? 0 : kh * g.dil_h - g.pad_h, dw = is_bias ? 0 : kw * g.dil_w - g.pad_w;
  const int wlo = dw < 0 ? -dw : 0, whi = dw > 0 ? g.W - dw : g.W;   // w with 0 <= w + dw < W
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r = r0; r < r1; r++) {
    const int h = r % g.H;
    const int ih = h + dh;
    if (ih < 0 || ih >= g.H) continue;
    const float4* gp = gr + (long)r * g.W * g.C4 + cq;
    const float4* xp = x + ((long)(r - h + ih) * g.W + dw) * g.C4 + cq;   // read at w >= wlo only
    if (is_bias) {
      for (int wv = 0; wv < g.W; wv++) {
        const float4 q = gp[wv * g.C4];
        acc = make_float4(acc.x + q.x, acc.y + q.y, acc.z + q.z, acc.w + q.w);
      }
    } else {
      for (int wv = wlo; wv < whi; wv++) acc = mul_add(acc, gp[wv * g.C4], xp[wv * g.C4]);
    }
  }
  partial[((size_t)s * (taps + 1) + t) * g.C4 + cq] = acc;
}

// second stage: one wave per (tap or bias, channel quad); lane l adds slabs l, l + 64, ..., then the xor butterfly
__global__ __launch_bounds__(64) void dwconv_wgrad_finish_kernel(const float4* __restrict__ partial, int S, int taps,
                                                                 int C4, float4* __restrict__ gw, float4* __restrict__ gb) {
  const int cq = blockIdx.x % C4, t = blockIdx.x / C4;
  const int lane = threadIdx.x;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = lane; s < S; s += 64) {
    const float4 q = partial[((size_t)s * (taps + 1) + t) * C4 + cq];
    acc = make_float4(acc.x + q.x, acc.y + q.y, acc.z + q.z, acc.w + q.w);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc.x += __shfl_xor(acc.x, off, 64);
    acc.y += __shfl_xor(acc.y, off, 64);
    acc.z += __shfl_xor(acc.z, off, 64);
    acc.w += __shfl_xor(acc.w, off, 64);
  }
  if (lane == 0) {
    if (t < taps) {
      gw[(size_t)t * C4 + cq] = acc;
    } else if (gb) {
      gb[cq] = acc;
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the shared argument rules -> status and the kernels' form of the geometry
int make_geom(int N, int H, int W, int C, int KH, int KW, int pad_h, int pad_w, int dil_h, int dil_w, Geom* out) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || KH < 1 || KW < 1 || pad_h < 0 || pad_w < 0 || dil_h < 1 || dil_w < 1)
    return JDET_E_BADARG;
  if (C % 4 != 0 || KH > kMaxK || KW > kMaxK || dil_h > kMaxK || dil_w > kMaxK) return JDET_E_UNSUPPORTED;
  if (2 * (long)pad_h != (long)dil_h * (KH - 1) || 2 * (long)pad_w != (long)dil_w * (KW - 1)) return JDET_E_UNSUPPORTED;
  if ((long)N * H * W * C >= 2147483648L) return JDET_E_UNSUPPORTED;
  *out = Geom{N, H, W, C / 4, KH, KW, pad_h, pad_w, dil_h, dil_w, (W + kPixels - 1) / kPixels};
  return JDET_OK;
}

int slabs_of(int N, int H) {
  const long R = (long)N * H;
  return (int)(R < JDET_DWCONV_MAX_SLABS ? R : JDET_DWCONV_MAX_SLABS);
}

template <int MODE>
int launch_conv(const float* x, const float* w, const float* bias, const float* gy, const Geom& g, float* y,
                hipStream_t st) {
  const long total = (long)g.N * g.H * g.WT * g.C4;   // < 2^31 / 4
  hipLaunchKernelGGL((dwconv_kernel<MODE>), dim3(jdet_cdiv(total, 256)), dim3(256), 0, st, (const float4*)x,
                     (const float4*)w, (const float4*)bias, (const float4*)gy, g, (int)total, (float4*)y);
  return jdet_launch_status();
}

}  // namespace

JDET_API int jdet_dwconv_nhwc_forward(const float* x, const float* w, const float* bias, int N, int H, int W, int C,
                                      int KH, int KW, int pad_h, int pad_w, int dil_h, int dil_w, int act, float* y,
                                      jdet_stream_t stream) {
  Geom g;
  if (!x || !w || !y || (act != JDET_DWCONV_ACT_NONE && act != JDET_DWCONV_ACT_GELU)) return JDET_E_BADARG;
  if (int e = make_geom(N, H, W, C, KH, KW, pad_h, pad_w, dil_h, dil_w, &g)) return e;
  if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y)) return JDET_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  return act == JDET_DWCONV_ACT_GELU ? launch_conv<1>(x, w, bias, nullptr, g, y, st)
                                     : launch_conv<0>(x, w, bias, nullptr, g, y, st);
}

JDET_API int jdet_dwconv_gelu_backward(const float* x, const float* w, const float* bias, const float* g_y, int N, int H,
                                       int W, int C, int KH, int KW, int pad_h, int pad_w, int dil_h, int dil_w,
                                       float* g_z, jdet_stream_t stream) {
  Geom g;
  if (!x || !w || !g_y || !g_z) return JDET_E_BADARG;
  if (int e = make_geom(N, H, W, C, KH, KW, pad_h, pad_w, dil_h, dil_w, &g)) return e;
  if (!aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(g_y) || !aligned16(g_z)) return JDET_E_BADARG;
  return launch_conv<2>(x, w, bias, g_y, g, g_z, (hipStream_t)stream);
}

JDET_API size_t jdet_dwconv_nhwc_wgrad_workspace(int N, int H, int W, int C, int KH, int KW) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || KH < 1 || KW < 1 || C % 4 != 0 || KH > kMaxK || KW > kMaxK) return 0;
  return (size_t)slabs_of(N, H) * ((size_t)KH * KW + 1) * (size_t)C * sizeof(float);
}

JDET_API int jdet_dwconv_nhwc_wgrad(const float* x, const float* g, int N, int H, int W, int C, int KH, int KW,
                                    int pad_h, int pad_w, int dil_h, int dil_w, float* gw, float* gb, void* workspace,
                                    size_t workspace_bytes, jdet_stream_t stream) {
  Geom q;
  if (!x || !g || !gw || !workspace) return JDET_E_BADARG;
  if (int e = make_geom(N, H, W, C, KH, KW, pad_h, pad_w, dil_h, dil_w, &q)) return e;
  if (!aligned16(x) || !aligned16(g) || !aligned16(gw) || !aligned16(gb) || !aligned16(workspace)) return JDET_E_BADARG;
  if (workspace_bytes < jdet_dwconv_nhwc_wgrad_workspace(N, H, W, C, KH, KW)) return JDET_E_WORKSPACE;
  const int S = slabs_of(N, H), taps = KH * KW;
  const int rows_per_slab = (N * H + S - 1) / S;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dwconv_wgrad_partial_kernel, dim3(jdet_cdiv((long)(taps + 1) * q.C4, 256), S), dim3(256), 0, st,
                     (const float4*)x, (const float4*)g, q, rows_per_slab, (float4*)workspace);
  if (int e = jdet_launch_status()) return e;
  hipLaunchKernelGGL(dwconv_wgrad_finish_kernel, dim3((taps + 1) * q.C4), dim3(64), 0, st, (const float4*)workspace, S,
                     taps, q.C4, (float4*)gw, (float4*)gb);
  return jdet_launch_status();
}
