// Top-down step of a feature pyramid with the bilinear resize of the RetinaNet-v1d configs
// (upsample_cfg = dict(mode="bilinear", tf_mode=True), upsample_div_factor = 2) as ONE pass per direction:
// out = (lateral + resize(top)) / div on channels-last maps.  The bilinear counterpart of upsample_add.hip; the resize
// rule is stated in include/jdet_hip_retina.h.  One function (tap_of) evaluates the fp32 source coordinate in both
// directions, so the backward's gather visits exactly the taps the forward read.
#include "common.h"
#include "jdet_hip_retina.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct Tap {
  int i0, i1;
  float d;
};

// dst index -> the two source indices and the weight of the second.  Only out >= in reaches here, so the clamp of the
// rule's `out > in` case is the identity when out == in (x = dst exactly).
__device__ __forceinline__ Tap tap_of(int dst, float scale, int in_size) {
  float x = (float)dst * scale;
  x = fminf(fmaxf(x, 0.f), (float)(in_size - 1));
  Tap t;
  t.i0 = min(max((int)floorf(x), 0), in_size - 1);
  t.d = x - (float)t.i0;
  t.i1 = min(t.i0 + 1, in_size - 1);
  return t;
}

// lat / out (N, H, W, C), top (N, Ht, Wt, C); one thread per (pixel, 4 channels)
__global__ __launch_bounds__(256) void upsample_add_bilinear_fwd_kernel(const float* __restrict__ lat,
                                                                        const float* __restrict__ top,
                                                                        float* __restrict__ out, int N, int H, int W,
                                                                        int Ht, int Wt, int C4, float sy, float sx,
                                                                        float div) {
  const long total = (long)N * H * W * C4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % C4);
    long p = t / C4;
    const int col = (int)(p % W);
    p /= W;
    const int row = (int)(p % H);
    const int n = (int)(p / H);
    const Tap r = tap_of(row, sy, Ht), q = tap_of(col, sx, Wt);
    const v4f* src = reinterpret_cast<const v4f*>(top) + (long)n * Ht * Wt * C4 + c;
    const v4f a = src[((long)r.i0 * Wt + q.i0) * C4], b = src[((long)r.i1 * Wt + q.i0) * C4];
    const v4f cc = src[((long)r.i0 * Wt + q.i1) * C4], d = src[((long)r.i1 * Wt + q.i1) * C4];
    const v4f ab = r.d * b + (1.f - r.d) * a;
    const v4f cd = r.d * d + (1.f - r.d) * cc;
    const v4f v = ab * (1.f - q.d) + cd * q.d;
    reinterpret_cast<v4f*>(out)[t] = (reinterpret_cast<const v4f*>(lat)[t] + v) / div;
  }
}

__device__ __forceinline__ float weight_on(const Tap& t, int src) {
  return (t.i0 == src ? 1.f - t.d : 0.f) + (t.i1 == src ? t.d : 0.f);
}

// g (N, H, W, C) -> g_top (N, Ht, Wt, C): sum over the fine pixels that read (yt, xt), rows then columns ascending, of
// g * (row weight * column weight), divided by div.  The candidates are a range around yt / scale with two indices of
// slack on both sides; tap_of decides.
__global__ __launch_bounds__(256) void upsample_add_bilinear_bwd_kernel(const float* __restrict__ g,
                                                                        float* __restrict__ g_top, int N, int H, int W,
                                                                        int Ht, int Wt, int C4, float sy, float sx,
                                                                        float div) {
  const long total = (long)N * Ht * Wt * C4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % C4);
    long p = t / C4;
    const int xt = (int)(p % Wt);
    p /= Wt;
    const int yt = (int)(p % Ht);
    const int n = (int)(p / Ht);
    const int y_lo = max(0, (int)floorf((float)(yt - 1) / sy) - 2), y_hi = min(H - 1, (int)ceilf((float)(yt + 1) / sy) + 2);
    const int x_lo = max(0, (int)floorf((float)(xt - 1) / sx) - 2), x_hi = min(W - 1, (int)ceilf((float)(xt + 1) / sx) + 2);
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    for (int y = y_lo; y <= y_hi; y++) {
      const float wr = weight_on(tap_of(y, sy, Ht), yt);
      if (wr == 0.f) continue;
      for (int x = x_lo; x <= x_hi; x++) {
        const float wc = weight_on(tap_of(x, sx, Wt), xt);
        if (wc == 0.f) continue;
        acc += reinterpret_cast<const v4f*>(g)[(((long)n * H + y) * W + x) * C4 + c] * (wr * wc);
      }
    }
    reinterpret_cast<v4f*>(g_top)[t] = acc / div;
  }
}

int check(const void* a, const void* b, const void* c, int N, int C, int H, int W, int Ht, int Wt, float div) {
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || Ht <= 0 || Wt <= 0 || div == 0.f) return JDET_E_BADARG;
  if (C % 4 != 0 || H < Ht || W < Wt) return JDET_E_UNSUPPORTED;
  if (N > 0 && (!a || !b || !c)) return JDET_E_BADARG;
  if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0) return JDET_E_BADARG;
  return JDET_OK;
}

unsigned grid_for(long total) {
  long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 262144 ? 262144 : (blocks > 0 ? blocks : 1));
}

}  // namespace

JDET_API int jdet_upsample_add_bilinear_nhwc_forward(const float* lateral, const float* top, int N, int C, int H,
                                                     int W, int Ht, int Wt, float div_factor, float* out,
                                                     jdet_stream_t stream) {
  const int e = check(lateral, top, out, N, C, H, W, Ht, Wt, div_factor);
  if (e || N == 0) return e;
  const long total = (long)N * H * W * (C / 4);
  hipLaunchKernelGGL(upsample_add_bilinear_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     lateral, top, out, N, H, W, Ht, Wt, C / 4, (float)Ht / (float)H, (float)Wt / (float)W, div_factor);
  return jdet_launch_status();
}

JDET_API int jdet_upsample_add_bilinear_nhwc_backward(const float* grad_out, int N, int C, int H, int W, int Ht,
                                                      int Wt, float div_factor, float* grad_top,
                                                      jdet_stream_t stream) {
  const int e = check(grad_out, grad_out, grad_top, N, C, H, W, Ht, Wt, div_factor);
  if (e || N == 0) return e;
  const long total = (long)N * Ht * Wt * (C / 4);
  hipLaunchKernelGGL(upsample_add_bilinear_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     grad_out, grad_top, N, H, W, Ht, Wt, C / 4, (float)Ht / (float)H, (float)Wt / (float)W,
                     div_factor);
  return jdet_launch_status();
}
