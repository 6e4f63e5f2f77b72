// The rotated, centre-cropped view of H2RBox on gfx950 (MI355X): H2RBox.rotate_crop for the image tensor.
//
// Reference semantics (a Jittor tensor program):
//   python/jdet/models/networks/h2rbox.py:L35-75   linspace x linspace grid (n, h, w, 2), a (n h w, 2) x (2, 2) matmul,
//                                                  grid_sample(bilinear, padding, align_corners=True) over the whole
//                                                  frame, then the centre crop
// The per-pixel rule is stated in include/jdet_hip.h.
//
// MI355X design (not a translation).  Only the cropped window is computed and the grid never exists: one thread owns one
// output pixel (n, y, x), derives its source position from its index in double (a dozen operations, shared by all C
// channels, so fp32 rounding of the coordinates never moves a sample), and walks the channels with the four corner
// offsets and weights in registers.  Writes are coalesced along x; the reads are a rotated gather of 4 C words per
// pixel, which the 4 MiB L2 of an XCD absorbs (neighbouring pixels share corners).  At the config's 2 x 3 x 1024^2 the
// call moves 25 MB in and 25 MB out: bandwidth-bound, one launch instead of linspace / meshgrid / stack / matmul /
// grid_sample / slice and their 16 MB grid.
#include "common.h"
#include "jdet_hip.h"

namespace {

constexpr int kBlock = 256;

// grid_sample's reflect_coordinates for align_corners = True (about 0 and size - 1), then its clip
__device__ __forceinline__ double reflect_coord(double v, int size) {
  const double span = (double)(size - 1);        // > 0: size >= 2 is checked on the host
  v = fabs(v);
  const double extra = fmod(v, span);
  const bool even = fmod(floor(v / span), 2.0) == 0.0;
  return even ? extra : span - extra;
}

__device__ __forceinline__ double clip_coord(double v, int size) { return fmin((double)(size - 1), fmax(v, 0.0)); }

__global__ __launch_bounds__(kBlock) void rotate_crop_kernel(const float* __restrict__ img, int C, int H, int W, int out_h,
                                                            int out_w, double cs, double sn, int identity, int padding,
                                                            float* __restrict__ out) {
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= out_h * out_w) return;
  const int n = blockIdx.y;
  const int y = pix / out_w, x = pix - y * out_w;
  const int X = x + (W - out_w) / 2, Y = y + (H - out_h) / 2;
  const size_t plane = (size_t)H * W, oplane = (size_t)out_h * out_w;
  const float* src = img + (size_t)n * C * plane;
  float* dst = out + (size_t)n * C * oplane + pix;
  if (identity) {                                   // theta == 0: the reference only slices
    for (int c = 0; c < C; c++) dst[c * oplane] = src[c * plane + (size_t)Y * W + X];
    return;
  }
  const double gx = -1.0 + 2.0 * (double)X / (double)(W - 1), gy = -1.0 + 2.0 * (double)Y / (double)(H - 1);
  const double sx = gx * cs + gy * sn, sy = -gx * sn + gy * cs;
  double ix = (sx + 1.0) / 2.0 * (double)(W - 1), iy = (sy + 1.0) / 2.0 * (double)(H - 1);
  if (padding == JDET_PAD_REFLECTION) {
    ix = reflect_coord(ix, W);
    iy = reflect_coord(iy, H);
  }
  if (padding != JDET_PAD_ZEROS) {
    ix = clip_coord(ix, W);
    iy = clip_coord(iy, H);
  }
  // (zeros padding: positions far outside give corners outside; clamp before the cast so the int never overflows)
  ix = fmin(fmax(ix, -2.0), (double)W + 1.0);
  iy = fmin(fmax(iy, -2.0), (double)H + 1.0);
  const double fx = floor(ix), fy = floor(iy);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const double ax = ix - fx, ay = iy - fy;
  const bool inx0 = x0 >= 0 && x0 < W, inx1 = x1 >= 0 && x1 < W, iny0 = y0 >= 0 && y0 < H, iny1 = y1 >= 0 && y1 < H;
  // a corner outside the frame keeps weight 0 and offset 0: never read
  const float wnw = inx0 && iny0 ? (float)((1.0 - ax) * (1.0 - ay)) : 0.f;
  const float wne = inx1 && iny0 ? (float)(ax * (1.0 - ay)) : 0.f;
  const float wsw = inx0 && iny1 ? (float)((1.0 - ax) * ay) : 0.f;
  const float wse = inx1 && iny1 ? (float)(ax * ay) : 0.f;
  const size_t onw = inx0 && iny0 ? (size_t)y0 * W + x0 : 0, one = inx1 && iny0 ? (size_t)y0 * W + x1 : 0;
  const size_t osw = inx0 && iny1 ? (size_t)y1 * W + x0 : 0, ose = inx1 && iny1 ? (size_t)y1 * W + x1 : 0;
  for (int c = 0; c < C; c++) {
    const float* p = src + c * plane;
    float v = p[onw] * wnw;
    v += p[one] * wne;
    v += p[osw] * wsw;
    v += p[ose] * wse;
    dst[c * oplane] = v;
  }
}

}  // namespace

JDET_API int jdet_rotate_crop(const float* img, int N, int C, int H, int W, int out_h, int out_w, float cos_t,
                              float sin_t, int padding, float* out, jdet_stream_t stream) {
  if (!img || !out || N <= 0 || C <= 0 || out_h <= 0 || out_w <= 0) return JDET_E_BADARG;
  if (H < 2 || W < 2 || out_h > H || out_w > W) return JDET_E_BADARG;
  if (padding != JDET_PAD_ZEROS && padding != JDET_PAD_BORDER && padding != JDET_PAD_REFLECTION) return JDET_E_BADARG;
  if (!(fabsf(cos_t) < 3.0e38f) || !(fabsf(sin_t) < 3.0e38f)) return JDET_E_BADARG;
  if (N > 65535 || (long)N * C * H * W > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;     // (N is the grid's y extent)
  const int identity = cos_t == 1.0f && sin_t == 0.0f;
  hipLaunchKernelGGL(rotate_crop_kernel, dim3(jdet_cdiv((long)out_h * out_w, kBlock), N), dim3(kBlock), 0,
                     (hipStream_t)stream, img, C, H, W, out_h, out_w, (double)cos_t, (double)sin_t, identity, padding, out);
  return jdet_launch_status();
}
