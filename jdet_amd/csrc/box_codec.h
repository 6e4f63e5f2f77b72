// Device arithmetic of the rotated delta decoder (models/boxes/box_ops.py:L176-178 norm_angle, L229-285
// delta2bbox_rotated), shared by the codec kernel (box_codec_assign.hip) and the Gaussian box losses
// (gaussian_loss.hip), which decode inside their loss pass.  One definition, so both round alike: the loss kernel
// instantiates it with its forward-mode dual type, whose value part performs the same float operations in the
// same order (with -ffp-contract=off, as the Makefile builds every kernel).
#pragma once
#include "common.h"

namespace {

struct Vec5 {
  float v[5];
};

__device__ __forceinline__ float codec_val(float x) { return x; }
__device__ __forceinline__ float codec_exp(float x) { return expf(x); }
__device__ __forceinline__ float codec_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// floor-mod norm_angle: (a + pi/4) mod pi - pi/4   (box_ops.py:L176-178, range [-pi/4, pi]).  The floor term is a
// step function: its derivative is zero, so it is evaluated on the value alone.
template <class T>
__device__ __forceinline__ T norm_angle(T a) {
  const float lo = (float)(-M_PI / 4), span = (float)M_PI;
  const T x = a - lo;
  const T r = x - floorf(codec_val(x) / span) * span;  // python-style % for a positive modulus
  return r + lo;
}

// one box: roi r (5 floats), deltas d (5 values) -> o (5 values); max_ratio = |log(wh_ratio_clip)|
template <class T>
__device__ __forceinline__ void delta2bbox_one(const float* __restrict__ r, const T* d, const Vec5& means,
                                               const Vec5& stds, float max_ratio, T* o) {
  const T dx = d[0] * stds.v[0] + means.v[0];
  const T dy = d[1] * stds.v[1] + means.v[1];
  T dw = d[2] * stds.v[2] + means.v[2];
  T dh = d[3] * stds.v[3] + means.v[3];
  const T da = d[4] * stds.v[4] + means.v[4];
  dw = codec_clamp(dw, -max_ratio, max_ratio);
  dh = codec_clamp(dh, -max_ratio, max_ratio);
  const float rx = r[0], ry = r[1], rw = r[2], rh = r[3], ra = r[4];
  const float c = cosf(ra), s = sinf(ra);
  o[0] = dx * rw * c - dy * rh * s + rx;
  o[1] = dx * rw * s + dy * rh * c + ry;
  o[2] = rw * codec_exp(dw);
  o[3] = rh * codec_exp(dh);
  o[4] = norm_angle((float)M_PI * da + ra);
}

}  // namespace
