// The view-consistency loss of H2RBox on gfx950 (MI355X), forward and backward.
//
// Reference semantics (a Jittor tensor program with a host sync at every step):
//   python/jdet/models/roi_heads/h2rbox_head.py:L399-506   nonzero() of the positives, a per-level Python loop mapping
//                                                          them to cells of the rotated view, boolean-mask scatters,
//                                                          .any(), gathers, distance2obb, the rotated targets
//   python/jdet/models/losses/h2rbox_loss.py:L42-66        centre L1 + min(shape IoU + |sin|, swapped IoU + |cos|)
//   python/jdet/models/boxes/box_ops.py:L694-707           distance2obb (regular_obb included)
// The rules (cell map, tie rule, validity, target, terms, gradient conventions) are stated in include/jdet_hip.h.
//
// MI355X design (not a translation).  Dense and fixed-shape: one thread owns one view-1 point of one image, finds its
// level and cell from its index, and skips everything (both prediction reads included) when its weight is 0 or its
// cell leaves the level -- so the geometry runs for the positives only while nothing is gathered, counted or synced.
// The per-row terms go out unreduced (4 words per point); the caller sums them and takes the reference's SCALAR
// minimum on the device.  A row's arithmetic runs in double and is rounded once on output: a few hundred operations,
// for the positives only.  The backward pass recomputes the row (two 5-word reads: cheaper than storing the
// intermediates) and routes the view-2 gradient through a per-row scratch that each view-2 point then gathers from the
// 3 x 3 block its inverse map points at, in ascending index: deterministic, no floating-point atomics.
// Everything is latency-bound at N ~ 22k points per image; the win is the absence of host syncs and of ~60 launches.
#include "common.h"
#include "jdet_hip.h"

namespace {

constexpr int kMaxLevels = JDET_FCOS_MAX_LEVELS;
constexpr int kMaxAgnostic = JDET_H2RBOX_MAX_AGNOSTIC;
constexpr int kBlock = 256;

struct AugParams {
  int32_t H[kMaxLevels], W[kMaxLevels], stride[kMaxLevels];
  int32_t off[kMaxLevels + 1];    // points of level l: [off[l], off[l+1]); levels beyond L are empty
  int32_t agnostic[kMaxAgnostic];
  int L, N, n_agnostic;
  float rot, cs, sn, ccx, ccy;    // (ccx, ccy) = ((crop_w - 1) / 2, (crop_h - 1) / 2)
  float shape_weight, angle_weight, eps;
};

struct Box {
  double cx, cy, w, h, a;
};

// torch.remainder (floor-mod) of a by b > 0
__device__ __forceinline__ double floor_mod(double a, double b) {
  double r = fmod(a, b);
  if (r != 0.0 && r < 0.0) r += b;
  return r;
}

// distance2obb of one row at one point; `swapped` = regular_obb exchanged w and h
__device__ __forceinline__ Box decode(double px, double py, const double* __restrict__ row, double* c, double* s, double* ox,
                                      double* oy, bool* swapped) {
  const double half_pi = 1.5707963267948966, pi = 3.141592653589793;
  const double l = row[0], t = row[1], r = row[2], b = row[3], th = row[4];
  sincos(th, s, c);
  const double w = l + r, h = t + b;
  *ox = (r - l) / 2;
  *oy = (b - t) / 2;
  Box o;
  o.cx = px + ((*c) * (*ox) + (*s) * (*oy));
  o.cy = py + (-(*s) * (*ox) + (*c) * (*oy));
  const bool keep = w > h;
  *swapped = !keep;
  o.w = keep ? w : h;
  o.h = keep ? h : w;
  o.a = floor_mod((keep ? th : th + half_pi) - (-half_pi), pi) + (-half_pi);
  return o;
}

// gradient of decode: (gcx, gcy, gw, gh, ga) of the regular box -> g[5] of the row [l, t, r, b, theta]
__device__ __forceinline__ void decode_backward(double c, double s, double ox, double oy, bool swapped, double gcx, double gcy,
                                                double gwr, double ghr, double ga, double* __restrict__ g) {
  const double gw = swapped ? ghr : gwr, gh = swapped ? gwr : ghr;
  const double gox = gcx * c + gcy * (-s), goy = gcx * s + gcy * c;
  g[0] = -gox / 2 + gw;
  g[1] = -goy / 2 + gh;
  g[2] = gox / 2 + gw;
  g[3] = goy / 2 + gh;
  g[4] = ga + gcx * (-s * ox + c * oy) + gcy * (-c * ox - s * oy);
}

// -log(max(iou, eps)) of [-pw, -ph, pw, ph] against [-tw, -th, tw, th] (bbox_overlaps, is_aligned) and, when `grad`,
// its derivatives by (pw, ph, tw, th)
__device__ __forceinline__ double centred_iou_loss(double pw, double ph, double tw, double th, double eps, bool grad,
                                                  double* g) {
  const double a1 = (pw - (-pw)) * (ph - (-ph)), a2 = (tw - (-tw)) * (th - (-th));
  const bool px = pw < tw, py = ph < th;          // which side is the min (and, negated, the max of the negatives)
  const double rx = (px ? pw : tw) - (px ? -pw : -tw), ry = (py ? ph : th) - (py ? -ph : -th);
  const bool cx = rx > 0.0, cy = ry > 0.0;
  const double wx = cx ? rx : 0.0, wy = cy ? ry : 0.0;
  const double overlap = wx * wy;
  const double uraw = a1 + a2 - overlap;
  const bool uclamp = !(uraw > eps);              // max(union, eps)
  const double u = uclamp ? eps : uraw;
  const double iou = overlap / u;
  const bool iclamp = !(iou > eps);
  const double loss = -log(iclamp ? eps : iou);
  if (grad) {
    g[0] = g[1] = g[2] = g[3] = 0.0;
    if (!iclamp) {
      const double dl = -1.0 / iou;                                   // d loss / d iou
      const double di_do = uclamp ? 1.0 / u : 1.0 / u + overlap / (u * u);   // d iou / d overlap (union moves by -1)
      const double di_da = uclamp ? 0.0 : -overlap / (u * u);         // d iou / d a1 = d iou / d a2
      const double go = dl * di_do, gar = dl * di_da;
      const double gwx = go * wy, gwy = go * wx;
      const double two_x = cx ? 2.0 : 0.0, two_y = cy ? 2.0 : 0.0;
      g[0] = (px ? two_x * gwx : 0.0) + gar * 4.0 * ph;
      g[1] = (py ? two_y * gwy : 0.0) + gar * 4.0 * pw;
      g[2] = (px ? 0.0 : two_x * gwx) + gar * 4.0 * th;
      g[3] = (py ? 0.0 : two_y * gwy) + gar * 4.0 * tw;
    }
  }
  return loss;
}

struct Cell {
  int level, x, y, q;   // q: the point's index inside its level
};

__device__ __forceinline__ Cell cell_of(const AugParams& P, int p) {
  Cell c;
  c.level = 0;
  while (c.level + 1 < P.L && p >= P.off[c.level + 1]) c.level++;
  c.q = p - P.off[c.level];
  c.y = c.q / P.W[c.level];
  c.x = c.q - c.y * P.W[c.level];
  return c;
}

// the view-2 point of cell (x, y), or -1 when it leaves the level; (xa, ya) its cell
__device__ __forceinline__ int aug_point(const AugParams& P, const Cell& c, int* xa, int* ya) {
  const int w = P.W[c.level], h = P.H[c.level];
  const float cx = (float)(w - 1) / 2, cy = (float)(h - 1) / 2;
  const float dx = (float)c.x - cx, dy = (float)c.y - cy;
  const float fx = rintf(dx * P.cs + dy * (-P.sn) + cx), fy = rintf(dx * P.sn + dy * P.cs + cy);
  if (!(fx >= 0.f && fx < (float)w && fy >= 0.f && fy < (float)h)) return -1;
  *xa = (int)fx;
  *ya = (int)fy;
  return P.off[c.level] + *ya * w + *xa;
}

__device__ __forceinline__ bool is_agnostic(const AugParams& P, const int32_t* __restrict__ labels, size_t o) {
  if (P.n_agnostic == 0) return false;
  const int lab = labels[o] + 1;                  // the reference compares 1-based labels
  bool hit = false;
  for (int k = 0; k < P.n_agnostic; k++) hit = hit || lab == P.agnostic[k];
  return hit;
}

// One row, forward (grad == false: out = terms[4]) or backward (grad == true: g1 = d / d pred row, g2 = d / d pred_aug
// row of sc * centre + sb * branch[k]).
__device__ __forceinline__ void aug_row(const AugParams& P, const Cell& c, int xa, int ya, const float* __restrict__ r1f,
                                        const float* __restrict__ r2f, float wgtf, bool agn, bool grad, int k, float scf,
                                        float sbf, float* __restrict__ terms, float* __restrict__ g1,
                                        float* __restrict__ g2) {
  double r1[5], r2[5];
  for (int i = 0; i < 5; i++) {
    r1[i] = (double)r1f[i];
    r2[i] = (double)r2f[i];
  }
  const double wgt = (double)wgtf, sc = (double)scf, sb = (double)sbf;
  const int stride = P.stride[c.level];
  const double p1x = (double)(c.x * stride + stride / 2), p1y = (double)(c.y * stride + stride / 2);
  const double p2x = (double)(xa * stride + stride / 2), p2y = (double)(ya * stride + stride / 2);
  double c1, s1, ox1, oy1, c2, s2, ox2, oy2;
  bool sw1, sw2;
  const Box V = decode(p1x, p1y, r1, &c1, &s1, &ox1, &oy1, &sw1);
  const Box Q = decode(p2x, p2y, r2, &c2, &s2, &ox2, &oy2, &sw2);
  const double dx = V.cx - P.ccx, dy = V.cy - P.ccy;
  const double tx = dx * P.cs + dy * (-P.sn) + P.ccx, ty = dx * P.sn + dy * P.cs + P.ccy;
  const double amask = agn ? 0.0 : 1.0;
  const double ta = (V.a + P.rot) * amask;
  const double ex = Q.cx - tx, ey = Q.cy - ty, da = Q.a - ta;
  double sd, cd;
  sincos(da, &sd, &cd);
  if (!grad) {
    const double i1 = centred_iou_loss(Q.w, Q.h, V.w, V.h, P.eps, false, nullptr);
    const double i2 = centred_iou_loss(Q.h, Q.w, V.w, V.h, P.eps, false, nullptr);
    terms[0] = (float)(wgt * (fabs(ex) + fabs(ey)));
    terms[1] = (float)(wgt * (P.shape_weight * i1 + P.angle_weight * fabs(sd)));
    terms[2] = (float)(wgt * (P.shape_weight * i2 + P.angle_weight * fabs(cd)));
    terms[3] = wgtf;
    return;
  }
  const double sgn_x = ex > 0.0 ? 1.0 : (ex < 0.0 ? -1.0 : 0.0), sgn_y = ey > 0.0 ? 1.0 : (ey < 0.0 ? -1.0 : 0.0);
  const double gqx = sc * wgt * sgn_x, gqy = sc * wgt * sgn_y;          // by Q.cx, Q.cy; the target's: the negatives
  double gi[4];
  double gqw, gqh;
  double gang;
  const double sbw = sb * wgt;
  if (k == 0) {
    centred_iou_loss(Q.w, Q.h, V.w, V.h, P.eps, true, gi);
    gqw = gi[0];
    gqh = gi[1];
    gang = (sd > 0.0 ? 1.0 : (sd < 0.0 ? -1.0 : 0.0)) * cd;
  } else {
    centred_iou_loss(Q.h, Q.w, V.w, V.h, P.eps, true, gi);
    gqw = gi[1];
    gqh = gi[0];
    gang = -(cd > 0.0 ? 1.0 : (cd < 0.0 ? -1.0 : 0.0)) * sd;
  }
  const double gs = sbw * P.shape_weight, ga = sbw * P.angle_weight * gang;
  double d1[5], d2[5];
  decode_backward(c2, s2, ox2, oy2, sw2, gqx, gqy, gs * gqw, gs * gqh, ga, d2);
  // the target side: centre through the rotation, w and h direct, the angle through the agnostic mask
  const double gtx = -gqx, gty = -gqy;
  const double gvx = gtx * P.cs + gty * P.sn, gvy = gtx * (-P.sn) + gty * P.cs;
  decode_backward(c1, s1, ox1, oy1, sw1, gvx, gvy, gs * gi[2], gs * gi[3], -ga * amask, d1);
  for (int i = 0; i < 5; i++) {
    g1[i] = (float)d1[i];
    g2[i] = (float)d2[i];
  }
}

__global__ __launch_bounds__(kBlock) void aug_forward_kernel(AugParams P, const float* __restrict__ pred,
                                                            const float* __restrict__ pred_aug,
                                                            const float* __restrict__ weight,
                                                            const int32_t* __restrict__ labels,
                                                            float* __restrict__ terms, int32_t* __restrict__ aug_index) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= P.N) return;
  const size_t base = (size_t)blockIdx.y * P.N, o = base + p;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  int q = -1;
  const float wgt = weight[o];
  if (wgt > 0.f) {
    const Cell c = cell_of(P, p);
    int xa, ya;
    q = aug_point(P, c, &xa, &ya);
    if (q >= 0)
      aug_row(P, c, xa, ya, pred + o * 5, pred_aug + (base + q) * 5, wgt, is_agnostic(P, labels, o), false, 0, 0.f, 0.f,
              t, nullptr, nullptr);
  }
  for (int i = 0; i < 4; i++) terms[o * 4 + i] = t[i];        // (scalar stores: the buffer is only 4-byte aligned)
  aug_index[o] = q;
}

__global__ __launch_bounds__(kBlock) void aug_backward_rows_kernel(AugParams P, const float* __restrict__ pred,
                                                                  const float* __restrict__ pred_aug,
                                                                  const float* __restrict__ weight,
                                                                  const int32_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ branch,
                                                                  const float* __restrict__ scale_centre,
                                                                  const float* __restrict__ scale_branch,
                                                                  float* __restrict__ grad_pred,
                                                                  float* __restrict__ contrib) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= P.N) return;
  const size_t base = (size_t)blockIdx.y * P.N, o = base + p;
  float g1[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, g2[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const float wgt = weight[o];
  if (wgt > 0.f) {
    const Cell c = cell_of(P, p);
    int xa, ya;
    const int q = aug_point(P, c, &xa, &ya);
    if (q >= 0)
      aug_row(P, c, xa, ya, pred + o * 5, pred_aug + (base + q) * 5, wgt, is_agnostic(P, labels, o), true,
              branch[0] != 0 ? 1 : 0, scale_centre[0], scale_branch[0], nullptr, g1, g2);
  }
  for (int i = 0; i < 5; i++) {
    grad_pred[o * 5 + i] = g1[i];
    contrib[o * 5 + i] = g2[i];
  }
}

__global__ __launch_bounds__(kBlock) void aug_backward_gather_kernel(AugParams P, const int32_t* __restrict__ aug_index,
                                                                    const float* __restrict__ contrib,
                                                                    float* __restrict__ grad_pred_aug) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= P.N) return;
  const size_t base = (size_t)blockIdx.y * P.N;
  const Cell c = cell_of(P, q);
  const int w = P.W[c.level], h = P.H[c.level];
  const float cx = (float)(w - 1) / 2, cy = (float)(h - 1) / 2;
  const float dx = (float)c.x - cx, dy = (float)c.y - cy;
  // the inverse map: (dx, dy) . [[cos, -sin], [sin, cos]]; clamped so the block stays representable
  const float fx = fminf(fmaxf(rintf(dx * P.cs + dy * P.sn + cx), -2.f), (float)w + 1.f);
  const float fy = fminf(fmaxf(rintf(dx * (-P.sn) + dy * P.cs + cy), -2.f), (float)h + 1.f);
  const int x0 = (int)fx, y0 = (int)fy;
  float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int yy = y0 - 1; yy <= y0 + 1; yy++) {         // ascending view-1 index: rows, then columns
    if (yy < 0 || yy >= h) continue;
    for (int xx = x0 - 1; xx <= x0 + 1; xx++) {
      if (xx < 0 || xx >= w) continue;
      const size_t o = base + P.off[c.level] + (size_t)yy * w + xx;
      if (aug_index[o] == q) {
        for (int i = 0; i < 5; i++) g[i] += contrib[o * 5 + i];
      }
    }
  }
  for (int i = 0; i < 5; i++) grad_pred_aug[(base + q) * 5 + i] = g[i];
}

inline bool finite_f(float v) { return fabsf(v) < 3.0e38f; }

// the checks both entry points share and the launch parameters
int aug_params(const int32_t* levels, int L, const float* pred, const float* pred_aug, const float* weight,
               const int32_t* labels, const int32_t* agnostic, int n_agnostic, int B, float rot, float cos_r, float sin_r,
               int crop_h, int crop_w, float shape_weight, float angle_weight, float eps, AugParams* P) {
  if (!levels || !pred || !pred_aug || !weight || B <= 0 || L <= 0 || crop_h <= 0 || crop_w <= 0 || n_agnostic < 0)
    return JDET_E_BADARG;
  if (n_agnostic > 0 && (!labels || !agnostic)) return JDET_E_BADARG;
  if (!(eps > 0.f) || !finite_f(rot) || !finite_f(cos_r) || !finite_f(sin_r) || !finite_f(shape_weight) ||
      !finite_f(angle_weight))
    return JDET_E_BADARG;
  if (L > kMaxLevels || n_agnostic > kMaxAgnostic || B > 65535) return JDET_E_UNSUPPORTED;
  long N = 0;
  for (int l = 0; l < kMaxLevels; l++) {
    P->off[l] = (int32_t)N;
    if (l < L) {
      const int H = levels[l * 3], W = levels[l * 3 + 1], s = levels[l * 3 + 2];
      if (H <= 0 || W <= 0 || s <= 0) return JDET_E_BADARG;
      if ((long)H * W > 0x7FFFFFFFL || (long)W * s > 0x7FFFFFFFL || (long)H * s > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;
      N += (long)H * W;
      if (N * B * 5 > 0x7FFFFFFFL) return JDET_E_UNSUPPORTED;
      P->H[l] = H;
      P->W[l] = W;
      P->stride[l] = s;
    } else {
      P->H[l] = P->W[l] = P->stride[l] = 1;
    }
  }
  P->off[kMaxLevels] = (int32_t)N;
  for (int k = 0; k < kMaxAgnostic; k++) P->agnostic[k] = k < n_agnostic ? agnostic[k] : 0;
  P->L = L;
  P->N = (int)N;
  P->n_agnostic = n_agnostic;
  P->rot = rot;
  P->cs = cos_r;
  P->sn = sin_r;
  P->ccx = (float)(crop_w - 1) / 2;
  P->ccy = (float)(crop_h - 1) / 2;
  P->shape_weight = shape_weight;
  P->angle_weight = angle_weight;
  P->eps = eps;
  return JDET_OK;
}

}  // namespace

JDET_API int jdet_h2rbox_aug_loss_forward(const int32_t* levels, int L, const float* pred, const float* pred_aug,
                                          const float* weight, const int32_t* labels, const int32_t* agnostic,
                                          int n_agnostic, int B, float rot, float cos_r, float sin_r, int crop_h,
                                          int crop_w, float shape_weight, float angle_weight, float eps, float* terms,
                                          int32_t* aug_index, jdet_stream_t stream) {
  if (!terms || !aug_index) return JDET_E_BADARG;
  AugParams P;
  const int st = aug_params(levels, L, pred, pred_aug, weight, labels, agnostic, n_agnostic, B, rot, cos_r, sin_r, crop_h,
                            crop_w, shape_weight, angle_weight, eps, &P);
  if (st != JDET_OK) return st;
  hipLaunchKernelGGL(aug_forward_kernel, dim3(jdet_cdiv(P.N, kBlock), B), dim3(kBlock), 0, (hipStream_t)stream, P, pred,
                     pred_aug, weight, labels, terms, aug_index);
  return jdet_launch_status();
}

JDET_API int jdet_h2rbox_aug_loss_backward(const int32_t* levels, int L, const float* pred, const float* pred_aug,
                                           const float* weight, const int32_t* labels, const int32_t* agnostic,
                                           int n_agnostic, int B, float rot, float cos_r, float sin_r, int crop_h,
                                           int crop_w, float shape_weight, float angle_weight, float eps,
                                           const int32_t* aug_index, const int32_t* branch, const float* scale_centre,
                                           const float* scale_branch, float* grad_pred, float* grad_pred_aug,
                                           float* contrib, jdet_stream_t stream) {
  if (!aug_index || !branch || !scale_centre || !scale_branch || !grad_pred || !grad_pred_aug || !contrib)
    return JDET_E_BADARG;
  AugParams P;
  const int st = aug_params(levels, L, pred, pred_aug, weight, labels, agnostic, n_agnostic, B, rot, cos_r, sin_r, crop_h,
                            crop_w, shape_weight, angle_weight, eps, &P);
  if (st != JDET_OK) return st;
  const dim3 grid(jdet_cdiv(P.N, kBlock), B);
  hipLaunchKernelGGL(aug_backward_rows_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, P, pred, pred_aug, weight,
                     labels, branch, scale_centre, scale_branch, grad_pred, contrib);
  int e = jdet_launch_status();
  if (e != JDET_OK) return e;
  hipLaunchKernelGGL(aug_backward_gather_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, P, aug_index, contrib,
                     grad_pred_aug);
  return jdet_launch_status();
}
