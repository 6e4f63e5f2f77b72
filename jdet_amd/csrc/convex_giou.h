// Device functions of the RepPoints convex GIoU: forward-mode dual numbers, Andrew monotone-chain hulls,
// Sutherland-Hodgman clipping, shoelace areas, all in double.  Shared by csrc/convex_giou.hip (jdet_convex_giou, the
// design notes are there) and csrc/convex_giou_loss.hip (jdet_convex_giou_loss): both evaluate jdet_convex_giou_dual,
// so a pair gives the same bits through either entry point.
#pragma once
#include "common.h"

namespace {


struct Dual {
  double v, d;
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dual dconst(double v) { return {v, 0.0}; }

struct DP {
  Dual x, y;
};

__device__ __forceinline__ Dual cross(const DP& o, const DP& a, const DP& b) {
  return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y);
}

constexpr int kMaxPts = 16;   // 9 + 4 hull inputs; a clipped polygon has at most 9 + 4 vertices

// Andrew's monotone chain; p[0..n) is sorted in place; returns the hull size, h counter-clockwise
__device__ int hull(DP* p, int n, DP* h) {
  for (int i = 1; i < n; i++) {        // insertion sort by (x, y) values
    const DP t = p[i];
    int j = i - 1;
    while (j >= 0 && (p[j].x.v > t.x.v || (p[j].x.v == t.x.v && p[j].y.v > t.y.v))) {
      p[j + 1] = p[j];
      j--;
    }
    p[j + 1] = t;
  }
  int m = 0;
  for (int i = 0; i < n; i++) {
    while (m >= 2 && cross(h[m - 2], h[m - 1], p[i]).v <= 0.0) m--;
    h[m++] = p[i];
  }
  const int lower = m + 1;
  for (int i = n - 2; i >= 0; i--) {
    while (m >= lower && cross(h[m - 2], h[m - 1], p[i]).v <= 0.0) m--;
    h[m++] = p[i];
  }
  return m > 1 ? m - 1 : m;            // the last point repeats the first
}

__device__ Dual area(const DP* p, int n) {     // shoelace, positive for counter-clockwise
  Dual s = dconst(0.0);
  for (int i = 0; i < n; i++) {
    const DP& a = p[i];
    const DP& b = p[i + 1 == n ? 0 : i + 1];
    s = s + (a.x * b.y - b.x * a.y);
  }
  return s * dconst(0.5);
}

// convex polygon p (n vertices, any orientation) clipped to the left of every edge of the counter-clockwise convex q
__device__ int clip(DP* p, int n, const DP* q, int nq, DP* tmp) {
  for (int e = 0; e < nq && n > 0; e++) {
    const DP& a = q[e];
    const DP& b = q[e + 1 == nq ? 0 : e + 1];
    int m = 0;
    for (int i = 0; i < n; i++) {
      const DP& cur = p[i];
      const DP& nxt = p[i + 1 == n ? 0 : i + 1];
      const Dual sc = cross(a, b, cur), sn = cross(a, b, nxt);
      const bool in_c = sc.v >= 0.0, in_n = sn.v >= 0.0;
      if (in_c) tmp[m++] = cur;
      if (in_c != in_n) {                       // the edge crosses the line: the crossing point moves with both ends
        const Dual t = sc / (sc - sn);
        tmp[m++] = DP{cur.x + t * (nxt.x - cur.x), cur.y + t * (nxt.y - cur.y)};
      }
    }
    n = m;
    for (int i = 0; i < n; i++) p[i] = tmp[i];
  }
  return n;
}

// GIoU of the hull of 9 points and a quadrilateral with the derivative w.r.t. coordinate j of the point set in the
// dual part (j outside 0..17: the dual part is 0).  pt(i) / quad(i) return coordinate i of the 18 / 8 as float.
template <class PtFn, class QuadFn>
__device__ __forceinline__ Dual jdet_convex_giou_dual(PtFn pt, QuadFn quad, int j) {
  DP pts[kMaxPts], P[kMaxPts], Q[4], work[kMaxPts], tmp[kMaxPts];
  for (int i = 0; i < 9; i++) {
    pts[i].x = Dual{(double)pt(2 * i), j == 2 * i ? 1.0 : 0.0};
    pts[i].y = Dual{(double)pt(2 * i + 1), j == 2 * i + 1 ? 1.0 : 0.0};
  }
  for (int i = 0; i < 4; i++) {
    Q[i].x = dconst((double)quad(2 * i));
    Q[i].y = dconst((double)quad(2 * i + 1));
  }
  for (int i = 0; i < 9; i++) work[i] = pts[i];
  const int nP = hull(work, 9, P);
  Dual aQ = area(Q, 4);
  if (aQ.v < 0.0) {                              // make the quadrilateral counter-clockwise
    const DP t = Q[1];
    Q[1] = Q[3];
    Q[3] = t;
    aQ = dconst(0.0) - aQ;
  }
  const Dual aP = area(P, nP);                   // the hull is counter-clockwise: >= 0
  for (int i = 0; i < nP; i++) work[i] = P[i];
  const int nI = clip(work, nP, Q, 4, tmp);
  Dual inter = nI >= 3 ? area(work, nI) : dconst(0.0);
  if (inter.v < 0.0) inter = dconst(0.0) - inter;
  const Dual uni = aP + aQ - inter;
  for (int i = 0; i < nP; i++) work[i] = P[i];
  for (int i = 0; i < 4; i++) work[nP + i] = Q[i];
  const int nC = hull(work, nP + 4, tmp);
  const Dual encl = area(tmp, nC);
  return inter / uni - (encl - uni) / encl;
}

}  // namespace
