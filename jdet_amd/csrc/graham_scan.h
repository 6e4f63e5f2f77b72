// The Graham scan of ops/convex_sort.py (L4-65, L159-194) on one masked point set, as a device function shared by
// convex_sort_kernel (convex_ops.hip: points, masks and indices in global memory) and the polygon IoU loss
// (poly_iou_loss.hip: points and masks in LDS, indices thread-private).  The callers hand in accessors, so both read
// their own layout and run the same operations in the same order:
//   start   argmin of m * y + (1 - m) * 1e7, first minimum (L169-171)
//   order   stable argsort of the cosine to the start point, descending (L175-176)
//   scan    skipping masked points and points within 1e-3 of the stack top; -1 fills the unused index slots
#pragma once
#include <hip/hip_runtime.h>

// px(i), py(i), mk(i): coordinates and 0/1 mask of point i; idx(i): int& slot i of npts + circular indices.
// Returns the number of hull points (the closing index of `circular` not counted).
template <int MAXN, class PX, class PY, class MK, class IDX>
__device__ __forceinline__ int jdet_graham_scan(PX px, PY py, MK mk, int npts, int circular, IDX idx) {
  const int index_size = circular ? npts + 1 : npts;
  for (int i = 0; i < index_size; i++) idx(i) = -1;
  int start = 0;
  float best = 0.f;
  for (int i = 0; i < npts; i++) {
    const float v = mk(i) * py(i) + (1 - mk(i)) * 10000000.f;
    if (i == 0 || v < best) {
      best = v;
      start = i;
    }
  }
  const float sx = px(start), sy = py(start);
  float key[MAXN];
  int order[MAXN];
  for (int i = 0; i < npts; i++) {
    const float dx = px(i) - sx, dy = py(i) - sy;
    const float c = dx / sqrtf(dx * dx + dy * dy + 0.000001f);
    int j = i;
    while (j > 0 && key[j - 1] < c) {
      key[j] = key[j - 1];
      order[j] = order[j - 1];
      j--;
    }
    key[j] = c;
    order[j] = i;
  }
  idx(0) = start;
  int c_i = 0;
  for (int _j = 0; _j < npts; _j++) {
    const int j = order[_j];
    if (j == start) continue;
    if (mk(j) < 0.5f) continue;
    const float x0 = px(j), y0 = py(j);
    float x1 = px(idx(c_i)), y1 = py(idx(c_i));
    const float d = (x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0);
    if ((double)d < 0.000001) continue;
    if (c_i < 2) {
      idx(++c_i) = j;
    } else {
      float x2 = px(idx(c_i - 1)), y2 = py(idx(c_i - 1));
      while (1) {
        const float t = (x1 - x2) * (y0 - y2) - (y1 - y2) * (x0 - x2);
        if (t >= 0) {
          idx(++c_i) = j;
          break;
        }
        if (c_i <= 1) {
          idx(c_i) = j;
          break;
        }
        c_i--;
        x1 = px(idx(c_i));
        y1 = py(idx(c_i));
        x2 = px(idx(c_i - 1));
        y2 = py(idx(c_i - 1));
      }
    }
  }
  const int n_hull = c_i + 1;
  if (circular) idx(++c_i) = idx(0);
  return n_hull;
}
