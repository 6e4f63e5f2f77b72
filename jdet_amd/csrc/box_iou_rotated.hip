// Rotated-box IoU and rotated NMS for gfx950 (MI355X).
//
// Reference semantics:
//   python/jdet/ops/box_iou_rotated.py:L13-310   (vertices, 16 edge intersections + 8 containment
//                                                  tests, Graham hull, shoelace area, IoU)
//   python/jdet/ops/box_iou_rotated_v1.py:L69-76 (opposite vertex convention)
//   python/jdet/ops/nms_rotated.py:L281-310      (label column -> IoU 0 across labels)
//   python/jdet/ops/nms_rotated.py:L414-449      (CPU greedy rule, `>=`), L352-411 + L450-493
//                                                (CUDA 64x64 bitmask kernel, `>`, host scan)
//
// MI355X design (not a translation):
//   * IoU is ALU/latency bound (20 B per box, ~400-3000 flop per overlapping pair).  The
//     intersection-point array (<= 24 points) is the only dynamically indexed state; it lives
//     in LDS as [slot][lane] (bank = lane -> conflict-free for any per-lane slot), everything
//     else is fully unrolled into VGPRs -> no scratch memory.
//   * a conservative circumscribed-circle test returns the exact 0 the reference would compute
//     for clearly disjoint pairs (the overwhelming majority) before any heavy work.
//   * float/double mix, comparison constants and operation order follow the reference's CPU
//     path literally and the file is compiled with -ffp-contract=off, so IoU values -- and
//     therefore NMS keep masks and assigner labels -- are bit-identical to the CPU oracle.
//     The hull sort replays libstdc++'s insertion sort (what std::sort runs for <= 16 elements).
//   * NMS: wave64 == 64-bit suppression word.  One wave per 64x64 tile of score-sorted boxes:
//     lanes are the 64 column boxes, the row box is wave-uniform, __ballot() yields the mask
//     word directly; only upper-triangle tiles run.  The greedy scan stays on the device (one
//     workgroup: diagonal tile resolved by v_readlane chain, remaining words OR-ed in parallel
//     into LDS) -- no cudaDeviceSynchronize + host loop as in the reference.
//   * the IoU of one pair (single_box_iou / iou_dispatch and their helpers) lives in rotated_iou.h: the ATSS
//     assigner (atss_assign.hip) calls the same function for its candidate pairs.
#include "common.h"
#include "nms_scan.h"
#include "rotated_iou.h"

namespace {

// ---------------------------------------------------------------------------------------------
// pairwise IoU: one lane per (i, j), j fastest (coalesced stores)
// ---------------------------------------------------------------------------------------------
constexpr int kIouBlock = 128;

__global__ __launch_bounds__(kIouBlock) void box_iou_kernel(const float* __restrict__ boxes1, int n1,
                                                            const float* __restrict__ boxes2, int n2,
                                                            int stride, int version, int sort_mode,
                                                            float* __restrict__ ious) {
  __shared__ float s_x[24 * kIouBlock];
  __shared__ float s_y[24 * kIouBlock];
  LanePts<kIouBlock> q;
  q.x = s_x + threadIdx.x;
  q.y = s_y + threadIdx.x;
  const long total = (long)n1 * n2;
  for (long p = (long)blockIdx.x * kIouBlock + threadIdx.x; p < total; p += (long)gridDim.x * kIouBlock) {
    const int i = (int)(p / n2), j = (int)(p % n2);
    float a[5], b[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
      a[k] = boxes1[(size_t)i * stride + k];
      b[k] = boxes2[(size_t)j * stride + k];
    }
    ious[p] = iou_dispatch<kIouBlock>(a, b, version, sort_mode, q);
  }
}

// ---------------------------------------------------------------------------------------------
// NMS: tile mask kernel (one wave per 64x64 tile) + on-device greedy scan
// ---------------------------------------------------------------------------------------------
// min / max label of the 64 boxes of tile `blk` (box_len == 6)
__device__ __forceinline__ void tile_label_range(const float* __restrict__ dets, const int32_t* __restrict__ order,
                                                 int n, int blk, int lane, float& lo, float& hi) {
  const int pos = blk * 64 + lane;
  const float l = pos < n ? dets[(size_t)order[pos] * 6 + 5] : 0.f;
  lo = pos < n ? l : INFINITY;
  hi = pos < n ? l : -INFINITY;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
}

// `mask` and `tile_jmax` arrive zeroed.  Tiles whose label ranges are disjoint (ml_nms with the boxes visited
// class by class: almost all of them) return at once; tile_jmax[r] = last column block of row block r that can hold
// a set bit, so that the scan reads only those.
// HBB: the boxes are (xc, yc, w, h, 0 [, label]) -- axis-aligned; the overlap is the rectangle formula
// inter / (a + b - inter) instead of the polygon clipping (same value up to rounding, ~30x fewer instructions: the
// RPN proposal NMS of the two-stage detectors, 8.7 k boxes per image, spent 0.55-0.74 ms here).
template <bool HBB>
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ dets, int n, int box_len,
                                                      const int32_t* __restrict__ order, float thr,
                                                      int cmp_ge, int sort_mode,
                                                      unsigned long long* __restrict__ mask,
                                                      int* __restrict__ tile_jmax) {
  const int row_blk = blockIdx.y, col_blk = blockIdx.x;
  if (col_blk < row_blk) return;  // only the upper triangle is ever read by the scan
  const int lane = threadIdx.x;
  if (box_len == 6 && col_blk != row_blk) {
    float rlo, rhi, clo, chi;
    tile_label_range(dets, order, n, row_blk, lane, rlo, rhi);
    tile_label_range(dets, order, n, col_blk, lane, clo, chi);
    if (rhi < clo || chi < rlo) return;   // no pair of equal labels in this tile
  }
  if (lane == 0) atomicMax(&tile_jmax[row_blk], col_blk);
  __shared__ float s_x[24 * 64];
  __shared__ float s_y[24 * 64];
  __shared__ float s_row[64 * 6];                  // the tile's row boxes (lane i staged row i)
  __shared__ float s_col[64 * 6];
  __shared__ unsigned short s_pair[64 * 64];       // candidate pairs (row << 6 | column), rotated boxes only
  __shared__ unsigned long long s_word[64];
  LanePts<64> q;
  q.x = s_x + lane;
  q.y = s_y + lane;
  const int col_blocks = (n + 63) >> 6;
  const int col = col_blk * 64 + lane;  // position in visiting order
  const bool col_ok = col < n;
  float cb[6] = {0, 0, 0, 0, 0, 0};
  if (col_ok) {
    const float* p = dets + (size_t)order[col] * box_len;
#pragma unroll
    for (int k = 0; k < 5; k++) cb[k] = p[k];
    if (box_len == 6) cb[5] = p[5];
  }
  const int rows = min(64, n - row_blk * 64);
  {
    float rb[6] = {0, 0, 0, 0, 0, 0};
    if (lane < rows) {
      const float* p = dets + (size_t)order[row_blk * 64 + lane] * box_len;
#pragma unroll
      for (int k = 0; k < 5; k++) rb[k] = p[k];
      if (box_len == 6) rb[5] = p[5];
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
      s_row[lane * 6 + k] = rb[k];
      s_col[lane * 6 + k] = cb[k];
    }
    s_word[lane] = 0ull;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  if (HBB) {
    for (int i = 0; i < rows; i++) {
      const int row = row_blk * 64 + i;
      float rb[6];
#pragma unroll
      for (int k = 0; k < 6; k++) rb[k] = s_row[i * 6 + k];   // same address in every lane: broadcast
      bool hit = false;
      if (col_ok && col > row && !(box_len == 6 && rb[5] != cb[5])) {
        const float iw = fminf(rb[0] + 0.5f * rb[2], cb[0] + 0.5f * cb[2]) - fmaxf(rb[0] - 0.5f * rb[2], cb[0] - 0.5f * cb[2]);
        const float ih = fminf(rb[1] + 0.5f * rb[3], cb[1] + 0.5f * cb[3]) - fmaxf(rb[1] - 0.5f * rb[3], cb[1] - 0.5f * cb[3]);
        const float inter = fmaxf(iw, 0.f) * fmaxf(ih, 0.f);
        const float uni = rb[2] * rb[3] + cb[2] * cb[3] - inter;
        const float ovr = uni > 0.f ? inter / uni : 0.f;
        hit = cmp_ge ? (ovr >= thr) : (ovr > thr);
      }
      const unsigned long long word = __ballot(hit);
      if (lane == 0 && word) mask[(size_t)row * col_blocks + col_blk] = word;
    }
    return;
  }
  // Rotated boxes, two phases.  The polygon clipping costs thousands of instructions and only pairs whose
  // circumscribed circles meet need it: running it inside the row loop left most lanes of most iterations idle while
  // one pair was being clipped (355 us for 2000 boxes, 4x the per-pair time of box_iou_kernel).
  //   1. every (row, column) pair of the tile that is in order, of one label (ml_nms: different labels -> IoU 0,
  //      nms_rotated.py:L283-286) and not surely disjoint is appended to a list (one cheap pass, lane = column);
  //   2. the list is clipped 64 pairs at a time, one pair per lane, and the hits OR-ed into the rows' words.
  // Same pairs, same function, same bits as before.  A threshold that an IoU of exactly 0 passes makes EVERY pair a
  // hit: then the disjoint ones have to stay in the list.
  const bool zero_hits = cmp_ge ? !(thr > 0.f) : (thr < 0.f);
  int total = 0;
  for (int i = 0; i < rows; i++) {
    const int row = row_blk * 64 + i;
    float rb[6];
#pragma unroll
    for (int k = 0; k < 6; k++) rb[k] = s_row[i * 6 + k];
    const bool cand = col_ok && col > row && !(box_len == 6 && rb[5] != cb[5]) &&
                      (zero_hits || !surely_disjoint(rb, cb));
    const unsigned long long word = __ballot(cand);
    if (cand) s_pair[total + __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0))] =
        (unsigned short)((i << 6) | lane);
    total += __popcll(word);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int t0 = 0; t0 < total; t0 += 64) {
    const int t = t0 + lane;
    if (t < total) {
      const int pr = s_pair[t];
      const int i = pr >> 6, j = pr & 63;
      float rb[5], b2[5];
#pragma unroll
      for (int k = 0; k < 5; k++) {
        rb[k] = s_row[i * 6 + k];
        b2[k] = s_col[j * 6 + k];
      }
      // argument order (earlier, later) as in the CPU loop L443
      const float ovr = iou_dispatch<64>(rb, b2, 0, sort_mode, q);
      if (cmp_ge ? (ovr >= thr) : (ovr > thr)) atomicOr(&s_word[i], 1ull << j);
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  if (lane < rows) {
    const unsigned long long word = s_word[lane];
    if (word) mask[(size_t)(row_blk * 64 + lane) * col_blocks + col_blk] = word;
  }
}

}  // namespace

JDET_API int jdet_box_iou_rotated(const float* boxes1, int n1, const float* boxes2, int n2, int stride,
                                  int version, int sort_mode, float* ious, jdet_stream_t stream) {
  if (n1 < 0 || n2 < 0 || stride < 5 || (version != 0 && version != 1) ||
      (sort_mode != 0 && sort_mode != 1))
    return JDET_E_BADARG;
  if (n1 == 0 || n2 == 0) return JDET_OK;
  if (!boxes1 || !boxes2 || !ious) return JDET_E_BADARG;
  const long total = (long)n1 * n2;
  const int grid = (int)((total + kIouBlock - 1) / kIouBlock > 1048576 ? 1048576
                                                                       : (total + kIouBlock - 1) / kIouBlock);
  hipLaunchKernelGGL(box_iou_kernel, dim3(grid), dim3(kIouBlock), 0, (hipStream_t)stream, boxes1, n1,
                     boxes2, n2, stride, version, sort_mode, ious);
  return jdet_launch_status();
}

JDET_API size_t jdet_nms_rotated_workspace(int n) { return jdet_nms::workspace_bytes(n); }

// horizontal != 0: every angle is 0 (the caller's promise): rectangle overlap instead of polygon clipping.
// n_labels > 1 (box_len 6 only): the labels are the integers 0 .. n_labels-1 and `order` visits the boxes label by
// label -- one scan workgroup per label instead of one for all.
JDET_API int jdet_nms_labeled(const float* dets, int n, int box_len, const int32_t* order, float iou_threshold,
                              int cmp_ge, int sort_mode, int horizontal, int n_labels, uint8_t* keep,
                              void* workspace, size_t workspace_bytes, jdet_stream_t stream) {
  if (n < 0 || (box_len != 5 && box_len != 6) || (sort_mode != 0 && sort_mode != 1) || n_labels < 1 ||
      n_labels > 65535 || (n_labels > 1 && box_len != 6))
    return JDET_E_BADARG;
  if (n == 0) return JDET_OK;
  if (!dets || !order || !keep || !workspace) return JDET_E_BADARG;
  if (workspace_bytes < jdet_nms_rotated_workspace(n)) return JDET_E_WORKSPACE;
  const int col_blocks = (n + 63) >> 6;
  if (col_blocks > jdet_nms::kScanMaxWords) return JDET_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* mask = (unsigned long long*)workspace;
  int* tile_jmax = (int*)((char*)workspace + jdet_nms::mask_bytes(n));
  int e = jdet_zero_async(workspace, jdet_nms_rotated_workspace(n), st);
  if (e) return e;
  if (horizontal)
    hipLaunchKernelGGL(nms_mask_kernel<true>, dim3(col_blocks, col_blocks), dim3(64), 0, st, dets, n, box_len,
                       order, iou_threshold, cmp_ge ? 1 : 0, sort_mode, mask, tile_jmax);
  else
    hipLaunchKernelGGL(nms_mask_kernel<false>, dim3(col_blocks, col_blocks), dim3(64), 0, st, dets, n, box_len,
                       order, iou_threshold, cmp_ge ? 1 : 0, sort_mode, mask, tile_jmax);
  e = jdet_launch_status();
  if (e) return e;
  return jdet_nms::launch_scan(mask, n, order, tile_jmax, dets + 5, 6, n_labels, keep, st);
}

JDET_API int jdet_nms_rotated(const float* dets, int n, int box_len, const int32_t* order,
                              float iou_threshold, int cmp_ge, int sort_mode, uint8_t* keep,
                              void* workspace, size_t workspace_bytes, jdet_stream_t stream) {
  return jdet_nms_labeled(dets, n, box_len, order, iou_threshold, cmp_ge, sort_mode, 0, 1, keep, workspace,
                          workspace_bytes, stream);
}
