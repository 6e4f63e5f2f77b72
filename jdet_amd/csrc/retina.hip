// The dense side of RetinaHead (models/roi_heads/retina_head.py of the reference, head mode "R" on horizontal anchors;
// include/jdet_hip_retina.h states every rule): ground-truth preparation, one-pass assignment + encoded targets for the
// whole batch, and the decode / threshold / compaction in front of the per-class NMS.  The reference assigns per level
// and per image through an (A, K) IoU matrix with (A, K, 2) corner tensors behind it, and loops over the classes with
// three synchronisations each; here one thread owns one (image, anchor), the gts pass through LDS, and the compaction
// order (class-major, anchor-ascending) comes from a prefix scan over per-workgroup counts, so it never depends on
// which workgroup ran first.
#include "common.h"
#include "jdet_hip_retina.h"

namespace {

constexpr int TPB = 256;
constexpr double PI_D = 3.14159265358979323846;

__device__ __forceinline__ int wave_of(int tid) { return tid >> 6; }

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// ---------------------------------------------------------------------------------------------------- gt preparation
__global__ __launch_bounds__(TPB) void retina_gt_prepare_kernel(const float* __restrict__ gts, int K,
                                                               float* __restrict__ rboxes,
                                                               float* __restrict__ rboxes_h) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k >= K) return;
  const double x = gts[k * 5 + 0], y = gts[k * 5 + 1];
  double w = gts[k * 5 + 2], h = gts[k * 5 + 3], a = gts[k * 5 + 4];
  if (a >= 0) a -= PI_D;
  if (a < -PI_D / 2) {
    a += PI_D / 2;
    const double t = w;
    w = h;
    h = t;
  }
  // cvt2_w_greater_than_h(reverse_hw=False)
  double ow, oh, oa;
  if (w > h) {
    ow = w, oh = h, oa = a - PI_D / 2;
  } else {
    ow = h, oh = w, oa = a;
  }
  rboxes[k * 5 + 0] = (float)x;
  rboxes[k * 5 + 1] = (float)y;
  rboxes[k * 5 + 2] = (float)ow;
  rboxes[k * 5 + 3] = (float)oh;
  rboxes[k * 5 + 4] = (float)oa;
  // rotated_box_to_bbox of (x, y, ow, oh, oa + pi/2): corners tl, tr, br, bl rotated about the centre
  const double c = cos(oa + PI_D / 2), s = sin(oa + PI_D / 2);
  const double xs[4] = {-ow / 2, ow / 2, ow / 2, -ow / 2}, ys[4] = {-oh / 2, -oh / 2, oh / 2, oh / 2};
  double x0 = 0, y0 = 0, x1 = 0, y1 = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double px = c * xs[i] - s * ys[i] + x, py = s * xs[i] + c * ys[i] + y;
    x0 = i == 0 ? px : fmin(x0, px);
    x1 = i == 0 ? px : fmax(x1, px);
    y0 = i == 0 ? py : fmin(y0, py);
    y1 = i == 0 ? py : fmax(y1, py);
  }
  rboxes_h[k * 4 + 0] = (float)x0;
  rboxes_h[k * 4 + 1] = (float)y0;
  rboxes_h[k * 4 + 2] = (float)x1;
  rboxes_h[k * 4 + 3] = (float)y1;
}

// ------------------------------------------------------------------------------------------------------------ targets
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (ceil(A / TPB), N).  block_pos[n * gridDim.x + blockIdx.x] = positives of this workgroup.
__global__ __launch_bounds__(TPB) void retina_targets_kernel(
    const float* __restrict__ anchors, int A, const float* __restrict__ rboxes, const float* __restrict__ rboxes_h,
    const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ gt_offsets, int total_gts, float pos_thr,
    float neg_hi, float neg_lo, int32_t* __restrict__ labels, float* __restrict__ label_weights,
    float* __restrict__ loc_targets, float* __restrict__ loc_weights, int32_t* __restrict__ raw_labels,
    int32_t* __restrict__ block_pos) {
  __shared__ float4 s_gt[JDET_RETINA_GT_CHUNK];
  __shared__ int s_cnt[TPB / 64];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int a = blockIdx.x * TPB + tid;
  const bool live = a < A;
  const int g0 = clampi(gt_offsets[n], 0, total_gts), g1 = clampi(gt_offsets[n + 1], g0, total_gts);
  float4 an = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) an = reinterpret_cast<const float4*>(anchors)[a];
  const float area_a = (an.z - an.x) * (an.w - an.y);
  float best = -INFINITY;
  int best_g = -1;
  for (int base = g0; base < g1; base += JDET_RETINA_GT_CHUNK) {
    const int cnt = min(JDET_RETINA_GT_CHUNK, g1 - base);
    __syncthreads();
    for (int k = tid; k < cnt; k += TPB) {
      const float* b = rboxes_h + (long)(base + k) * 4;
      s_gt[k] = make_float4(b[0], b[1], b[2], b[3]);
    }
    __syncthreads();
    if (live) {
      for (int k = 0; k < cnt; k++) {
        const float4 b = s_gt[k];
        const float tlx = fmaxf(an.x, b.x), tly = fmaxf(an.y, b.y);
        const float brx = fminf(an.z, b.z), bry = fminf(an.w, b.w);
        const float inside = (tlx < brx && tly < bry) ? 1.f : 0.f;
        const float area_i = ((brx - tlx) * (bry - tly)) * inside;
        const float area_b = (b.z - b.x) * (b.w - b.y);
        const float iou = area_i / ((area_a + area_b) - area_i);
        if (iou > best) {          // strict: a tie stays with the first gt
          best = iou;
          best_g = base + k;
        }
      }
    }
  }
  int lab = -1;
  bool iou_pos = false;
  if (g1 == g0) {
    lab = 0;                       // an image without gts: every anchor is a negative
  } else if (best_g >= 0) {
    if (best < neg_hi && best >= neg_lo) lab = 0;
    if (best >= pos_thr) {
      lab = gt_labels[best_g];
      iou_pos = true;
    }
  }
  float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (live && iou_pos) {
    const double x = ((double)an.x + (double)an.z) / 2, y = ((double)an.y + (double)an.w) / 2;
    const double w = (double)an.z - (double)an.x, h = (double)an.w - (double)an.y;
    const bool tall = h > w;
    const double sw = tall ? h : w, sh = tall ? w : h, sa = tall ? -PI_D : -PI_D / 2;
    const float* g = rboxes + (long)best_g * 5;
    t[0] = (float)(((double)g[0] - x) / (sw + 1));
    t[1] = (float)(((double)g[1] - y) / (sh + 1));
    t[2] = (float)log((double)g[2] / (sw + 1) + 1e-5);
    t[3] = (float)log((double)g[3] / (sh + 1) + 1e-5);
    t[4] = (float)((double)g[4] - sa);
  }
  const bool positive = live && lab > 0;
  if (live) {
    const long r = (long)n * A + a;
    raw_labels[r] = lab;
    labels[r] = lab < 0 ? 0 : lab;
    label_weights[r] = lab >= 0 ? 1.f : 0.f;
    const float lw = positive ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < 5; c++) {
      loc_targets[r * 5 + c] = t[c];
      loc_weights[r * 5 + c] = lw;
    }
  }
  const unsigned long long m = __ballot(positive);
  if ((tid & 63) == 0) s_cnt[wave_of(tid)] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < TPB / 64; w++) s += s_cnt[w];
    block_pos[(long)n * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void retina_normalizer_kernel(const int32_t* __restrict__ block_pos, int N, int nb,
                                                              float* __restrict__ normalizer) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  long s = 0;
  for (int b = 0; b < nb; b++) s += block_pos[(long)n * nb + b];
  normalizer[n] = (float)(s > 1 ? s : 1);
}

// ------------------------------------------------------------------------------------------------------------- detect
__device__ __forceinline__ float score_of(float logit) { return (float)(1.0 / (1.0 + exp(-(double)logit))); }

struct Proposal {
  double x, y, w, h, a;
};

__device__ __forceinline__ Proposal proposal_of(float4 an) {
  Proposal p;
  p.x = ((double)an.x + (double)an.z) / 2;
  p.y = ((double)an.y + (double)an.w) / 2;
  const double w = (double)an.z - (double)an.x, h = (double)an.w - (double)an.y;
  const bool tall = h > w;
  p.w = tall ? h : w;
  p.h = tall ? w : h;
  p.a = tall ? -PI_D / 2 : 0.0;
  return p;
}

__device__ __forceinline__ float decoded_angle(const Proposal& p, const float* l) { return (float)((double)l[4] + p.a); }

__device__ __forceinline__ bool angle_ok(float a) {
  const float half_pi = (float)(PI_D / 2);
  return a < half_pi && a > -half_pi;
}

// partial[c * nb + b] = selected anchors of class c in workgroup b
__global__ __launch_bounds__(TPB) void retina_detect_count_kernel(const float* __restrict__ anchors,
                                                                 const float* __restrict__ loc,
                                                                 const float* __restrict__ logits, int A, int C,
                                                                 float thr, int32_t* __restrict__ partial) {
  __shared__ int s_cnt[TPB / 64];
  const int tid = threadIdx.x, a = blockIdx.x * TPB + tid, nb = gridDim.x;
  bool ok = false;
  if (a < A) ok = angle_ok(decoded_angle(proposal_of(reinterpret_cast<const float4*>(anchors)[a]), loc + (long)a * 5));
  for (int c = 0; c < C; c++) {
    const bool sel = ok && score_of(logits[(long)a * C + c]) > thr;
    const unsigned long long m = __ballot(sel);
    if ((tid & 63) == 0) s_cnt[wave_of(tid)] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < TPB / 64; w++) s += s_cnt[w];
      partial[(long)c * nb + blockIdx.x] = s;
    }
    __syncthreads();
  }
}

// one workgroup: prefix[i] = sum of partial[0 .. i) for i = 0 .. T (T = C * nb), counts[c] = prefix[(c+1) nb] - prefix[c nb]
__global__ __launch_bounds__(TPB) void retina_detect_scan_kernel(const int32_t* __restrict__ partial, int C, int nb,
                                                                int32_t* __restrict__ prefix,
                                                                int32_t* __restrict__ counts) {
  __shared__ int s_sum[TPB];
  const int tid = threadIdx.x;
  const long T = (long)C * nb;
  const long per = (T + TPB - 1) / TPB;
  const long lo = min(T, tid * per), hi = min(T, lo + per);
  int s = 0;
  for (long i = lo; i < hi; i++) s += partial[i];
  s_sum[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < TPB; i++) {
      const int v = s_sum[i];
      s_sum[i] = run;
      run += v;
    }
    prefix[T] = run;
  }
  __syncthreads();
  int run = s_sum[tid];
  for (long i = lo; i < hi; i++) {
    prefix[i] = run;
    run += partial[i];
  }
  __threadfence_block();
  __syncthreads();
  for (int c = tid; c < C; c += TPB) counts[c] = prefix[(long)(c + 1) * nb] - prefix[(long)c * nb];
}

__global__ __launch_bounds__(TPB) void retina_detect_fill_kernel(const float* __restrict__ anchors,
                                                                const float* __restrict__ loc,
                                                                const float* __restrict__ logits, int A, int C,
                                                                float thr, float scale_x, float scale_y,
                                                                const int32_t* __restrict__ prefix, int M,
                                                                float* __restrict__ boxes, float* __restrict__ scores,
                                                                int32_t* __restrict__ labels) {
  __shared__ int s_cnt[TPB / 64];
  const int tid = threadIdx.x, a = blockIdx.x * TPB + tid, nb = gridDim.x;
  bool ok = false;
  float box[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (a < A) {
    const Proposal p = proposal_of(reinterpret_cast<const float4*>(anchors)[a]);
    const float* l = loc + (long)a * 5;
    box[4] = decoded_angle(p, l);
    ok = angle_ok(box[4]);
    if (ok) {
      const double cx = (double)l[0] * p.w + p.x, cy = (double)l[1] * p.h + p.y;
      const double w = exp((double)l[2]) * p.w, h = exp((double)l[3]) * p.h;
      const double x1 = cx - 0.5 * w, y1 = cy - 0.5 * h, x2 = cx + 0.5 * w, y2 = cy + 0.5 * h;
      box[0] = (float)((x1 + x2) / 2) * scale_x;
      box[1] = (float)((y1 + y2) / 2) * scale_y;
      box[2] = (float)(x2 - x1) * scale_x;
      box[3] = (float)(y2 - y1) * scale_y;
    }
  }
  for (int c = 0; c < C; c++) {
    float sc = 0.f;
    bool sel = false;
    if (ok) {
      sc = score_of(logits[(long)a * C + c]);
      sel = sc > thr;
    }
    const unsigned long long m = __ballot(sel);
    if ((tid & 63) == 0) s_cnt[wave_of(tid)] = __popcll(m);
    __syncthreads();
    if (sel) {
      long pos = (long)prefix[(long)c * nb + blockIdx.x] + lanes_below(m);
      for (int w = 0; w < wave_of(tid); w++) pos += s_cnt[w];
      if (pos >= 0 && pos < M) {
#pragma unroll
        for (int k = 0; k < 5; k++) boxes[pos * 5 + k] = box[k];
        scores[pos] = sc;
        labels[pos] = c;
      }
    }
    __syncthreads();
  }
}

inline int blocks_of(long n) { return (int)((n + TPB - 1) / TPB); }

}  // namespace

JDET_API int jdet_retina_gt_prepare(const float* gts, int K, float* rboxes, float* rboxes_h, jdet_stream_t stream) {
  if (K < 0) return JDET_E_BADARG;
  if (K == 0) return JDET_OK;
  if (!gts || !rboxes || !rboxes_h) return JDET_E_BADARG;
  hipLaunchKernelGGL(retina_gt_prepare_kernel, dim3(blocks_of(K)), dim3(TPB), 0, (hipStream_t)stream, gts, K, rboxes,
                     rboxes_h);
  return jdet_launch_status();
}

JDET_API size_t jdet_retina_targets_workspace(int N, int A) {
  if (N <= 0 || A <= 0) return 0;
  return (size_t)N * (size_t)blocks_of(A) * sizeof(int32_t);
}

JDET_API int jdet_retina_targets(const float* anchors, int A, const float* rboxes, const float* rboxes_h,
                                 const int32_t* gt_labels, const int32_t* gt_offsets, int N, int total_gts,
                                 float pos_iou_thresh, float neg_iou_thresh_hi, float neg_iou_thresh_lo,
                                 int32_t* labels, float* label_weights, float* loc_targets, float* loc_weights,
                                 int32_t* raw_labels, float* normalizer, void* workspace, size_t workspace_bytes,
                                 jdet_stream_t stream) {
  if (N < 0 || A < 0 || total_gts < 0) return JDET_E_BADARG;
  if (N == 0) return JDET_OK;
  if (!normalizer || !gt_offsets) return JDET_E_BADARG;
  if (N > 65535) return JDET_E_UNSUPPORTED;           // the image index is the grid's y
  if (A > 0 && (!anchors || !labels || !label_weights || !loc_targets || !loc_weights || !raw_labels))
    return JDET_E_BADARG;
  if (total_gts > 0 && (!rboxes || !rboxes_h || !gt_labels)) return JDET_E_BADARG;
  if (((uintptr_t)anchors & 15) != 0) return JDET_E_BADARG;
  if (workspace_bytes < jdet_retina_targets_workspace(N, A)) return JDET_E_WORKSPACE;
  if (A > 0 && !workspace) return JDET_E_BADARG;
  const int nb = A > 0 ? blocks_of(A) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL(retina_targets_kernel, dim3(nb, N), dim3(TPB), 0, (hipStream_t)stream, anchors, A, rboxes,
                       rboxes_h, gt_labels, gt_offsets, total_gts, pos_iou_thresh, neg_iou_thresh_hi,
                       neg_iou_thresh_lo, labels, label_weights, loc_targets, loc_weights, raw_labels,
                       (int32_t*)workspace);
    const int e = jdet_launch_status();
    if (e) return e;
  }
  hipLaunchKernelGGL(retina_normalizer_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     (const int32_t*)workspace, N, nb, normalizer);
  return jdet_launch_status();
}

JDET_API size_t jdet_retina_detect_workspace(int A, int C) {
  if (A < 0 || C <= 0) return 0;
  return (2 * (size_t)C * (size_t)blocks_of(A) + 1) * sizeof(int32_t);
}

JDET_API int jdet_retina_detect_count(const float* anchors, const float* loc, const float* logits, int A, int C,
                                      float score_thresh, int32_t* counts, void* workspace, size_t workspace_bytes,
                                      jdet_stream_t stream) {
  if (A < 0 || C <= 0 || !counts) return JDET_E_BADARG;
  if (A > 0 && (!anchors || !loc || !logits)) return JDET_E_BADARG;
  if (((uintptr_t)anchors & 15) != 0) return JDET_E_BADARG;
  if ((long)C * blocks_of(A) >= (1L << 30)) return JDET_E_UNSUPPORTED;
  if (workspace_bytes < jdet_retina_detect_workspace(A, C)) return JDET_E_WORKSPACE;
  if (!workspace) return JDET_E_BADARG;
  const int nb = blocks_of(A);
  int32_t* partial = (int32_t*)workspace;
  int32_t* prefix = partial + (size_t)C * nb;
  if (nb > 0) {
    hipLaunchKernelGGL(retina_detect_count_kernel, dim3(nb), dim3(TPB), 0, (hipStream_t)stream, anchors, loc, logits, A,
                       C, score_thresh, partial);
    const int e = jdet_launch_status();
    if (e) return e;
  }
  hipLaunchKernelGGL(retina_detect_scan_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const int32_t*)partial, C,
                     nb, prefix, counts);
  return jdet_launch_status();
}

JDET_API int jdet_retina_detect_fill(const float* anchors, const float* loc, const float* logits, int A, int C,
                                     float score_thresh, float scale_x, float scale_y, const void* workspace,
                                     size_t workspace_bytes, int M, float* boxes, float* scores, int32_t* labels,
                                     jdet_stream_t stream) {
  if (A < 0 || C <= 0 || M < 0) return JDET_E_BADARG;
  if (A > 0 && (!anchors || !loc || !logits)) return JDET_E_BADARG;
  if (M > 0 && (!boxes || !scores || !labels)) return JDET_E_BADARG;
  if (((uintptr_t)anchors & 15) != 0) return JDET_E_BADARG;
  if ((long)C * blocks_of(A) >= (1L << 30)) return JDET_E_UNSUPPORTED;
  if (workspace_bytes < jdet_retina_detect_workspace(A, C)) return JDET_E_WORKSPACE;
  if (!workspace) return JDET_E_BADARG;
  if (A == 0 || M == 0) return JDET_OK;
  const int nb = blocks_of(A);
  const int32_t* prefix = (const int32_t*)workspace + (size_t)C * nb;
  hipLaunchKernelGGL(retina_detect_fill_kernel, dim3(nb), dim3(TPB), 0, (hipStream_t)stream, anchors, loc, logits, A, C,
                     score_thresh, scale_x, scale_y, prefix, M, boxes, scores, labels);
  return jdet_launch_status();
}
