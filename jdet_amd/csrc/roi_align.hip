// RoIAlign family for gfx950 (MI355X): the exported entry points of the forward (kernels and launcher:
// roi_align_fwd.h; backward: roi_align_bwd.hip), the XCD-aware RoI schedule and the NCHW <-> NHWC transposes.  Two
// arithmetics, each behind its OWN entry points -- the library holds no process-wide mode and reads no environment:
//   jdet_roi_align_forward / _cl_roi / _cl            merged taps (the product path)
//   jdet_roi_align_forward_reference / _cl_reference  the reference's operation order (bit-identical to the CPU
//                                                     oracle: the parity twin of the tests and of smoke())
// The measured alternatives (channel-sliced, line-deduplicated, pair-merged and footprint-staged kernels) and the
// profiling builds of the product kernels compile into libjdet_experimental.so (its RoIAlign translation unit includes
// roi_align_fwd.h); nothing of them is in this library.
#include "roi_align_fwd.h"

namespace {

// ---------------------------------------------------------------------------------------------
// XCD-aware spatial schedule.
// The feature map (67 MB at 256x256x256 fp32) does not fit a 4 MiB XCD L2, and workgroup b runs
// on XCD b % 8: with RoIs in arbitrary order every XCD streams the whole map through the fabric
// (measured: FETCH 451 MB per launch for 67 MB of map, L2 hit 37 %).  This kernel buckets RoIs by
// the Morton code of their centre cell (counting sort, one workgroup, O(R)), then deals
// contiguous runs of the sorted list to the 8 XCDs: order[b] = sorted[start(b % 8) + b / 8].
// Each XCD then sweeps one compact region of the map and concurrently resident workgroups are
// spatial neighbours (measured: FETCH 139 MB, L2 hit 73 %).
// ---------------------------------------------------------------------------------------------
constexpr int kOrderThreads = 1024;
constexpr int kOrderCellsLog2 = 5;                   // 32 x 32 cells per image
constexpr int kOrderCells = 1 << (2 * kOrderCellsLog2);
constexpr int kOrderMaxImages = 8;                   // bins in LDS: 8 * 1024 * 4 B = 32 KiB

__device__ __forceinline__ unsigned morton2(unsigned x, unsigned y) {
  auto spread = [](unsigned v) {
    v &= 0xffff;
    v = (v | (v << 8)) & 0x00ff00ff;
    v = (v | (v << 4)) & 0x0f0f0f0f;
    v = (v | (v << 2)) & 0x33333333;
    v = (v | (v << 1)) & 0x55555555;
    return v;
  };
  return spread(x) | (spread(y) << 1);
}

__global__ __launch_bounds__(kOrderThreads) void roi_order_kernel(const float* __restrict__ rois, int R,
                                                                 int roi_cols, float spatial_scale, int N,
                                                                 int H, int W, int32_t* __restrict__ order,
                                                                 int32_t* __restrict__ sorted_tmp) {
  constexpr int kKeep = 8;                      // RoIs per thread whose key stays in registers
  constexpr int kLdsSorted = kKeep * kOrderThreads;  // R <= 8192: sorted list lives in LDS
  __shared__ int s_bins[kOrderMaxImages * kOrderCells];
  __shared__ int s_scan[kOrderThreads / 64];
  __shared__ int s_sorted[kLdsSorted];
  const int nimg = min(N, kOrderMaxImages);
  const int nbins = nimg * kOrderCells;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nbins; i += kOrderThreads) s_bins[i] = 0;
  __syncthreads();
  auto key_of = [&](int r) -> int {
    const float* p = rois + (size_t)r * roi_cols;
    float cx, cy;
    if (roi_cols == 5) {
      cx = 0.5f * (p[1] + p[3]) * spatial_scale;
      cy = 0.5f * (p[2] + p[4]) * spatial_scale;
    } else {
      cx = p[1] * spatial_scale;
      cy = p[2] * spatial_scale;
    }
    int b = (int)p[0];
    b = min(max(b, 0), nimg - 1);
    const float fx = fminf(fmaxf(cx / (float)W, 0.f), 0.999999f);
    const float fy = fminf(fmaxf(cy / (float)H, 0.f), 0.999999f);
    const unsigned ix = (unsigned)(fx * (1 << kOrderCellsLog2));
    const unsigned iy = (unsigned)(fy * (1 << kOrderCellsLog2));
    return b * kOrderCells + (int)morton2(ix, iy);
  };
  int mykey[kKeep];
#pragma unroll
  for (int i = 0; i < kKeep; i++) {
    const int r = threadIdx.x + i * kOrderThreads;
    mykey[i] = r < R ? key_of(r) : 0;
    if (r < R) atomicAdd(&s_bins[mykey[i]], 1);
  }
  for (int r = threadIdx.x + kKeep * kOrderThreads; r < R; r += kOrderThreads) atomicAdd(&s_bins[key_of(r)], 1);
  __syncthreads();
  // exclusive scan of the bins: contiguous slice per thread, wave scan by DPP-style shuffles,
  // one LDS hop across the 16 waves
  const int per = (nbins + kOrderThreads - 1) / kOrderThreads;
  const int lo = threadIdx.x * per, hi = min(lo + per, nbins);
  int sum = 0;
  for (int i = lo; i < hi; i++) sum += s_bins[i];
  int incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) s_scan[wave] = incl;
  __syncthreads();
  int wave_base = 0;
  for (int w = 0; w < wave; w++) wave_base += s_scan[w];
  int run = wave_base + incl - sum;
  for (int i = lo; i < hi; i++) {
    const int c = s_bins[i];
    s_bins[i] = run;
    run += c;
  }
  __syncthreads();
  const bool in_lds = R <= kLdsSorted;
#pragma unroll
  for (int i = 0; i < kKeep; i++) {
    const int r = threadIdx.x + i * kOrderThreads;
    if (r < R) {
      const int pos = atomicAdd(&s_bins[mykey[i]], 1);
      if (in_lds) s_sorted[pos] = r; else sorted_tmp[pos] = r;
    }
  }
  for (int r = threadIdx.x + kKeep * kOrderThreads; r < R; r += kOrderThreads)
    sorted_tmp[atomicAdd(&s_bins[key_of(r)], 1)] = r;
  if (!in_lds) __threadfence();  // global scratch is re-read by other waves: agent-scope release
  __syncthreads();
  // deal contiguous runs to the 8 XCDs (workgroup b -> XCD b % 8 is the observed dispatch rule;
  // a different placement only costs speed): start(x) = sum_{y<x} ceil((R - y) / 8)
  for (int b = threadIdx.x; b < R; b += kOrderThreads) {
    const int x = b & 7, p = b >> 3;
    int start = 0;
#pragma unroll
    for (int y = 0; y < 7; y++) start += y < x ? ((R - y + 7) >> 3) : 0;
    order[b] = in_lds ? s_sorted[start + p]
                      : __hip_atomic_load(sorted_tmp + start + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// (Round 6, measured and removed: the same schedule from a multi-workgroup launch -- every workgroup computes all keys into
// LDS and ranks its own 16 / 32 RoIs by counting, 8 / 16 lanes per RoI over (key << 13 | index) words, no inter-workgroup
// exchange.  5.8 us with 63 workgroups, 7.2 us with 125 (rocprofv3) against 5.0 us for the counting sort above: the
// R key computations every workgroup repeats cost what the serial chain costs.  profiles/r06_roi_plan_notes.md.)

// ---------------------------------------------------------------------------------------------
// NCHW <-> NHWC tiled transposes: per image a (C, HW) <-> (HW, C) matrix transpose.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ x,
                                                        float* __restrict__ y, int rows, int cols) {
  // x: (batch, rows, cols) -> y: (batch, cols, rows); 32x32 tiles, +1 pad (conflict-free)
  __shared__ float tile[32][33];
  const size_t base = (size_t)blockIdx.z * rows * cols;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int rr = r0 + ty + i, ccol = c0 + tx;
    if (rr < rows && ccol < cols) tile[ty + i][tx] = x[base + (size_t)rr * cols + ccol];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int ccol = c0 + ty + i, rr = r0 + tx;
    if (rr < rows && ccol < cols) y[base + (size_t)ccol * rows + rr] = tile[tx][ty + i];
  }
}

int launch_transpose(const float* x, float* y, int batch, int rows, int cols, hipStream_t st) {
  if (batch == 0 || rows == 0 || cols == 0) return JDET_OK;
  dim3 grid(jdet_cdiv(cols, 32), jdet_cdiv(rows, 32), batch);
  if (grid.y > 65535 || grid.z > 65535) return JDET_E_UNSUPPORTED;
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, st, x, y, rows, cols);
  return jdet_launch_status();
}

int forward_any(int mode, int variant, const float* feat, int N, int C, int H, int W, const float* rois, int R, int PH,
                int PW, float spatial_scale, int sample_num, int n_orient, const int32_t* order, float* out,
                bool out_cl, jdet_stream_t stream) {
  int e = check_common(variant, feat, rois, out, N, C, H, W, R, PH, PW, n_orient);
  if (e) return e;
  if (out_cl) {
    if (C % 4 != 0 || (size_t)H * W * C * 4 >= (1ull << 31)) return JDET_E_UNSUPPORTED;
    if (variant == JDET_ROI_RIROI && n_orient != 4 && n_orient != 8) return JDET_E_UNSUPPORTED;
  }
  if (R == 0) return JDET_OK;
  hipStream_t st = (hipStream_t)stream;
  return with_variant(variant, [&](auto v) {
    constexpr int V = decltype(v)::value;
    return launch_fwd<V>(feat, rois, out, R, C, H, W, PH, PW, spatial_scale, sample_num,
                         V == JDET_ROI_RIROI ? n_orient : 1, order, st, out_cl, mode);
  });
}

// channels-last result under the XCD-aware spatial order; the schedule lives in the caller's workspace
int forward_cl_any(int mode, int variant, const float* feat, int N, int C, int H, int W, const float* rois, int R,
                   int PH, int PW, float spatial_scale, int sample_num, int n_orient, float* out_cl, void* workspace,
                   size_t workspace_bytes, jdet_stream_t stream) {
  int e = check_common(variant, feat, rois, out_cl, N, C, H, W, R, PH, PW, n_orient);
  if (e) return e;
  if (C % 4 != 0 || (size_t)H * W * C * 4 >= (1ull << 31)) return JDET_E_UNSUPPORTED;
  if (variant == JDET_ROI_RIROI && n_orient != 4 && n_orient != 8) return JDET_E_UNSUPPORTED;
  if (R == 0) return JDET_OK;
  if (!workspace || workspace_bytes < jdet_roi_align_forward_cl_workspace(R, PH, PW)) return JDET_E_WORKSPACE;
  const int32_t* order = nullptr;
  if (R >= 64) {   // below that the map traffic is too small for the schedule to matter
    int32_t* o = (int32_t*)workspace;
    const int cols = (variant == JDET_ROI_HBB_V0 || variant == JDET_ROI_HBB_V1) ? 5 : 6;
    e = jdet_roi_spatial_order(rois, R, cols, spatial_scale, N, H, W, o, o + R, stream);
    if (e) return e;
    order = o;
  }
  return forward_any(mode, variant, feat, N, C, H, W, rois, R, PH, PW, spatial_scale, sample_num, n_orient, order,
                     out_cl, true, stream);
}

}  // namespace

JDET_API int jdet_nchw_to_nhwc(const float* x, int N, int C, int H, int W, float* y,
                               jdet_stream_t stream) {
  if (N < 0 || C < 0 || H < 0 || W < 0 || ((long)N * C * H * W > 0 && (!x || !y))) return JDET_E_BADARG;
  return launch_transpose(x, y, N, C, H * W, (hipStream_t)stream);
}

JDET_API int jdet_nhwc_to_nchw(const float* x, int N, int C, int H, int W, float* y,
                               jdet_stream_t stream) {
  if (N < 0 || C < 0 || H < 0 || W < 0 || ((long)N * C * H * W > 0 && (!x || !y))) return JDET_E_BADARG;
  return launch_transpose(x, y, N, H * W, C, (hipStream_t)stream);
}

JDET_API int jdet_roi_spatial_order(const float* rois, int R, int roi_cols, float spatial_scale, int N,
                                    int H, int W, int32_t* order, int32_t* workspace,
                                    jdet_stream_t stream) {
  if (R < 0 || (roi_cols != 5 && roi_cols != 6) || N <= 0 || H <= 0 || W <= 0) return JDET_E_BADARG;
  if (R == 0) return JDET_OK;
  if (!rois || !order || !workspace) return JDET_E_BADARG;
  hipLaunchKernelGGL(roi_order_kernel, dim3(1), dim3(kOrderThreads), 0, (hipStream_t)stream, rois, R,
                     roi_cols, spatial_scale, N, H, W, order, workspace);
  return jdet_launch_status();
}

JDET_API int jdet_roi_align_forward(int variant, const float* feat, int N, int C, int H, int W,
                                    const float* rois, int R, int PH, int PW, float spatial_scale,
                                    int sample_num, int n_orient, const int32_t* order, float* out,
                                    jdet_stream_t stream) {
  return forward_any(kFwdMerged, variant, feat, N, C, H, W, rois, R, PH, PW, spatial_scale, sample_num, n_orient, order,
                     out, false, stream);
}

// the same call in the reference's operation order (per-lane accumulation exactly as the reference kernel's:
// bit-identical to the CPU oracle)
JDET_API int jdet_roi_align_forward_reference(int variant, const float* feat, int N, int C, int H, int W,
                                              const float* rois, int R, int PH, int PW, float spatial_scale,
                                              int sample_num, int n_orient, const int32_t* order, float* out,
                                              jdet_stream_t stream) {
  return forward_any(kFwdReference, variant, feat, N, C, H, W, rois, R, PH, PW, spatial_scale, sample_num, n_orient,
                     order, out, false, stream);
}

// RoI-stationary forward with a channels-last result (R, PH, PW, C): same kernels, results stored straight from
// registers (one contiguous 1 KiB row chunk per wave and bin) instead of being transposed through LDS.
JDET_API int jdet_roi_align_forward_cl_roi(int variant, const float* feat, int N, int C, int H, int W,
                                           const float* rois, int R, int PH, int PW, float spatial_scale,
                                           int sample_num, int n_orient, const int32_t* order, float* out_cl,
                                           jdet_stream_t stream) {
  return forward_any(kFwdMerged, variant, feat, N, C, H, W, rois, R, PH, PW, spatial_scale, sample_num, n_orient, order,
                     out_cl, true, stream);
}

// Product forward with a channels-last result: the RoI-stationary kernels under the XCD-aware spatial order.
JDET_API size_t jdet_roi_align_forward_cl_workspace(int R, int PH, int PW) {
  if (R <= 0 || PH <= 0 || PW <= 0) return 256;
  return 256 + 2 * sizeof(int32_t) * (size_t)R;      // the two int32 arrays of the spatial order
}

JDET_API int jdet_roi_align_forward_cl(int variant, const float* feat, int N, int C, int H, int W, const float* rois,
                                       int R, int PH, int PW, float spatial_scale, int sample_num, int n_orient,
                                       float* out_cl, void* workspace, size_t workspace_bytes, jdet_stream_t stream) {
  return forward_cl_any(kFwdMerged, variant, feat, N, C, H, W, rois, R, PH, PW, spatial_scale, sample_num, n_orient,
                        out_cl, workspace, workspace_bytes, stream);
}

JDET_API int jdet_roi_align_forward_cl_reference(int variant, const float* feat, int N, int C, int H, int W,
                                                 const float* rois, int R, int PH, int PW, float spatial_scale,
                                                 int sample_num, int n_orient, float* out_cl, void* workspace,
                                                 size_t workspace_bytes, jdet_stream_t stream) {
  return forward_cl_any(kFwdReference, variant, feat, N, C, H, W, rois, R, PH, PW, spatial_scale, sample_num, n_orient,
                        out_cl, workspace, workspace_bytes, stream);
}
