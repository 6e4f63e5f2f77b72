// The measurement side of the RoIAlign forward, outside the product ABI: the product's forward header (../roi_align_fwd.h:
// kernels and launcher) plus everything that exists to be measured against it, behind jdet_roi_align_forward_cl_mode --
//   mode 0: the product arithmetic launched from THIS translation unit, with the profiling builds of the merged kernel
//           selectable from the environment (JDET_ROI_FWD_GRAN, JDET_ROI_FWD_LDS_KB: launch_mode below)
//   mode 2: merged taps through the channel-sliced kernels (roi_align_sliced.h): XCD x owns channels [32 x, 32 x + 32) of
//           every RoI; reads beyond the L2 1.34 M -> 0.55 M requests, 63.7-80 us against 58 us (profiles/r04_roi_fwd_notes.md)
//   mode 3: taps deduplicated over a line of bins (roi_align_line.h): rows through the L1 -45 %, 71 us against 58 us
//   mode 4: the footprint-staged kernel (roi_align_stage.h, round 6): distinct pixels of a line by LDS-DMA, a measured no-go
//   mode 5: taps merged over PAIRS of neighbouring bins, two accumulators (roi_align_pair.h, round 6): rows -22 %, L1 accesses
//           -20 %, VALU +46 %: 59.4 us against 56.4 us for the rolling-window product kernel (profiles/r06_roi_fwd_ring.md)
//   mode 6: the per-bin tap loop of rounds 1-5, which the rolling window replaced and must equal bit for bit
//           (tests/test_gpu_roi_align_ring.py)
// Kept with their parity tests as the measured answers to "partition the XCDs by channel", "deduplicate the pixel rows of
// neighbouring bins" and "stage a line's footprint in LDS"; none is a product path.  Where a mode does not apply to a
// shape, the product launcher runs.
#include <stdlib.h>

#include "roi_align_fwd.h"

namespace {
#include "roi_align_sliced.h"   // namespace jdet_roi_sliced, uses ri_mix<>
#include "roi_align_line.h"
#include "roi_align_pair.h"
}  // namespace
// (outside the anonymous namespace: the launcher takes the kernel's address for hipFuncSetAttribute, and hipcc does not
//  emit the host-side handle of an internal-linkage kernel template whose address is taken)
#include "roi_align_stage.h"

#include "jdet_experimental.h"

namespace {

constexpr int kFwdProduct = 0, kFwdSliced = 2, kFwdLine = 3, kFwdStaged = 4, kFwdPair = 5, kFwdPerBin = 6;

// Tuning knobs of the measured kernels (A/B-able from the environment for profiling runs).
int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// ---- footprint-staged forward (roi_align_stage.h): channels-last result, 2x2 samples per bin, PH, PW <= 8 ----
template <int VARIANT, int CPP, int P7>
int launch_staged(const float* feat, const float* rois, float* out, int R, int C, int H, int W, int PH, int PW,
                  float scale, const int32_t* order, hipStream_t st) {
  using namespace jdet_roi_stage;
  auto kern = roi_align_fwd_staged_kernel<VARIANT, CPP, P7>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       Layout<CPP>::kTotal);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  static const int abl = env_int("JDET_ROI_STAGE_ABL", 0);   // profiling: 1 prologue only, 2 no DMA, 4 no compute, 8 no stores
  hipLaunchKernelGGL(kern, dim3(R), dim3(kThreads), Layout<CPP>::kTotal, st, feat, rois, out, C, H, W, PH, PW, scale,
                     order, abl);
  return jdet_launch_status();
}

inline bool staged_ok(int C, int PH, int PW, int sample_num, int cpp) {
  return sample_num == 2 && PH <= 8 && PW <= 8 && C % cpp == 0;
}

// The RoI-stationary launches (`order`: a schedule of jdet_roi_spatial_order, or NULL).  The caller has checked what the
// vector kernels need: C % 4 == 0, a map under 2 GiB per image, RiRoIAlign with 4 or 8 orientation planes.
template <int VARIANT>
int launch_mode(int mode, const float* feat, const float* rois, float* out, int R, int C, int H, int W, int PH, int PW,
                float scale, int sample_num, int nO, const int32_t* order, hipStream_t st) {
  const dim3 grid(R, jdet_cdiv(C, kChunkC)), block(256);
  const int nbins = PH * PW;
  const bool merged = sample_num == 2 && nbins <= 64;   // where the product launches its merged-tap kernel
  auto product = [&] {
    return launch_fwd<VARIANT>(feat, rois, out, R, C, H, W, PH, PW, scale, sample_num, nO, order, st, true, kFwdMerged);
  };
  if constexpr (VARIANT == JDET_ROI_RIROI) {
    auto ri = [&](auto no) {
      constexpr int NO = decltype(no)::value;
      if (mode == kFwdPair && pair_ok(PH, PW))
        hipLaunchKernelGGL((roi_align_fwd_pair_kernel<JDET_ROI_ROTATED, NO>), grid, block, (size_t)36 * 1024, st, feat,
                           rois, out, C, H, W, PH, PW, scale, order);
      else if (mode == kFwdPerBin)
        hipLaunchKernelGGL((roi_align_fwd_merged_kernel<JDET_ROI_ROTATED, 4, 0, true, NO>), grid, block, kFwdListLds, st,
                           feat, rois, out, C, H, W, PH, PW, scale, order);
      else
        return product();
      return jdet_launch_status();
    };
    if (!merged) return product();
    return nO == 8 ? ri(std::integral_constant<int, 8>{}) : ri(std::integral_constant<int, 4>{});
  } else {
    if (mode == kFwdStaged && staged_ok(C, PH, PW, sample_num, 64)) {
      static const int cpp = env_int("JDET_ROI_STAGE_CPP", 64);
      const bool p7 = PH == 7 && PW == 7;
      if (cpp == 32)
        return p7 ? launch_staged<VARIANT, 32, 1>(feat, rois, out, R, C, H, W, PH, PW, scale, order, st)
                  : launch_staged<VARIANT, 32, 0>(feat, rois, out, R, C, H, W, PH, PW, scale, order, st);
      return p7 ? launch_staged<VARIANT, 64, 1>(feat, rois, out, R, C, H, W, PH, PW, scale, order, st)
                : launch_staged<VARIANT, 64, 0>(feat, rois, out, R, C, H, W, PH, PW, scale, order, st);
    }
    if (!merged) return product();
    // JDET_ROI_FWD_LDS_KB: the LDS request of the merged launches (workgroups per CU; the product asks for kFwdClLds)
    static const int lds_kb = env_int("JDET_ROI_FWD_LDS_KB", (int)(kFwdClLds / 1024));
    const size_t lds_cl = lds_kb > 16 ? (size_t)lds_kb * 1024 : kFwdListLds;
#define JDET_MERGED(ABL_)                                                                                             \
  hipLaunchKernelGGL((roi_align_fwd_merged_kernel<VARIANT, 4, ABL_, true>), grid, block, lds_cl, st, feat, rois, out, C, \
                     H, W, PH, PW, scale, order)
    if (mode == kFwdLine && PH <= kLineMaxBins && PW <= kLineMaxBins && nbins * 4 <= 256) {
      // 36 KiB of tables = 4 workgroups per CU as well
      static const int line_batch16 = env_int("JDET_ROI_FWD_LINE_BATCH16", 0);     // (A/B runs: 16 rows per batch)
      const size_t lds_ln = (size_t)kLineMaxBins * kLineSlots * (4 + 32);
      if (PH <= 7 && PW <= 7 && !line_batch16)
        hipLaunchKernelGGL((roi_align_fwd_line_kernel<VARIANT, 7, 8>), grid, block, lds_ln, st, feat, rois, out, C, H, W,
                           PH, PW, scale, order);
      else if (PH <= 7 && PW <= 7)
        hipLaunchKernelGGL((roi_align_fwd_line_kernel<VARIANT, 7, 16>), grid, block, lds_ln, st, feat, rois, out, C, H, W,
                           PH, PW, scale, order);
      else
        hipLaunchKernelGGL((roi_align_fwd_line_kernel<VARIANT, 8, 16>), grid, block, lds_ln, st, feat, rois, out, C, H, W,
                           PH, PW, scale, order);
    } else if (mode == kFwdPair && pair_ok(PH, PW)) {
      hipLaunchKernelGGL((roi_align_fwd_pair_kernel<VARIANT, 0>), grid, block, lds_cl, st, feat, rois, out, C, H, W, PH, PW,
                         scale, order);
    } else if (mode == kFwdPerBin) {
      JDET_MERGED(0);
    } else if (mode == kFwdProduct) {
      // JDET_ROI_FWD_GRAN (read once per process): 2 / 1 = the per-bin loop with that many rows per guarded group;
      // 128 = per-bin loop + workgroup time stamps into the output rows (scripts/r6_fwd_stamps.py); 384 = rolling window +
      // stamps; 768 = prologue only; anything else: the rolling window, as the product launches it
      static const int gran = env_int("JDET_ROI_FWD_GRAN", 256);
      if (gran == 2) JDET_MERGED(32);
      else if (gran == 1) JDET_MERGED(64);
      else if (gran == 128) JDET_MERGED(128);
      else if (gran == 384) JDET_MERGED(384);
      else if (gran == 768) JDET_MERGED(768);
      else JDET_MERGED(256);
    } else {
      return product();
    }
#undef JDET_MERGED
    return jdet_launch_status();
  }
}

// ---- channel-sliced forward (experimental/roi_align_sliced.h): measured slower than the RoI-stationary kernels
// (profiles/r04_roi_fwd_notes.md) ----
bool sliced_ok(int variant, int R, int N, int C, int H, int W, int PH, int PW, int sample_num, int nO) {
  if (sample_num != 2) return false;
  const long nbins = (long)PH * PW;
  if (nbins < jdet_roi_sliced::kItemsPerWave || C % jdet_roi_sliced::kSliceC != 0) return false;
  if ((size_t)N * H * W * C * 4 >= (1ull << 31) || (long)R * nbins >= (1L << 30)) return false;
  if (variant == JDET_ROI_RIROI && nO != 4 && nO != 8) return false;
  return true;
}

template <int VARIANT, int NO>
int launch_sliced(const float* feat, const float* rois, float* out, int R, int N, int C, int H, int W, int PH, int PW,
                  float scale, int nO, void* ws, hipStream_t st) {
  using namespace jdet_roi_sliced;
  const int nbins = PH * PW;
  const PlanWs w = plan_carve(ws, R, nbins);
  // EXPERIMENT (profiling): JDET_ROI_SLICED_PLANAR=1 reads `feat` as [slice][pixel][32 channels] (every slice one
  // contiguous plane) instead of NHWC -- the caller must pass a map permuted that way
  static const int planar = env_int("JDET_ROI_SLICED_PLANAR", 0);
  const int pix_bytes = planar ? kSliceC * 4 : C * 4;
  const unsigned slice_stride = planar ? (unsigned)((size_t)N * H * W * kSliceC * 4) : (unsigned)(kSliceC * 4);
  hipLaunchKernelGGL((roi_sort_plan_kernel<VARIANT>), dim3(1 + (R + 3) / 4), dim3(1024), 0, st, rois, R, scale, N,
                     pix_bytes, H, W, PH, PW, nO, w.hdr, w.order, w.rrec, w.ent);
  const int nslices = C / kSliceC;
  const long items = (long)R * nbins;
#define JDET_SL(B_, P_, NW_)                                                                                          \
  hipLaunchKernelGGL((roi_pool_sliced_kernel<NO, B_, P_, NW_>),                                                       \
                     dim3((unsigned)(nslices * ((items + NW_ * kItemsPerWave - 1) / (NW_ * kItemsPerWave)))),         \
                     dim3(NW_ * 64), 0, st, feat, w.order, w.rrec, w.ent, out, R, N, C, H * W, nbins, nslices, slice_stride)
  if constexpr (NO == 0) {   // tuning knobs (profiling runs)
    static const int batch = env_int("JDET_ROI_SLICED_BATCH", 8), pred = env_int("JDET_ROI_SLICED_PRED", 0),
                     nw = env_int("JDET_ROI_SLICED_WAVES", 4);
    if (nw == 16 && batch == 4 && pred == 1) JDET_SL(4, 1, 16);
    else if (nw == 16) JDET_SL(8, 0, 16);
    else if (nw == 8 && batch == 4 && pred == 1) JDET_SL(4, 1, 8);
    else if (nw == 1 && batch == 4 && pred == 1) JDET_SL(4, 1, 1);
    else if (batch == 4 && pred == 0) JDET_SL(4, 0, 4);
    else if (batch == 16 && pred == 0) JDET_SL(16, 0, 4);
    else if (batch == 4 && pred == 1) JDET_SL(4, 1, 4);
    else if (batch == 8 && pred == 1) JDET_SL(8, 1, 4);
    else JDET_SL(8, 0, 4);
  } else {
    JDET_SL(8, 0, 4);
  }
#undef JDET_SL
  return jdet_launch_status();
}

}  // namespace

JDET_API size_t jdet_roi_align_forward_cl_mode_workspace(int mode, int R, int PH, int PW) {
  if (R <= 0 || PH <= 0 || PW <= 0) return 256;
  if (mode == kFwdSliced) return jdet_roi_sliced::plan_carve(nullptr, R, (long)PH * PW).bytes;
  return 256 + 2 * sizeof(int32_t) * (size_t)R;
}

JDET_API int jdet_roi_align_forward_cl_mode(int mode, int variant, const float* feat, int N, int C, int H, int W,
                                            const float* rois, int R, int PH, int PW, float spatial_scale,
                                            int sample_num, int n_orient, const int32_t* order, float* out_cl,
                                            void* workspace, size_t workspace_bytes, jdet_stream_t stream) {
  if (mode != kFwdProduct && mode != kFwdSliced && mode != kFwdLine && mode != kFwdStaged && mode != kFwdPair &&
      mode != kFwdPerBin)
    return JDET_E_BADARG;
  int e = check_common(variant, feat, rois, out_cl, N, C, H, W, R, PH, PW, n_orient);
  if (e) return e;
  if (C % 4 != 0 || (size_t)H * W * C * 4 >= (1ull << 31)) return JDET_E_UNSUPPORTED;
  if (variant == JDET_ROI_RIROI && n_orient != 4 && n_orient != 8) return JDET_E_UNSUPPORTED;
  if (R == 0) return JDET_OK;
  hipStream_t st = (hipStream_t)stream;
  if (mode == kFwdSliced) {
    if (!sliced_ok(variant, R, N, C, H, W, PH, PW, sample_num, n_orient)) return JDET_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < jdet_roi_align_forward_cl_mode_workspace(mode, R, PH, PW)) return JDET_E_WORKSPACE;
    return with_variant(variant, [&](auto v) {
      constexpr int V = decltype(v)::value;
      if constexpr (V == JDET_ROI_RIROI) {   // rotated geometry, planes mixed per bin
        if (n_orient == 8)
          return launch_sliced<JDET_ROI_ROTATED, 8>(feat, rois, out_cl, R, N, C, H, W, PH, PW, spatial_scale, 8, workspace, st);
        return launch_sliced<JDET_ROI_ROTATED, 4>(feat, rois, out_cl, R, N, C, H, W, PH, PW, spatial_scale, 4, workspace, st);
      } else {
        return launch_sliced<V, 0>(feat, rois, out_cl, R, N, C, H, W, PH, PW, spatial_scale, 1, workspace, st);
      }
    });
  }
  return with_variant(variant, [&](auto v) {
    constexpr int V = decltype(v)::value;
    return launch_mode<V>(mode, feat, rois, out_cl, R, C, H, W, PH, PW, spatial_scale, sample_num,
                          V == JDET_ROI_RIROI ? n_orient : 1, order, st);
  });
}
