// RoIAlign family for gfx950 (MI355X): ROIAlignRotated, ROIAlignRotated_v1, RiRoIAlign and the
// horizontal ROIAlign v0/v1 -- the PRODUCT forward: its three kernel families (merged taps, vector, scalar fallback)
// and the launcher that picks among them.  roi_align.hip holds the entry points; the backward is roi_align_bwd.hip.
// Everything that exists to be measured -- alternative kernels, profiling instantiations of the kernels below, the
// environment knobs that select them -- lives in libjdet_experimental.so, whose RoIAlign translation unit includes this
// header: nothing here reads the environment or compiles conditionally.
//
// Reference semantics (per output element, fp32):
//   python/jdet/ops/roi_align_rotated.py:L21-127 (fwd), L128-255 (bwd)
//   python/jdet/ops/roi_align_rotated_v1.py:L71-145, L193-298
//   python/jdet/ops/riroi_align.py:L70-163, L228-358
//   python/jdet/ops/roi_align.py:L13-204
// The reference launches one CUDA thread per output element (n,c,ph,pw): every thread
// recomputes sin/cos + bin geometry and gathers 16 scattered floats from an NCHW map.
//
// MI355X design (not a translation):
//   * feature map is NHWC, so one bilinear tap is ONE contiguous C-vector: a wave64 reads a
//     256-channel tap with a single global_load_dwordx4 (64 lanes x 16 B = 1 KiB).
//   * one workgroup (4 waves) per (RoI, 256-channel chunk).  Sample geometry (position,
//     4 weights, 4 pixel offsets) is computed ONCE per sample, lane-parallel (lane = sample),
//     and broadcast to the wave with v_readlane -> all control flow in the tap loop is
//     wave-uniform and the weights live in SGPRs.
//   * per-lane accumulation order is exactly the reference's (w1*lt + w2*rt + w3*lb + w4*rb,
//     summed iy-major, then / count) with FMA contraction off -> forward is bit-identical to
//     the CPU oracle.
//   * results are staged in LDS as [channel][bin] and written out as one contiguous,
//     float4-coalesced (C_chunk*PH*PW) block in the reference's (R,C,PH,PW) layout.
#pragma once
#include <type_traits>

#include "roi_geom.h"

namespace {

using namespace jdet_roi;

// ---------------------------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));

// accumulate one sample for the 4 channels of a float4 lane (reference operation order)
__device__ __forceinline__ void acc_sample4(float (&acc)[4], float w1, float w2, float w3, float w4,
                                            const v4f& lt, const v4f& rt, const v4f& lb, const v4f& rb) {
  acc[0] += (w1 * lt.x + w2 * rt.x + w3 * lb.x + w4 * rb.x);
  acc[1] += (w1 * lt.y + w2 * rt.y + w3 * lb.y + w4 * rb.y);
  acc[2] += (w1 * lt.z + w2 * rt.z + w3 * lb.z + w4 * rb.z);
  acc[3] += (w1 * lt.w + w2 * rt.w + w3 * lb.w + w4 * rb.w);
}

// RiRoIAlign (riroi_align.py:L130-152): the channels are C/nO groups of nO orientation planes, and output plane o of
// a group is  r_var * plane (o - ind) + l_var * plane (o - ind + 1)  (indices mod nO) of the sampled value, `ind` and
// the two fractions being per-RoI constants.  Lane owns 4 consecutive channels: a whole group when nO == 4, half of
// one when nO == 8 (the other half sits in the neighbouring lane).  IND is a template argument (the caller switches
// on the wave-uniform `ind`), so every plane lookup is a static register pick -- plus one select on the lane's
// parity when nO == 8, where the two lanes of a pair need planes 4 apart.  Accumulates in the reference's order:
// acc += r_var * val + l_var * val_plus, once per sample.
template <int NO, int IND>
__device__ __forceinline__ void ri_accumulate(float (&acc)[4], const float (&val)[4], int lane, float r_var,
                                              float l_var) {
  if (NO == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      acc[k] += r_var * val[(k - IND + 4) & 3] + l_var * val[(k - IND + 5) & 3];
  } else {
    const bool odd = lane & 1;
    float a[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float other = __shfl_xor(val[k], 1, 64);
      a[k] = odd ? other : val[k];          // planes 0..3 of the group
      a[4 + k] = odd ? val[k] : other;      // planes 4..7
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {           // this lane's output plane o = 4 * odd + k
      const int i0 = (k - IND + 8) & 7, i1 = (k - IND + 9) & 7;
      const float v = odd ? a[i0 ^ 4] : a[i0];
      const float vp = odd ? a[i1 ^ 4] : a[i1];
      acc[k] += r_var * v + l_var * vp;
    }
  }
}

template <int NO>
__device__ __forceinline__ void ri_dispatch(float (&acc)[4], const float (&val)[4], int lane, int ind, float r_var,
                                            float l_var) {
  switch (ind) {   // wave-uniform
    case 0: ri_accumulate<NO, 0>(acc, val, lane, r_var, l_var); break;
    case 1: ri_accumulate<NO, 1>(acc, val, lane, r_var, l_var); break;
    case 2: ri_accumulate<NO, 2>(acc, val, lane, r_var, l_var); break;
    case 3: ri_accumulate<NO, 3>(acc, val, lane, r_var, l_var); break;
    case 4: ri_accumulate<NO, 4 % NO>(acc, val, lane, r_var, l_var); break;
    case 5: ri_accumulate<NO, 5 % NO>(acc, val, lane, r_var, l_var); break;
    case 6: ri_accumulate<NO, 6 % NO>(acc, val, lane, r_var, l_var); break;
    default: ri_accumulate<NO, 7 % NO>(acc, val, lane, r_var, l_var); break;
  }
}

// The same mix with `ind` as a run-time value (wave-uniform or per lane), for the kernels that mix ONCE per finished bin:
// every plane lookup is a 4-way select on (index & 3) plus, for nO == 8, a select between the lane's own registers and
// its pair lane's (the two lanes of a pair hold planes 0-3 / 4-7 of a group).  No register arrays indexed at run time:
// the switch of ri_dispatch above costs 8 template instances whose plane arrays end up in scratch (RiRoIAlign ran
// 92 us against 59 us for the plain dialect at the north-star point).
__device__ __forceinline__ float ri_sel4(const float (&v)[4], int i) {
  const float lo = (i & 1) ? v[1] : v[0], hi = (i & 1) ? v[3] : v[2];
  return (i & 2) ? hi : lo;
}

template <int NO>
__device__ __forceinline__ void ri_mix(float (&out)[4], const float (&val)[4], int lane, int ind, float r_var,
                                       float l_var) {
  if (NO == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      out[k] = 0.f + (r_var * ri_sel4(val, (k - ind) & 3) + l_var * ri_sel4(val, (k - ind + 1) & 3));
  } else {
    const int odd = lane & 1;
    float other[4];
#pragma unroll
    for (int k = 0; k < 4; k++) other[k] = __shfl_xor(val[k], 1, 64);
#pragma unroll
    for (int k = 0; k < 4; k++) {          // this lane's output plane o = 4 * odd + k; source planes (o - ind), (o - ind + 1) mod 8
      const int ta = (4 * odd + k - ind) & 7, tb = (4 * odd + k - ind + 1) & 7;
      const float va = ((ta >> 2) == odd) ? ri_sel4(val, ta & 3) : ri_sel4(other, ta & 3);
      const float vb = ((tb >> 2) == odd) ? ri_sel4(val, tb & 3) : ri_sel4(other, tb & 3);
      out[k] = 0.f + (r_var * va + l_var * vb);
    }
  }
}

// ... and with `ind` as a template argument (the caller switches on the wave-uniform value ONCE, around its whole bin
// loop): every plane lookup is a static register pick.  Lane parity drops out: output plane 4 odd + k reads plane
// (4 odd + t) mod 8 with t = (k - IND) mod 8, i.e. component t & 3 of the lane itself when t < 4, of its pair lane
// otherwise.
template <int NO, int IND>
__device__ __forceinline__ void ri_mix_static(float (&out)[4], const float (&val)[4], float r_var, float l_var) {
  if (NO == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = 0.f + (r_var * val[(k - IND + 4) & 3] + l_var * val[(k - IND + 5) & 3]);
  } else {
    float other[4];
#pragma unroll
    for (int k = 0; k < 4; k++) other[k] = __shfl_xor(val[k], 1, 64);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      constexpr int dummy = 0;
      (void)dummy;
      const int ta = (k - IND + 8) & 7, tb = (k - IND + 9) & 7;
      const float va = ta < 4 ? val[ta & 3] : other[ta & 3];
      const float vb = tb < 4 ? val[tb & 3] : other[tb & 3];
      out[k] = 0.f + (r_var * va + l_var * vb);
    }
  }
}

// one sample into the lane's 4 accumulators; NO == 0: plain RoIAlign, NO == 4 / 8: RiRoIAlign with that many planes
template <int NO>
__device__ __forceinline__ void acc_sample(float (&acc)[4], const RoiGeom& g, int lane, float w1, float w2, float w3,
                                           float w4, const v4f& lt, const v4f& rt, const v4f& lb, const v4f& rb) {
  if constexpr (NO == 0) {
    acc_sample4(acc, w1, w2, w3, w4, lt, rt, lb, rb);
  } else {
    const float val[4] = {(w1 * lt.x + w2 * rt.x + w3 * lb.x + w4 * rb.x), (w1 * lt.y + w2 * rt.y + w3 * lb.y + w4 * rb.y),
                          (w1 * lt.z + w2 * rt.z + w3 * lb.z + w4 * rb.z), (w1 * lt.w + w2 * rt.w + w3 * lb.w + w4 * rb.w)};
    ri_dispatch<NO>(acc, val, lane, g.ind, g.r_var, g.l_var);
  }
}

// ---- vector fast path: C % 4 == 0, map < 2 GiB per image; RiRoI with 4 or 8 orientation planes -------------
// Lane owns 4 consecutive channels.  Taps are fetched with buffer_load_dwordx4 whose per-tap
// pixel byte offset is an SGPR (soffset) -- no per-load 64-bit VALU address arithmetic -- and the
// per-sample geometry is broadcast from the owning lane with v_readlane.
//   NW  = waves per workgroup;  SG = samples whose 4*SG taps are all in flight before first use
// Per-RoI prologue shared by the vector kernels: geometry with the control-flow / addressing
// scalars pinned into SGPRs (hipcc otherwise wraps every buffer_load in a waterfall loop, guide
// T20), and a raw buffer descriptor over the RoI's image (out-of-range reads return 0).
template <int VARIANT, bool TRIG = true>
__device__ __forceinline__ RoiGeom vec_prologue(const float* feat, const float* rois, int r, int C, int H,
                                                int W, int PH, int PW, float spatial_scale,
                                                int sample_num, __amdgpu_buffer_rsrc_t& rsrc, int nO = 1) {
  constexpr int ROI_COLS = (VARIANT == JDET_ROI_HBB_V0 || VARIANT == JDET_ROI_HBB_V1) ? 5 : 6;
  RoiGeom g = roi_geom<VARIANT, TRIG>(rois + (size_t)r * ROI_COLS, spatial_scale, sample_num, PH, PW, nO, false);
  g.batch = __builtin_amdgcn_readfirstlane(g.batch);
  g.ind = __builtin_amdgcn_readfirstlane(g.ind);
  g.grid_h = __builtin_amdgcn_readfirstlane(g.grid_h);
  g.grid_w = __builtin_amdgcn_readfirstlane(g.grid_w);
  const float* img = feat + (size_t)g.batch * H * W * C;
  const unsigned long long img_bits = (unsigned long long)img;
  const unsigned img_lo = __builtin_amdgcn_readfirstlane((unsigned)img_bits);
  const unsigned img_hi = __builtin_amdgcn_readfirstlane((unsigned)(img_bits >> 32));
  const void* img_u = (const void*)(((unsigned long long)img_hi << 32) | img_lo);
  rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(img_u), 0, __builtin_amdgcn_readfirstlane((int)((size_t)H * W * C * 4)), 0x00020000);
  return g;
}

// Direct path for one (RoI, <=256-channel chunk): every tap is a buffer_load_dwordx4 whose pixel
// byte offset is an SGPR; results go to s_out[channel][bin].  NW waves split the bins.
// OUT_CL: results go straight from registers to the channels-last output row (r, bin, c0 + 4*lane .. +3) -- one
// contiguous 1 KiB non-temporal store per (wave, bin), no LDS staging; otherwise to s_out[channel][bin].
template <int VARIANT, int NW, int SG, bool OUT_CL = false, int NO = 0>
__device__ __forceinline__ void direct_chunk(const RoiGeom& g, const __amdgpu_buffer_rsrc_t rsrc, int c0,
                                             int cc, int C, int H, int W, int PW, int nbins, int wave,
                                             int lane, float* __restrict__ s_out, float* __restrict__ out_row = nullptr) {
  const bool lane_ok = lane * 4 < cc;
  const int voff = (c0 + (lane_ok ? lane * 4 : 0)) * 4;  // byte offset of this lane's channels
  const int pix_bytes = C * 4;
  const int spb = g.grid_h * g.grid_w;
  const int nb = (nbins - wave + NW - 1) / NW;
  const int bpc = spb <= 64 ? (spb > 0 ? 64 / spb : 64) : 1;
  const int passes = spb <= 64 ? 1 : (spb + 63) / 64;

  // lane = one sample of this wave's bins; offsets pre-multiplied to bytes
  auto lane_sample = [&](int kg, int pass) -> Sample {
    int my_kb, my_r;
    if (passes == 1) {
      my_kb = spb > 0 ? lane / spb : 0;
      my_r = spb > 0 ? lane % spb : 0;
    } else {
      my_kb = 0;
      my_r = pass * 64 + lane;
    }
    const int my_bin = wave + NW * (kg + my_kb);
    const bool ok = my_kb < bpc && my_bin < nbins && my_r < spb && g.grid_w > 0;
    const int iy = ok ? my_r / g.grid_w : 0;
    const int ix = ok ? my_r % g.grid_w : 0;
    const int bb = ok ? my_bin : 0;
    Sample s = make_sample<VARIANT>(g, bb / PW, bb % PW, iy, ix, H, W);
    s.o1 *= pix_bytes; s.o2 *= pix_bytes; s.o3 *= pix_bytes; s.o4 *= pix_bytes;
    return s;
  };
  auto tap = [&](int soff) -> v4f {
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
  };

  for (int kg = 0; kg < nb; kg += bpc) {
    Sample mine = lane_sample(kg, 0);
    for (int kb = 0; kb < bpc && kg + kb < nb; kb++) {
      const int bin = wave + NW * (kg + kb);
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int pass = 0; pass < passes; pass++) {
        if (passes > 1) mine = lane_sample(kg, pass);
        const int lane0 = passes == 1 ? kb * spb : 0;
        const int ns = passes == 1 ? spb : min(64, spb - pass * 64);
        int j = 0;
        for (; j + SG <= ns; j += SG) {
          Sample sv[SG];
          int all_valid = 1;
#pragma unroll
          for (int u = 0; u < SG; u++) {
            sv[u] = bcast(mine, lane0 + j + u);
            all_valid &= sv[u].valid;
          }
          if (all_valid) {
            v4f t[SG][4];
#pragma unroll
            for (int u = 0; u < SG; u++) {
              t[u][0] = tap(sv[u].o1);
              t[u][1] = tap(sv[u].o2);
              t[u][2] = tap(sv[u].o3);
              t[u][3] = tap(sv[u].o4);
            }
#pragma unroll
            for (int u = 0; u < SG; u++)
              acc_sample<NO>(acc, g, lane, sv[u].w1, sv[u].w2, sv[u].w3, sv[u].w4, t[u][0], t[u][1], t[u][2], t[u][3]);
          } else {
#pragma unroll
            for (int u = 0; u < SG; u++)
              if (sv[u].valid)
                acc_sample<NO>(acc, g, lane, sv[u].w1, sv[u].w2, sv[u].w3, sv[u].w4, tap(sv[u].o1), tap(sv[u].o2),
                               tap(sv[u].o3), tap(sv[u].o4));
          }
        }
        for (; j < ns; j++) {
          const Sample s = bcast(mine, lane0 + j);
          if (s.valid)
            acc_sample<NO>(acc, g, lane, s.w1, s.w2, s.w3, s.w4, tap(s.o1), tap(s.o2), tap(s.o3), tap(s.o4));
        }
      }
      if (lane_ok) {
        if (OUT_CL) {
          const v4f o = {acc[0] / g.count, acc[1] / g.count, acc[2] / g.count, acc[3] / g.count};
          __builtin_nontemporal_store(o, reinterpret_cast<v4f*>(out_row + (size_t)bin * C + c0 + lane * 4));
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++) s_out[(lane * 4 + k) * nbins + bin] = acc[k] / g.count;
        }
      }
    }
  }
}

template <int VARIANT, int NW, int SG, bool OUT_CL = false, int NO = 0>
__global__ __launch_bounds__(NW * 64) void roi_align_fwd_vec_kernel(
    const float* __restrict__ feat, const float* __restrict__ rois, float* __restrict__ out,
    int C, int H, int W, int PH, int PW, float spatial_scale, int sample_num,
    const int32_t* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) float s_out[];  // [cc][nbins]
  const int r = order ? order[blockIdx.x] : blockIdx.x;  // XCD-aware spatial schedule
  const int c0 = blockIdx.y * kChunkC;
  const int cc = min(kChunkC, C - c0);
  const int nbins = PH * PW;
  // wave id is wave-uniform but threadIdx-derived: make that provable (SGPR) for the compiler
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  __amdgpu_buffer_rsrc_t rsrc;
  const RoiGeom g = vec_prologue<VARIANT>(feat, rois, r, C, H, W, PH, PW, spatial_scale, sample_num, rsrc,
                                          NO ? NO : 1);
  if (g.batch < 0) return;  // masked RoI (belongs to another pyramid level): its output rows are not ours
  if (OUT_CL) {
    direct_chunk<VARIANT, NW, SG, true, NO>(g, rsrc, c0, cc, C, H, W, PW, nbins, wave, lane, s_out,
                                                 out + (size_t)r * nbins * C);
    return;
  }
  direct_chunk<VARIANT, NW, SG, false, NO>(g, rsrc, c0, cc, C, H, W, PW, nbins, wave, lane, s_out);
  __syncthreads();
  float* __restrict__ dst = out + ((size_t)r * C + c0) * nbins;
  // coalesced write-out of the contiguous [cc][nbins] block (cc % 4 == 0 -> 16 B aligned)
  const int total = cc * nbins;
  const float4* s4 = reinterpret_cast<const float4*>(s_out);
  float4* d4 = reinterpret_cast<float4*>(dst);
  for (int i = threadIdx.x; i < (total >> 2); i += NW * 64) d4[i] = s4[i];
}

// ---- merged-tap path (sample_num == 2: the configuration every reference config uses) -----------
// PMC on the reference-order kernel above (profiles/r01_roi_align_fwd_rocprofv3_summary.txt): 2714 VALU
// instructions per wave -- 8 fp32 ops per tap-channel-quad with contraction off, 4 divides per bin,
// double-precision trig in every wave -- keep the SIMDs ~45 % busy, and 1.51 M dwordx4 tap loads keep
// the vector-memory path ~60 % busy: co-limited, neither hides behind the other.  This path attacks both:
//   * the 4 samples of a bin sit bin/2 apart; whenever that is under a pixel their 16 taps revisit
//     the same few pixels (bench RoIs: 58 % of the taps are distinct within their bin).  Lane =
//     sample; inside each quad of lanes (= one bin) every tap looks up the other 15, the first
//     occurrence of a pixel takes the summed weight (pre-divided by the sample count), the rest are
//     dropped; survivors are compacted per bin through a 2 KiB/wave LDS scratch (overlaid on the
//     output staging block, before anything is staged) so that lane 4*bin+i holds entries i, 4+i, ...
//   * the tap loop runs over the dense list in batches of 4 loads: per surviving tap one
//     buffer_load_dwordx4 + two v_pk_fma_f32, no guards, no divides.
//   * sin/cos in double once per workgroup (wave 0) instead of once per wave.
// Result = reference value up to fp32 re-association of the weights (<= a few ulp of sum|w.v|);
// The *_reference entry points select the reference-order kernel above (bit-identical to the oracle).
// NO = 4 / 8: RiRoIAlign -- VARIANT is the rotated geometry, the orientation planes are mixed once per bin on the
// finished sum (the reference mixes per sample: equal up to fp32 re-association, like the merged weights).
// ABL = 0 (the per-bin tap loop) or 256 (the rolling window, channels-last output only) in this library.  The experimental
// library instantiates the profiling builds: 32 / 64 rows requested in guarded groups of 2 / 1 (per-bin loop), 128
// workgroup time stamps into the output rows, 512 prologue only (with 256).

// profiling builds (ABL & 128): the 100 MHz wall clock read WHEN `dep` has been produced (the operand pins the order)
__device__ __forceinline__ long long stamp_after(int dep) {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep) : "memory");
  return (long long)t;
}

template <int VARIANT, int NW, int ABL = 0, bool OUT_CL = false, int NO = 0>
__global__ __launch_bounds__(NW * 64) void roi_align_fwd_merged_kernel(
    const float* __restrict__ feat, const float* __restrict__ rois, float* __restrict__ out,
    int C, int H, int W, int PH, int PW, float spatial_scale, const int32_t* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) float s_out[];  // [cc][nbins]; first 2 KiB/wave: tap lists
  __shared__ float s_trig[2];
  long long stamp0 = 0;
  if (ABL & 128) stamp0 = wall_clock64();   // profiling builds: workgroup start / end / placement (scripts/r6_fwd_stamps.py)
  const int r = order ? order[blockIdx.x] : blockIdx.x;
  const int c0 = blockIdx.y * kChunkC;
  const int cc = min(kChunkC, C - c0);
  const int nbins = PH * PW;                       // <= 16 * NW on this path
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  constexpr int ROI_COLS = (VARIANT == JDET_ROI_HBB_V0 || VARIANT == JDET_ROI_HBB_V1) ? 5 : 6;
  constexpr bool kRot = ROI_COLS == 6;
  const float* roi = rois + (size_t)r * ROI_COLS;
  if (kRot && wave == 0 && lane == 0) {
    s_trig[0] = (float)cos((double)roi[5]);
    s_trig[1] = (float)sin((double)roi[5]);
  }
  __amdgpu_buffer_rsrc_t rsrc;
  RoiGeom g = vec_prologue<VARIANT, false>(feat, rois, r, C, H, W, PH, PW, spatial_scale, 2, rsrc);
  if (g.batch < 0) return;
  long long st_a = 0, st_b = 0, st_c = 0, st_d = 0;
  if (ABL & 128) st_a = stamp_after(__float_as_int(g.bin_w));      // RoI row read (order -> row: two dependent loads)
  if (kRot) {
    __syncthreads();
    g.cosT = s_trig[0];
    g.sinT = s_trig[1];
  }
  if (ABL & 128) st_b = stamp_after(__float_as_int(g.cosT));       // double-precision trig of wave 0, barrier

  const bool lane_ok = lane * 4 < cc;
  const int voff = (c0 + (lane_ok ? lane * 4 : 0)) * 4;
  const int pix_bytes = C * 4;
  const int q = lane & 3, kb_mine = lane >> 2;
  // wave w owns bins w, w+NW, ... (measured: better than contiguous runs -- neighbouring bins in flight
  // together share their L1 misses)
  const int nb = (nbins - wave + NW - 1) / NW;
  const int my_bin = wave + NW * kb_mine;
  const bool bin_ok = kb_mine < nb;
  const int bb = bin_ok ? my_bin : 0;
  Sample s = make_sample<VARIANT>(g, bb / PW, bb % PW, q >> 1, q & 1, H, W);
  if (!bin_ok) s.valid = 0;
  const int o[4] = {s.o1 * pix_bytes, s.o2 * pix_bytes, s.o3 * pix_bytes, s.o4 * pix_bytes};
  if (ABL & 128) st_c = stamp_after(o[0] + o[3]);                   // sample geometry
  const float w[4] = {s.w1, s.w2, s.w3, s.w4};
  float tw[4] = {w[0], w[1], w[2], w[3]};
  bool first[4] = {true, true, true, true};
#pragma unroll
  for (int k = 1; k < 4; k++)
#pragma unroll
    for (int j = 0; j < k; j++)
      if (o[j] == o[k]) {   // x_high == x_low / y_high == y_low at the map border
        tw[j] += w[k];      // (first occurrence collects; later ones are dropped)
        first[k] = false;
      }
  // (measured in round 6: the same exchanges as DPP quad_perm moves -- VALU instead of the LDS crossbar -- made the stage
  //  slower, 1.5 -> 2.9 us under the stamps: the prologue competes for VALU issue with the tap loops of the other waves)
  const int qbase = lane & ~3;
#pragma unroll
  for (int d = 1; d < 4; d++) {
    const int src = qbase | ((q + d) & 3);
    const bool earlier = ((q + d) & 3) < q;
    const int ov = __shfl(s.valid, src, 64);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int oo = __shfl(o[j], src, 64);
      const float ww = __shfl(w[j], src, 64);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool same = ov && oo == o[k];
        tw[k] += same ? ww : 0.f;
        first[k] = first[k] && !(same && earlier);
      }
    }
  }
  int ri_ind = 0;
  float ri_l = 0.f, ri_r = 1.f;
  if (NO) {
    ri_params(roi[5], NO, ri_ind, ri_l, ri_r);
    ri_ind = __builtin_amdgcn_readfirstlane(ri_ind);
  }
  const float inv_count = 1.f / g.count;   // count == 4 here: exact
  int keep[4], mycnt = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    keep[k] = s.valid && first[k];
    mycnt += keep[k];
  }
  // compaction: position inside the bin = kept taps of lower quad lanes + own lower kept taps
  int below = 0, n_bin = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int ci = __shfl(mycnt, qbase | i, 64);
    below += i < q ? ci : 0;
    n_bin += ci;
  }
  if (ABL & 128) st_d = stamp_after(n_bin + __float_as_int(tw[0]) + __float_as_int(tw[3]));   // taps merged inside the bins
  int2* list = reinterpret_cast<int2*>(s_out) + wave * 256 + kb_mine * 16;
  int pos = below;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (keep[k]) list[pos++] = make_int2(o[k], __float_as_int(tw[k] * inv_count));
  __builtin_amdgcn_wave_barrier();   // list is private to the wave; LDS ops of a wave retire in order
  if constexpr ((ABL & 256) != 0 && OUT_CL) {
    // ---- rolling window (round 6).  Stamps of the per-bin loop below (scripts/r6_fwd_stamps.py): a workgroup lives
    // 20.8 us whatever its RoI's size (18 us for the smallest quarter, 25 us for the largest) -- each wave walks its 13 bins
    // one memory round trip at a time (request <= 16 rows, wait for ALL of them, 64 FMAs, store, next bin), and with
    // 2000 workgroups on 1024 slots the launch is two such lifetimes plus a ragged end of one.  Here the wave's rows form
    // ONE sequence of groups of 4 (bin after bin; lane g of the wave holds group g: 4 offsets, 4 weights, the bin and
    // whether the group closes it) and a ring of RING groups stays in flight: the oldest group is waited for alone
    // (counted vmcnt), folded into the accumulator, its registers refilled with the group RING ahead; a bin's row is
    // stored when its last group has been folded.  Same entries, same order, same fmaf as the loop below: bit-identical.
    constexpr int RING = 4;
    const int ngq = bin_ok ? (n_bin + 3) >> 2 : 0;          // groups of this quad's bin (the same in its four lanes)
    // first group of the quad's bin = groups of the bins below: four ballots over the quads' first lanes, bits below the lane
    int below_g = 0, gtot = 0;
#pragma unroll
    for (int b = 1; b <= 4; b++) {
      const unsigned long long mk = __ballot(q == 0 && ngq >= b);
      below_g += __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0));
      gtot += __builtin_popcountll(mk);
    }
    const int start = below_g - (q > 0 ? ngq : 0);          // (lanes 1..3 of a quad counted their own bin's bits)
    // a bin without a single valid sample has no group: its row of zeros is written here
    for (unsigned long long empty = __ballot(bin_ok && q == 0 && n_bin == 0); empty; empty &= empty - 1) {
      const int bin0 = jdet_readlane_i(my_bin, __builtin_ctzll(empty));
      if (lane_ok)
        __builtin_nontemporal_store(v4f{0.f, 0.f, 0.f, 0.f},
                                    reinterpret_cast<v4f*>(out + ((size_t)r * nbins + bin0) * C + c0 + lane * 4));
    }
    // lane (bin, q) forms group q of its bin from the bin's list and PUSHES it to lane start + q (ds_permute: one LDS
    // crossbar trip for the nine words; lanes without a group aim at lane 63, which no group reaches: at most 52 groups)
    const int2* lw = reinterpret_cast<const int2*>(s_out) + wave * 256 + kb_mine * 16;
    const int2 g0 = lw[0];
    int go[4], gmeta;
    float gw[4];
    {
      const int dst = (q < ngq ? start + q : 63) << 2;
      const int my_meta = (my_bin << 1) | (q == ngq - 1 ? 1 : 0);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int2 e = lw[4 * q + i];
        const bool live = 4 * q + i < n_bin;
        go[i] = __builtin_amdgcn_ds_permute(dst, live ? e.x : g0.x);
        gw[i] = __int_as_float(__builtin_amdgcn_ds_permute(dst, live ? e.y : 0));
      }
      gmeta = __builtin_amdgcn_ds_permute(dst, my_meta);
    }
    // The row loads are inline assembly and the kernel counts its own vmcnt: with the builtin, hipcc (ROCm 7.2) folds the
    // conditional row stores into its scoreboard and drains the whole ring (vmcnt(3) .. (0)) at the first group of every
    // turn.  Loads and stores of a wave retire in order on the VM counter, so "all but the 4 k youngest" is safe whatever
    // stores sit in between (it then also waits for a younger load or two).  Form (ii) of the guide's 5.7: "=&v"
    // destinations, then one wait statement naming the four registers "+v" before their first use.
    typedef int v4i_ __attribute__((ext_vector_type(4)));
    v4i_ rs;
    {
      const unsigned long long img_bits = (unsigned long long)(feat + (size_t)g.batch * H * W * C);
      rs.x = __builtin_amdgcn_readfirstlane((int)(unsigned)img_bits);
      rs.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(img_bits >> 32) & 0xffffu));
      rs.z = __builtin_amdgcn_readfirstlane((int)((size_t)H * W * C * 4));
      rs.w = 0x00020000;
    }
    if (ABL & 512) {   // profiling builds: the prologue alone (12 us at the north-star point: profiles/r06_roi_fwd_ring.md)
      if (lane < gtot)
        out[((size_t)r * nbins + wave) * C + lane] = __int_as_float(go[0] + go[1] + go[2] + go[3] + gmeta) + gw[0] + gw[1] + gw[2] + gw[3];
      return;
    }
    long long stamp_mid = 0;
    if (ABL & 128) stamp_mid = stamp_after(go[0] + go[3] + gmeta);  // lists compacted, group table built
    auto ring = [&](auto ind_c) {
      constexpr int IND = decltype(ind_c)::value;
      v4f t[RING][4];
      v4f acc = {0.f, 0.f, 0.f, 0.f};
      auto issue = [&](auto sc, int gj) {
        constexpr int S = decltype(sc)::value;
        const int o0 = jdet_readlane_i(go[0], gj), o1 = jdet_readlane_i(go[1], gj);
        const int o2 = jdet_readlane_i(go[2], gj), o3 = jdet_readlane_i(go[3], gj);
        v4f &a0 = t[S][0], &a1 = t[S][1], &a2 = t[S][2], &a3 = t[S][3];   // (asm operands do not capture by themselves)
        const int vo = voff;
        const v4i_ rd = rs;
        asm volatile(
            "s_nop 4\n\t"
            "buffer_load_dwordx4 %0, %4, %5, %6 offen\n\t"
            "buffer_load_dwordx4 %1, %4, %5, %7 offen\n\t"
            "buffer_load_dwordx4 %2, %4, %5, %8 offen\n\t"
            "buffer_load_dwordx4 %3, %4, %5, %9 offen"
            : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3)
            : "v"(vo), "s"(rd), "s"(o0), "s"(o1), "s"(o2), "s"(o3)
            : "memory");
      };
      // wait until at most 4 * younger row loads of this wave are outstanding: the group in ring slot S has landed
      auto landed = [&](auto sc, int younger) {
        constexpr int S = decltype(sc)::value;
        v4f &a0 = t[S][0], &a1 = t[S][1], &a2 = t[S][2], &a3 = t[S][3];
        // (the waits carry no register operands: four statements that each tie the ring registers "+v" meet in PHIs, and
        //  the copies hipcc places for them READ the registers ahead of the wait -- lanes of garbage at the map border, where
        //  the run-time counts are taken; one operand-carrying pin after the join orders the FMAs behind whichever wait ran)
        if (younger >= 3)
          asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else if (younger == 2)
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (younger == 1)
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "memory");
      };
      auto consume = [&](auto sc, int gi, int younger) {
        constexpr int S = decltype(sc)::value;
        landed(sc, younger);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float wt = jdet_readlane_f(gw[i], gi);
          acc.x = __builtin_fmaf(wt, t[S][i].x, acc.x);
          acc.y = __builtin_fmaf(wt, t[S][i].y, acc.y);
          acc.z = __builtin_fmaf(wt, t[S][i].z, acc.z);
          acc.w = __builtin_fmaf(wt, t[S][i].w, acc.w);
        }
        const int meta = jdet_readlane_i(gmeta, gi);
        if (meta & 1) {
          v4f o4 = acc;
          if constexpr (NO != 0) {
            const float val[4] = {acc.x, acc.y, acc.z, acc.w};
            float mixed[4];
            ri_mix_static<NO, IND>(mixed, val, ri_r, ri_l);
            o4 = v4f{mixed[0], mixed[1], mixed[2], mixed[3]};
          }
          if (lane_ok)
            __builtin_nontemporal_store(o4, reinterpret_cast<v4f*>(out + ((size_t)r * nbins + (meta >> 1)) * C + c0 + lane * 4));
          acc = v4f{0.f, 0.f, 0.f, 0.f};
        }
      };
      using S0 = std::integral_constant<int, 0>;
      using S1 = std::integral_constant<int, 1>;
      using S2 = std::integral_constant<int, 2>;
      using S3 = std::integral_constant<int, 3>;
      if (0 < gtot) issue(S0{}, 0);
      if (1 < gtot) issue(S1{}, 1);
      if (2 < gtot) issue(S2{}, 2);
      if (3 < gtot) issue(S3{}, 3);
      int gq = 0;
      for (; gq + 2 * RING <= gtot; gq += RING) {     // a whole ring to fold AND a whole ring to request
        consume(S0{}, gq + 0, 3); issue(S0{}, gq + 0 + RING);
        consume(S1{}, gq + 1, 3); issue(S1{}, gq + 1 + RING);
        consume(S2{}, gq + 2, 3); issue(S2{}, gq + 2 + RING);
        consume(S3{}, gq + 3, 3); issue(S3{}, gq + 3 + RING);
      }
      // the last turns: group gi has min(gtot, gi + RING) - 1 - gi younger groups in flight
      auto younger_of = [&](int gi) { return min(gtot, gi + RING) - 1 - gi; };
      if (gq + 0 < gtot) { consume(S0{}, gq + 0, younger_of(gq + 0)); if (gq + 0 + RING < gtot) issue(S0{}, gq + 0 + RING); }
      if (gq + 1 < gtot) { consume(S1{}, gq + 1, younger_of(gq + 1)); if (gq + 1 + RING < gtot) issue(S1{}, gq + 1 + RING); }
      if (gq + 2 < gtot) { consume(S2{}, gq + 2, younger_of(gq + 2)); if (gq + 2 + RING < gtot) issue(S2{}, gq + 2 + RING); }
      if (gq + 3 < gtot) { consume(S3{}, gq + 3, younger_of(gq + 3)); if (gq + 3 + RING < gtot) issue(S3{}, gq + 3 + RING); }
      gq += RING;
      if (gq + 0 < gtot) consume(S0{}, gq + 0, younger_of(gq + 0));
      if (gq + 1 < gtot) consume(S1{}, gq + 1, younger_of(gq + 1));
      if (gq + 2 < gtot) consume(S2{}, gq + 2, younger_of(gq + 2));
      if (gq + 3 < gtot) consume(S3{}, gq + 3, younger_of(gq + 3));
    };
    if constexpr (NO == 0) {
      ring(std::integral_constant<int, 0>{});
    } else {
      switch (ri_ind) {   // wave-uniform
        case 0: ring(std::integral_constant<int, 0>{}); break;
        case 1: ring(std::integral_constant<int, 1>{}); break;
        case 2: ring(std::integral_constant<int, 2>{}); break;
        case 3: ring(std::integral_constant<int, 3>{}); break;
        case 4: ring(std::integral_constant<int, 4 % (NO ? NO : 1)>{}); break;
        case 5: ring(std::integral_constant<int, 5 % (NO ? NO : 1)>{}); break;
        case 6: ring(std::integral_constant<int, 6 % (NO ? NO : 1)>{}); break;
        default: ring(std::integral_constant<int, 7 % (NO ? NO : 1)>{}); break;
      }
    }
    if (ABL & 128) {   // (profiling builds: workgroup stamps, as at the end of the per-bin path)
      __syncthreads();
      if (threadIdx.x == 0) {
        const long long stamp1 = wall_clock64();
        int* d = reinterpret_cast<int*>(out + (size_t)r * nbins * C);
        d[0] = (int)(stamp0 & 0xffffffff); d[1] = (int)(stamp0 >> 32);
        d[2] = (int)(stamp1 & 0xffffffff); d[3] = (int)(stamp1 >> 32);
        d[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        d[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20) | ((int)(stamp_mid - stamp0) << 8);   // + prologue ticks
        d[6] = (blockIdx.x & 7) | ((int)(st_a - stamp0) << 3) | ((int)(st_b - stamp0) << 13) | ((int)(st_c - stamp0) << 23);
        d[7] = 0x5741 | ((int)(st_d - stamp0) << 16);
      }
    }
    return;
  }
  int e_o[4];
  float e_w[4];
  const int2 e0 = list[0];
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int2 e = list[4 * b + q];
    const bool live = 4 * b + q < n_bin;
    e_o[b] = live ? e.x : e0.x;                       // pad: entry 0's pixel (a tap of this bin) ...
    e_w[b] = live ? __int_as_float(e.y) : 0.f;        // ... with weight 0
  }
  __syncthreads();   // every wave has read its list: s_out may now be used for results
  long long stamp_mid = 0;
  if (ABL & 128) stamp_mid = wall_clock64();

  auto tap = [&](int soff) -> v4f {
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
  };
  // (RiRoIAlign: the bin loop is instantiated once per orientation shift and entered through one switch on the
  //  wave-uniform `ind`, so that the mix inside is pure register renaming)
  auto bins = [&](auto ind_c) {
  constexpr int IND = decltype(ind_c)::value;
  constexpr int GR = (ABL & 64) ? 1 : (ABL & 32) ? 2 : 4;
  for (int kb = 0; kb < nb; kb++) {
    const int bin = wave + NW * kb;
    const int l0 = kb * 4;
    const int n = jdet_readlane_i(n_bin, l0);
    v4f t[4][4];
    // rows are requested in groups of GR entries (wave-uniform guards): a bin's list is padded to a multiple of GR with
    // weight-0 copies of its first pixel, and a padded row costs its 16 vector-L1 accesses like any other
#pragma unroll
    for (int b = 0; b < 4; b++)
      if (4 * b < n) {
#pragma unroll
        for (int i = 0; i < 4; i += GR)
          if (GR == 4 || 4 * b + i < n) {
#pragma unroll
            for (int u = 0; u < GR; u++) t[b][i + u] = tap(jdet_readlane_i(e_o[b], l0 + i + u));
          }
      }
    v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; b++)
      if (4 * b < n) {
#pragma unroll
        for (int i = 0; i < 4; i += GR)
          if (GR == 4 || 4 * b + i < n) {
#pragma unroll
            for (int u = 0; u < GR; u++) {
              const float wt = jdet_readlane_f(e_w[b], l0 + i + u);
              acc.x = __builtin_fmaf(wt, t[b][i + u].x, acc.x);
              acc.y = __builtin_fmaf(wt, t[b][i + u].y, acc.y);
              acc.z = __builtin_fmaf(wt, t[b][i + u].z, acc.z);
              acc.w = __builtin_fmaf(wt, t[b][i + u].w, acc.w);
            }
          }
      }
    if constexpr (NO != 0) {
      const float val[4] = {acc.x, acc.y, acc.z, acc.w};
      float mixed[4];
      ri_mix_static<NO, IND>(mixed, val, ri_r, ri_l);
      acc = v4f{mixed[0], mixed[1], mixed[2], mixed[3]};
    }
    if (lane_ok) {
      if (OUT_CL) {   // channels-last row (r, bin, :): one contiguous 1 KiB store per wave, no LDS staging
        __builtin_nontemporal_store(acc, reinterpret_cast<v4f*>(out + ((size_t)r * nbins + bin) * C + c0 + lane * 4));
      } else {
        s_out[(lane * 4 + 0) * nbins + bin] = acc.x;
        s_out[(lane * 4 + 1) * nbins + bin] = acc.y;
        s_out[(lane * 4 + 2) * nbins + bin] = acc.z;
        s_out[(lane * 4 + 3) * nbins + bin] = acc.w;
      }
    }
  }
  };
  if constexpr (NO == 0) {
    bins(std::integral_constant<int, 0>{});
  } else {
    switch (ri_ind) {   // wave-uniform
      case 0: bins(std::integral_constant<int, 0>{}); break;
      case 1: bins(std::integral_constant<int, 1>{}); break;
      case 2: bins(std::integral_constant<int, 2>{}); break;
      case 3: bins(std::integral_constant<int, 3>{}); break;
      case 4: bins(std::integral_constant<int, 4 % (NO ? NO : 1)>{}); break;
      case 5: bins(std::integral_constant<int, 5 % (NO ? NO : 1)>{}); break;
      case 6: bins(std::integral_constant<int, 6 % (NO ? NO : 1)>{}); break;
      default: bins(std::integral_constant<int, 7 % (NO ? NO : 1)>{}); break;
    }
  }
  if (OUT_CL) {
    if (ABL & 128) {   // the stamps overwrite the first 8 words of the RoI's first output row
      __syncthreads();
      if (threadIdx.x == 0) {
        const long long stamp1 = wall_clock64();
        int* d = reinterpret_cast<int*>(out + (size_t)r * nbins * C);
        d[0] = (int)(stamp0 & 0xffffffff); d[1] = (int)(stamp0 >> 32);
        d[2] = (int)(stamp1 & 0xffffffff); d[3] = (int)(stamp1 >> 32);
        d[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID: wave / SIMD / CU / SH / SE
        d[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20) | ((int)(stamp_mid - stamp0) << 8);    // XCC_ID + prologue ticks
        d[6] = blockIdx.x;
        d[7] = 0x5741;
      }
    }
    return;
  }
  __syncthreads();
  float* __restrict__ dst = out + ((size_t)r * C + c0) * nbins;
  const int total = cc * nbins;
  // write-once output: non-temporal stores keep the 100 MB result stream from evicting map lines out of L2
  // (67.5 -> 64.6 us/step)
  typedef float v4s __attribute__((ext_vector_type(4)));
  const v4s* sv = reinterpret_cast<const v4s*>(s_out);
  v4s* dv = reinterpret_cast<v4s*>(dst);
  for (int i = threadIdx.x; i < (total >> 2); i += NW * 64) __builtin_nontemporal_store(sv[i], &dv[i]);
}

// (An LDS pixel-cache variant -- per-RoI bitmap + rank dedup, distinct pixels staged once per 64-channel pass, taps
// served by ds_read_b128 -- was built and measured at 155 us against 69 us for the direct path at the time: four
// channel passes with two barriers each and 2 workgroups per CU leave the vector-memory path idle most of the time.
// Removed; DESIGN.md 3.1 / 7 describe what would have to be different.)

template <int VARIANT, int CHMAP>
__global__ __launch_bounds__(kBlock) void roi_align_fwd_kernel(
    const float* __restrict__ feat, const float* __restrict__ rois, float* __restrict__ out,
    int C, int H, int W, int PH, int PW, float spatial_scale, int sample_num, int nO,
    const int32_t* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) float s_out[];  // [cc][nbins]
  constexpr int ROI_COLS = (VARIANT == JDET_ROI_HBB_V0 || VARIANT == JDET_ROI_HBB_V1) ? 5 : 6;
  constexpr int NW = kBlock / 64;
  const int r = order ? order[blockIdx.x] : blockIdx.x;
  const int c0 = blockIdx.y * kChunkC;
  const int cc = min(kChunkC, C - c0);
  const int nbins = PH * PW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  const RoiGeom g = roi_geom<VARIANT>(rois + (size_t)r * ROI_COLS, spatial_scale, sample_num, PH,
                                      PW, nO, false);
  if (g.batch < 0) return;  // masked RoI (block-uniform)
  const float* __restrict__ img = feat + (size_t)g.batch * H * W * C;

  int src0[4], src1[4];
  bool cval[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int cl = chan_of<CHMAP>(lane, k);
    cval[k] = cl < cc;
    const int ch = c0 + (cval[k] ? cl : 0);
    if (VARIANT == JDET_ROI_RIROI) {
      const int c = ch / nO, o = ch % nO;
      const int ind_rot = (o - g.ind + nO) % nO;
      const int ind_rot_plus = (ind_rot + 1 + nO) % nO;
      src0[k] = c * nO + ind_rot;
      src1[k] = c * nO + ind_rot_plus;
    } else {
      src0[k] = ch;
      src1[k] = ch;
    }
  }

  const int spb = g.grid_h * g.grid_w;
  const int nb = (nbins - wave + NW - 1) / NW;
  const int bpc = spb <= 64 ? (spb > 0 ? 64 / spb : 64) : 1;
  const int passes = spb <= 64 ? 1 : (spb + 63) / 64;

  auto lane_sample = [&](int kg, int pass) -> Sample {
    int my_kb, my_r;
    if (passes == 1) {
      my_kb = spb > 0 ? lane / spb : 0;
      my_r = spb > 0 ? lane % spb : 0;
    } else {
      my_kb = 0;
      my_r = pass * 64 + lane;
    }
    const int my_bin = wave + NW * (kg + my_kb);
    const bool ok = my_kb < bpc && my_bin < nbins && my_r < spb && g.grid_w > 0;
    const int iy = ok ? my_r / g.grid_w : 0;
    const int ix = ok ? my_r % g.grid_w : 0;
    const int bb = ok ? my_bin : 0;
    return make_sample<VARIANT>(g, bb / PW, bb % PW, iy, ix, H, W);
  };

  for (int kg = 0; kg < nb; kg += bpc) {
    Sample mine = lane_sample(kg, 0);
    for (int kb = 0; kb < bpc && kg + kb < nb; kb++) {
      const int bin = wave + NW * (kg + kb);
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int pass = 0; pass < passes; pass++) {
        if (passes > 1) mine = lane_sample(kg, pass);
        const int lane0 = passes == 1 ? kb * spb : 0;
        const int ns = passes == 1 ? spb : min(64, spb - pass * 64);
        for (int j = 0; j < ns; j++) {
          const Sample s = bcast(mine, lane0 + j);
          if (!s.valid) continue;  // reference returns 0 for out-of-map samples
#pragma unroll
          for (int k = 0; k < 4; k++) {
            if (!cval[k]) continue;
            const float lt = img[(size_t)s.o1 * C + src0[k]];
            const float rt = img[(size_t)s.o2 * C + src0[k]];
            const float lb = img[(size_t)s.o3 * C + src0[k]];
            const float rb = img[(size_t)s.o4 * C + src0[k]];
            const float val = (s.w1 * lt + s.w2 * rt + s.w3 * lb + s.w4 * rb);
            if (VARIANT == JDET_ROI_RIROI) {
              const float lt1 = img[(size_t)s.o1 * C + src1[k]];
              const float rt1 = img[(size_t)s.o2 * C + src1[k]];
              const float lb1 = img[(size_t)s.o3 * C + src1[k]];
              const float rb1 = img[(size_t)s.o4 * C + src1[k]];
              const float val_plus = (s.w1 * lt1 + s.w2 * rt1 + s.w3 * lb1 + s.w4 * rb1);
              acc[k] += g.r_var * val + g.l_var * val_plus;
            } else {
              acc[k] += val;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (cval[k]) s_out[chan_of<CHMAP>(lane, k) * nbins + bin] = acc[k] / g.count;
    }
  }
  __syncthreads();
  float* __restrict__ dst = out + ((size_t)r * C + c0) * nbins;
  const int total = cc * nbins;
  if (((total & 3) == 0) && ((((size_t)r * C + c0) * nbins) & 3) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(s_out);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = threadIdx.x; i < (total >> 2); i += kBlock) d4[i] = s4[i];
  } else {
    for (int i = threadIdx.x; i < total; i += kBlock) dst[i] = s_out[i];
  }
}

// ---------------------------------------------------------------------------------------------
// Launcher
// ---------------------------------------------------------------------------------------------
// Arithmetic of a forward call (an argument of the launcher, chosen by the ENTRY POINT -- there is no process-wide
// mode): merged taps (the product entry points) or the reference's operation order (the *_reference entry points:
// bit-identical to the CPU oracle, the parity twin).
constexpr int kFwdMerged = 0, kFwdReference = 1;

// Launch shape of the vector kernels: the winners of the tuning ladders of rounds 1-3 (2 / 4 / 8 / 16 waves per workgroup,
// 2 / 4 / 8 samples in flight; profiles/r01_roi_align_fwd_ablations.txt).
constexpr int kFwdWaves = 4, kFwdSG = 4;
// The merged kernel keeps its per-wave tap lists in the first 2 KiB / wave of the dynamic LDS block (the request has
// room for 8 waves).
constexpr size_t kFwdListLds = 8 * 2048;
// LDS request of the channels-last merged launch.  It caps the workgroups per CU at 4 (36 KiB each; the tap lists need
// 16): one workgroup fewer in flight per CU leaves the time where it is (59.4 vs 60.9 us at the north-star point) and
// cuts the reads beyond the L2 by 14 % (1.34 M vs 1.55 M 128-byte requests, profiles/r03_roi_pool_notes.md) -- fewer
// RoIs in flight, smaller working set.
constexpr size_t kFwdClLds = 36 * 1024;

// The vector kernels: C % 4 == 0 and a map under 2 GiB per image.  NO = 0, or the orientation planes (4 / 8) of a
// RiRoIAlign call, which are mixed in registers: once per bin on the merged path (rotated geometry), per sample in
// the reference's order.
template <int VARIANT, int NO>
int launch_fwd_vec(const float* feat, const float* rois, float* out, int R, int C, int H, int W, int PH, int PW,
                   float scale, int sample_num, const int32_t* order, hipStream_t st, bool out_cl, int mode) {
  constexpr int V = NO ? JDET_ROI_ROTATED : VARIANT;
  const dim3 grid(R, jdet_cdiv(C, kChunkC)), block(kFwdWaves * 64);
  const size_t lds = (size_t)min(C, kChunkC) * PH * PW * sizeof(float);   // the (channel, bin) staging block of an NCHW result
  const bool merged = sample_num == 2 && mode != kFwdReference && PH * PW <= 64 && (out_cl || lds >= kFwdListLds);
  if (merged && out_cl)   // rolling-window tap loop, rows stored straight from registers
    hipLaunchKernelGGL((roi_align_fwd_merged_kernel<V, kFwdWaves, 256, true, NO>), grid, block,
                       NO ? kFwdListLds : kFwdClLds, st, feat, rois, out, C, H, W, PH, PW, scale, order);
  else if (merged)
    hipLaunchKernelGGL((roi_align_fwd_merged_kernel<V, kFwdWaves, 0, false, NO>), grid, block, lds, st, feat, rois, out,
                       C, H, W, PH, PW, scale, order);
  else if (out_cl)
    hipLaunchKernelGGL((roi_align_fwd_vec_kernel<VARIANT, kFwdWaves, kFwdSG, true, NO>), grid, block, 16, st, feat,
                       rois, out, C, H, W, PH, PW, scale, sample_num, order);
  else
    hipLaunchKernelGGL((roi_align_fwd_vec_kernel<VARIANT, kFwdWaves, kFwdSG, false, NO>), grid, block, lds, st, feat,
                       rois, out, C, H, W, PH, PW, scale, sample_num, order);
  return jdet_launch_status();
}

template <int VARIANT>
int launch_fwd(const float* feat, const float* rois, float* out, int R, int C, int H, int W, int PH,
               int PW, float scale, int sample_num, int nO, const int32_t* order, hipStream_t st,
               bool out_cl = false, int mode = kFwdMerged) {
  const bool vec_ok = (C % 4 == 0) && (size_t)H * W * C * 4 < (1ull << 31);
  if constexpr (VARIANT == JDET_ROI_RIROI) {
    if (vec_ok && nO == 8)
      return launch_fwd_vec<VARIANT, 8>(feat, rois, out, R, C, H, W, PH, PW, scale, sample_num, order, st, out_cl, mode);
    if (vec_ok && nO == 4)
      return launch_fwd_vec<VARIANT, 4>(feat, rois, out, R, C, H, W, PH, PW, scale, sample_num, order, st, out_cl, mode);
  } else {
    if (vec_ok)
      return launch_fwd_vec<VARIANT, 0>(feat, rois, out, R, C, H, W, PH, PW, scale, sample_num, order, st, out_cl, mode);
  }
  // channels-last output: vector kernels only (the callers check jdet_roi_align_forward_cl_supported)
  if (out_cl) return JDET_E_UNSUPPORTED;
  const dim3 grid(R, jdet_cdiv(C, kChunkC));
  const size_t lds = (size_t)min(C, kChunkC) * PH * PW * sizeof(float);
  if (C % 4 == 0 && VARIANT != JDET_ROI_RIROI)
    hipLaunchKernelGGL((roi_align_fwd_kernel<VARIANT, 0>), grid, dim3(kBlock), lds, st, feat, rois, out,
                       C, H, W, PH, PW, scale, sample_num, nO, order);
  else
    hipLaunchKernelGGL((roi_align_fwd_kernel<VARIANT, 1>), grid, dim3(kBlock), lds, st, feat, rois, out,
                       C, H, W, PH, PW, scale, sample_num, nO, order);
  return jdet_launch_status();
}

}  // namespace
