// What the fp32-MFMA implicit-GEMM convolutions (conv_igemm.hip, conv_bn_kernel.h) hold in common, once: the tile
// constants, the LDS swizzle, the XCD-aware tile order, an output row's pixel, the MFMAs of a K step, the index forms of
// the KG = 2 hand-over and of the C/D layout, and the host rules both launch plans use.  The K pipeline itself is
// conv_mfma_loop.inc.  See conv_igemm.hip's header for the tiling.  What differs stays in the kernels: how a tap's source
// offsets are formed (their `advance` / `load_set`) and what happens to the accumulators.
// Everything here compiles to the machine code the kernels had with these pieces written out in each of them
// (profiles/conv_split_machine_code.md).  That is why three short loops are still written in both kernels -- fragment
// offsets, accumulator zeroing, the KG = 2 hand-over: as functions with reference outputs called from the kernel body
// they changed register allocation (and added 4 B of scratch to one instantiation); they call swz_bytes / red_index here.
// conv_wgrad.hip (K-major operands, its own LDS layout and loop) takes only the typedefs, kOob, buf_load and out_dim.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr unsigned kOob = 0xFFFFFFF0u;   // a byte offset past every buffer: the load returns zeros

__device__ __forceinline__ v4f buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// byte position of chunk (4 floats) `chunk` of LDS row `row`: chunk c of row r is stored at position c ^ f(r)
template <int BK>
__device__ __forceinline__ int swz_bytes(int row, int chunk) {
  return (row * BK + ((chunk ^ (BK == 16 ? (row >> 2) & 3 : (row >> 1) & 7)) << 2)) * 4;
}

// one workgroup = 4 * KG waves, BT x BT outputs, K step = BK channels of one tap
template <int BT, int BK, int KG>
struct MfmaTile {
  static constexpr int NTHR = 256 * KG;
  static constexpr int T = BT / 64;             // 32 x 32 tiles per wave and direction
  static constexpr int CH = BK / 4;             // 16-byte chunks per LDS row
  static constexpr int RPP = NTHR / CH;         // loader: RPP rows x CH chunks per pass
  static constexpr int PASSES = BT / RPP;
  static constexpr int TILE = BT * BK * 4;      // bytes of one operand tile; LDS holds [buffer][A | B] = 4 * TILE
  static constexpr int QN = BK / 8 / KG;        // 8-deep slices per wave and K step
  static_assert(PASSES >= 1 && QN >= 1, "tile shape");
  static_assert(KG == 1 || 4 * T * T * 16 * 64 * 4 <= 4 * TILE, "reduction buffer");
};

// ---- XCD-aware tile id: consecutive workgroup ids go round-robin over the 8 XCDs, so XCD x takes the x-th contiguous
// band of M tiles with the N tiles of one M tile adjacent.
// (32-bit unsigned index arithmetic throughout the prologue: the hosts refuse positions * channels >= 2^30.  Round 6,
//  workgroup time stamps -- scripts/r6_conv_stamps.py -- showed 7-8.6 us between a workgroup's start and its first operand
//  request on the layers that fill the chip four workgroups per CU: 64-bit divisions, ~200 VALU instructions each, run by
//  sixteen waves per CU at once)
// returns the logical tile id: M tile = id / N tiles, N tile = the rest
__device__ __forceinline__ int xcd_logical() {
  const int total = gridDim.x;
  int logical = blockIdx.x;
  if ((total & 7) == 0) logical = (blockIdx.x & 7) * (total >> 3) + (blockIdx.x >> 3);
  return logical;
}

// output row lm of an (N, Ho, Wo) map -> ok = inside the map, image and (y, x) * scale (zeros outside); scale = the stride
// takes the row straight to its input pixel
__device__ __forceinline__ void row_pixel(long lm, long M, int Ho, int Wo, int scale, bool& ok, int& img, int& y, int& x) {
  ok = lm < M;
  img = y = x = 0;
  if (ok) {
    const unsigned hw = (unsigned)(Ho * Wo), ulm = (unsigned)lm;
    const unsigned im = ulm / hw;
    const unsigned rem = ulm - im * hw;
    const unsigned oy = rem / (unsigned)Wo;
    img = (int)im;
    y = (int)oy * scale;
    x = (int)(rem - oy * (unsigned)Wo) * scale;
  }
}

// ---- compute role: wave (kg, wm, wn) owns outputs [wm*BT/2, +BT/2) x [wn*BT/2, +BT/2) and the 8-deep slices
// q = qq * KG + kg of every K step; fa_off / fb_off are the byte positions of its lane's fragments (tile 0, buffer 0).
// the MFMAs of one K step out of LDS buffer `buf`: ONE ds_read_b128 per operand tile feeds four MFMAs
template <int BT, int BK, int KG>
__device__ __forceinline__ void mfma_step(const char* s_raw, int buf, const int (&fa_off)[MfmaTile<BT, BK, KG>::QN],
                                          const int (&fb_off)[MfmaTile<BT, BK, KG>::QN],
                                          v16f (&acc)[MfmaTile<BT, BK, KG>::T][MfmaTile<BT, BK, KG>::T]) {
  constexpr int T = MfmaTile<BT, BK, KG>::T, QN = MfmaTile<BT, BK, KG>::QN, TILE = MfmaTile<BT, BK, KG>::TILE;
  const char* sb = s_raw + buf * 2 * TILE;
#pragma unroll
  for (int qq = 0; qq < QN; qq++) {
    v4f fa[T], fb[T];
#pragma unroll
    for (int i = 0; i < T; i++) {       // tile i: 32 rows further = the same swizzle (f repeats every 16 / 32 rows)
      fa[i] = *reinterpret_cast<const v4f*>(sb + fa_off[qq] + i * 32 * BK * 4);
      fb[i] = *reinterpret_cast<const v4f*>(sb + fb_off[qq] + i * 32 * BK * 4);
    }
#pragma unroll
    for (int kk = 0; kk < 4; kk++)
#pragma unroll
      for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][kk], fb[j][kk], acc[i][j], 0, 0, 0);
  }
}

// ---- KG = 2: the second wave group hands its partial tile over through LDS (the operand buffers are free after the K
// loop) as [wave & 3][T*T*16][64 lanes] and leaves; the first group reads the values back tile by tile at red_index (no
// second accumulator set live).
template <int T>
__device__ __forceinline__ int red_index(int wave, int lane, int i, int j, int e) {
  return (((wave & 3) * T * T + i * T + j) * 16 + e) * 64 + lane;
}

// C/D layout of the 32 x 32 MFMA: column = lane & 31, row = cd_row(reg) + 4 * (lane >> 5)
__device__ __forceinline__ constexpr int cd_row(int e) { return (e & 3) + 8 * (e >> 2); }

using Set0 = std::integral_constant<int, 0>;      // the register sets of the K pipeline (conv_mfma_loop.inc)
using Set1 = std::integral_constant<int, 1>;

// ---- host: the rules both launch plans use ----
inline int out_dim(int in, int R, int stride) { return (in + 2 * (R / 2) - R) / stride + 1; }

// K steps split over workgroups for small maps (a tile's long reduction is otherwise the floor of the launch): only
// below 384 64 x 64 tiles, aiming at ~768 workgroups -- widening either (below 768 tiles / 1024-2048 workgroups) measured
// equal or 5-15 % slower at the layer3 / layer4 shapes (profiles/r05_conv_bn.md).  1 = no split.
inline int ksplit_rule(long tiles64, int steps) {
  if (tiles64 >= 384) return 1;
  int k = (int)(768 / tiles64);                 // aim at ~3 workgroups per CU
  if (k > 8) k = 8;
  if (k > steps / 4) k = steps / 4;             // at least 4 K steps per part
  return k < 2 ? 1 : k;
}

}  // namespace
