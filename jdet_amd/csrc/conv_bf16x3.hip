// 3x3 / stride 1 / pad 1 channels-last forward convolution, fp32 in and out, on the bf16 matrix pipe through an exact
// three-way split of every fp32 operand (include/jdet_hip.h).  The same implicit GEMM as conv_igemm.hip
//   Y[m, n] = sum_{tap, c} X[pixel(m) + tap, c] * Wt[n, (tap, c)]          m = (image, y, x), n = output channel
// for the big dense 256 -> 256 layers that sit at the fp32 MFMA's limit there (v_mfma_f32_32x32x2_f32: 64 cycles for 4 096
// FLOP; v_mfma_f32_32x32x16_bf16: 32 cycles for 32 768).
//
// Numerics.  Split by truncation on the fp32 bits:
//   a1 = bits(x) & 0xFFFF0000,  r = x - a1,  a2 = bits(r) & 0xFFFF0000,  a3 = r - a2
// Both subtractions are exact, a1 + a2 + a3 == x exactly, every part is a bf16 value with the sign of x (or zero):
// 8 + 8 + 8 mantissa bits.  (Truncation, not v_cvt_pk_bf16_f32: rounding can flip the sign of the remainder and costs
// the exactness argument.)  Six products per operand pair go into ONE fp32 accumulator per output, small terms first
// within a 16-deep K block:  a3b1, a1b3, a2b2, a2b1, a1b2, a1b1.  Every bf16 x bf16 product is exact in fp32; the dropped
// terms a2b3, a3b2, a3b3 are <= 1.2e-7 |a b|, about one fp32 rounding per product.  Emulated on the CPU at K = 2304
// against float64 the six-term form errs 5.9e-6 (post-ReLU inputs) / 7.5e-6 (signed) where an fp32 fma chain errs
// 5.4e-6 / 9.3e-6 (profiles/conv_bf16x3.md); with fewer terms it is 4-10 x worse, so all six stay.
// Non-finite inputs give non-finite outputs, but not always the same ones as the fp32 kernel: x = Inf splits into
// (Inf, NaN, NaN), so an output the fp32 kernel reports as Inf comes out NaN here.
//
// Tiling (one workgroup = 4 waves as 2 x 2, 128 x 128 outputs, K step = 16 channels of one tap):
//   * a wave owns 64 x 64 outputs = 2 x 2 tiles of 32 x 32 (64 accumulator registers) and issues 2 * 2 * 6 = 24 MFMAs per
//     K step.  Lane l of v_mfma_f32_32x32x16_bf16 holds row / column l & 31 and the 8 values k = 8 (l >> 5) .. + 7 of both
//     operands; which channels those are is free as long as A and B agree.
//   * LDS holds, per buffer, three bf16 planes of each operand tile as [row][2 halves of 8 bf16 = 16 bytes]; half h of row
//     r is stored at position h ^ ((r >> 3) & 1), which spreads the 16-byte fragment reads of 8 rows x 1 half over all
//     banks.  2 buffers x 2 operands x 3 planes x 4 KB = 48 KB.  One ds_read_b128 per fragment: 12 per 24 MFMAs.
//   * the loader: thread t takes row t >> 1 and half t & 1 of both tiles = channel chunks (4 floats) h and h + 2 of the K
//     step, as two raw buffer loads each (a lane pair covers 32 contiguous bytes per load), two K steps = one 128-byte
//     line per row at a time; rows outside the image / past Cout carry an out-of-range offset and read as zeros, as in
//     conv_igemm.hip.  The split runs between the loads and the
//     LDS stores: 2 ands, 2 subtractions per value and 3 byte permutes per value pair, then three ds_write_b128 per tile.
//   * double-buffered LDS, the operand chunks requested two to three K steps ahead into two register sets, the split of
//     step s + 1 scheduled between the MFMAs of step s, one barrier per K step; XCD-aware tile order; the epilogue (+ bias, ReLU,
//     x row mask) is conv_igemm.hip's, statement for statement.
#include "conv_mfma.h"
#include "jdet_hip.h"

namespace {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

struct SplitConvArgs {
  const float* x;        // (N, H, W, Cin)
  const float* w;        // (Cout, 3, 3, Cin)
  const float* bias;     // (Cout) or null
  const float* rowmask;  // (N*H*W) or null: multiplies the finished row (after bias / ReLU)
  float* y;              // (N, H, W, Cout)
  int N, H, W, Cin, Cout, relu;
};

constexpr int kBT = 128, kBK = 16;
constexpr int kPlane = kBT * kBK * 2;       // bytes of one bf16 plane of one operand tile
constexpr int kOperand = 3 * kPlane;
constexpr int kBuffer = 2 * kOperand;       // [A: 3 planes | B: 3 planes]

// byte position of half `half` (8 bf16) of row `row` inside a plane
__device__ __forceinline__ int plane_bytes(int row, int half) { return row * 32 + ((half ^ ((row >> 3) & 1)) << 4); }

// the high halves of two dwords as one: (hi & 0xFFFF0000) | (lo >> 16)
__device__ __forceinline__ unsigned pack_hi(unsigned hi, unsigned lo) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// eight fp32 values -> their three bf16 planes, value k in bf16 slot k of each
__device__ __forceinline__ void split8(const v4f& lo, const v4f& hi, v4u& p1, v4u& p2, v4u& p3) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float x0 = k < 2 ? lo[2 * k] : hi[2 * k - 4], x1 = k < 2 ? lo[2 * k + 1] : hi[2 * k - 3];
    const unsigned b0 = __builtin_bit_cast(unsigned, x0), b1 = __builtin_bit_cast(unsigned, x1);
    p1[k] = pack_hi(b1, b0);
    const float r0 = x0 - __builtin_bit_cast(float, b0 & 0xFFFF0000u);
    const float r1 = x1 - __builtin_bit_cast(float, b1 & 0xFFFF0000u);
    const unsigned c0 = __builtin_bit_cast(unsigned, r0), c1 = __builtin_bit_cast(unsigned, r1);
    p2[k] = pack_hi(c1, c0);
    const float t0 = r0 - __builtin_bit_cast(float, c0 & 0xFFFF0000u);
    const float t1 = r1 - __builtin_bit_cast(float, c1 & 0xFFFF0000u);
    p3[k] = pack_hi(__builtin_bit_cast(unsigned, t1), __builtin_bit_cast(unsigned, t0));
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void conv3x3_bf16x3_kernel(SplitConvArgs a) {
  constexpr int T = 2;
  __shared__ __attribute__((aligned(16))) char s_raw[2 * kBuffer];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long M = (long)a.N * a.H * a.W;
  const int NT = (a.Cout + kBT - 1) / kBT;
  const int logical = xcd_logical();
  // (32-bit unsigned index arithmetic in the prologue -- the host refuses positions * channels >= 2^30; see conv_mfma.h)
  const int mtile = (int)((unsigned)logical / (unsigned)NT);
  const long m0 = (long)mtile * kBT;
  const int n0 = (logical - mtile * NT) * kBT;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)(M * a.Cin * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, (unsigned)((long)a.Cout * 9 * a.Cin * 4), 0x00020000);
  // ---- loader role: row tid / 2, half tid % 2 = channel chunks h and h + 2 of the K step, of both tiles ----
  const int lrow = tid >> 1, lhalf = tid & 1;
  bool m_ok;
  int img, py, px;
  row_pixel(m0 + lrow, M, a.H, a.W, 1, m_ok, img, py, px);
  // byte offset of this thread's first weight chunk at (tap 0, channel 0)
  const unsigned wv = n0 + lrow < a.Cout ? ((unsigned)((n0 + lrow) * 9 * a.Cin + lhalf * 4)) * 4u : kOob;
  const int st_off = plane_bytes(lrow, lhalf);
  const int nsteps = 9 * (a.Cin / kBK);

  unsigned av = kOob;                    // byte offset of the tap's source pixel, or kOob
  auto set_tap = [&](int tap) {
    const int r = (tap * 11) >> 5, s = tap - r * 3;      // tap / 3 for tap < 9
    const int yy = py + r - 1, xx = px + s - 1;
    const bool in = m_ok && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
    const unsigned off = ((unsigned)(((img * a.H + yy) * a.W + xx) * a.Cin + lhalf * 4)) * 4u;
    av = in ? off : kOob;
  };
  // Two register sets, each the chunks of TWO K steps (32 channels = one 128-byte line per row and operand: requested 16
  // channels at a time, each line would be fetched from L2 twice).  Load j of a set takes chunk 2 j + h: loads 0, 1 are
  // the first K step, loads 2, 3 the second.
  v4f ra[2][4], rb[2][4];
  auto load_set = [&](auto setc, int tap, int c) {     // c: first channel of the step pair
    constexpr int S = decltype(setc)::value;
    const unsigned sa = (unsigned)(c * 4), sb = (unsigned)((tap * a.Cin + c) * 4);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      ra[S][j] = buf_load(rx, av, sa + 32u * j);
      rb[S][j] = buf_load(rw, wv, sb + 32u * j);
    }
  };
  auto store_half = [&](auto setc, auto halfc, int buf) {     // split K step `half` of the set into LDS buffer buf
    constexpr int S = decltype(setc)::value, J = 2 * decltype(halfc)::value;
    char* const dst = s_raw + buf * kBuffer + st_off;
    v4u p1, p2, p3;
    split8(ra[S][J], ra[S][J + 1], p1, p2, p3);
    *reinterpret_cast<v4u*>(dst) = p1;
    *reinterpret_cast<v4u*>(dst + kPlane) = p2;
    *reinterpret_cast<v4u*>(dst + 2 * kPlane) = p3;
    split8(rb[S][J], rb[S][J + 1], p1, p2, p3);
    *reinterpret_cast<v4u*>(dst + kOperand) = p1;
    *reinterpret_cast<v4u*>(dst + kOperand + kPlane) = p2;
    *reinterpret_cast<v4u*>(dst + kOperand + 2 * kPlane) = p3;
  };

  // ---- compute role: wave (wm, wn) owns outputs [wm*64, +64) x [wn*64, +64) ----
  const int wm = (wave >> 1) & 1, wn = wave & 1;
  const int fa_off = plane_bytes(wm * (kBT / 2) + (lane & 31), lane >> 5);      // (tile 0, plane 0, buffer 0)
  const int fb_off = kOperand + plane_bytes(wn * (kBT / 2) + (lane & 31), lane >> 5);
  v16f acc[T][T];
#pragma unroll
  for (int i = 0; i < T; i++)
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;
  auto mfma_step = [&](int buf) {
    const char* sb = s_raw + buf * kBuffer;
    v8bf fa[T][3], fb[T][3];
#pragma unroll
    for (int i = 0; i < T; i++)          // tile i: 32 rows further = the same swizzle
#pragma unroll
      for (int p = 0; p < 3; p++) {
        fa[i][p] = *reinterpret_cast<const v8bf*>(sb + fa_off + p * kPlane + i * 32 * 32);
        fb[i][p] = *reinterpret_cast<const v8bf*>(sb + fb_off + p * kPlane + i * 32 * 32);
      }
    // the six terms, small first: a3b1, a1b3, a2b2, a2b1, a1b2, a1b1
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int t = 0; t < 6; t++)
#pragma unroll
      for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[t]], fb[j][PB[t]], acc[i][j], 0, 0, 0);
  };

  // ---- K pipeline over pairs of K steps.  Pair d lives in register set d & 1; entering pair d, LDS buffer 0 holds its
  // first step and set (d + 1) & 1 holds pair d + 1 (requested one pair ago).  Step 2d: MFMAs out of buffer 0 while the
  // pair's second step is split into buffer 1; step 2d + 1: pair d + 2 is requested into the set just used up, MFMAs out
  // of buffer 1 while the FIRST step of pair d + 1 is split into buffer 0 -- every chunk is split at least two K steps
  // after its request, and the split's VALU work sits between the step's MFMAs (sched_group_barrier) instead of behind
  // them.  The requests are unconditional (a conditional one makes the compiler wait for every load in flight): past
  // the last pair the cursor stays on the last tap and the loads re-read it, in bounds, for nobody
  // (the scalar offset of a raw buffer load is not range-checked: the cursor must never leave the tensors).
  int tap = 0, c = 0;
  auto advance = [&]() {          // the load cursor: next 32 channels, then the next tap; branch-free
    c += 2 * kBK;
    const bool wrap = c == a.Cin;
    c = wrap ? 0 : c;
    tap = wrap && tap < 8 ? tap + 1 : tap;
    set_tap(tap);
  };
  // one MFMA, then a share of the split, 24 times: 16 values x 5.5 VALU operations = 88 over the step's 24 MFMAs
  auto interleave = [&]() {
#pragma unroll
    for (int k = 0; k < 24; k++) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
    }
  };
  using Half0 = std::integral_constant<int, 0>;
  using Half1 = std::integral_constant<int, 1>;
  auto pair_steps = [&](auto cur, auto nxt) {
    mfma_step(0);
    store_half(cur, Half1{}, 1);     // the other buffer: its last readers passed the previous barrier
    interleave();
    __syncthreads();
    advance();
    load_set(cur, tap, c);           // pair d + 2
    mfma_step(1);
    store_half(nxt, Half0{}, 0);     // (after the last pair: the re-read tap, for nobody)
    interleave();
    __syncthreads();
  };
  const int npairs = nsteps / 2;     // 9 * Cin / 32 (the host takes Cin % 32 == 0 only)
  set_tap(0);
  load_set(Set0{}, tap, c);
  advance();
  load_set(Set1{}, tap, c);
  store_half(Set0{}, Half0{}, 0);
  __syncthreads();
  for (int d = 0; d + 1 < npairs; d += 2) {      // straight-line body: the waits count the loads in flight exactly
    pair_steps(Set0{}, Set1{});
    pair_steps(Set1{}, Set0{});
  }
  if (npairs & 1) pair_steps(Set0{}, Set1{});

  // ---- epilogue (conv_igemm.hip's): C/D layout of the 32x32 MFMA: column = lane & 31, row = cd_row(reg) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < T; i++) {
    float mk[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const long m = m0 + wm * (kBT / 2) + i * 32 + cd_row(e) + 4 * (lane >> 5);
      mk[e] = (a.rowmask && m < M) ? a.rowmask[m] : 1.f;       // all 16 loads in flight together
    }
#pragma unroll
    for (int j = 0; j < T; j++) {
      const int n = n0 + wn * (kBT / 2) + j * 32 + (lane & 31);
      const float b = (a.bias && n < a.Cout) ? a.bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const long m = m0 + wm * (kBT / 2) + i * 32 + cd_row(e) + 4 * (lane >> 5);
        if (m < M && n < a.Cout) {
          float v = acc[i][j][e];
          v += b;
          if (a.relu) v = fmaxf(v, 0.f);
          if (a.rowmask) v *= mk[e];
          a.y[(size_t)m * a.Cout + n] = v;
        }
      }
    }
  }
}

}  // namespace

JDET_API int jdet_conv3x3_bf16x3_supported(int Cin, int Cout) { return Cin > 0 && Cin % 32 == 0 && Cout > 0; }

JDET_API int jdet_conv3x3_bf16x3_forward(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout,
                                         const float* bias, int relu, const float* rowmask, float* y_nhwc,
                                         jdet_stream_t stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return JDET_E_BADARG;
  if (!jdet_conv3x3_bf16x3_supported(Cin, Cout)) return JDET_E_UNSUPPORTED;
  if (N == 0) return JDET_OK;
  if (!x_nhwc || !w_krsc || !y_nhwc) return JDET_E_BADARG;
  if ((((uintptr_t)x_nhwc) | ((uintptr_t)w_krsc)) & 15) return JDET_E_BADARG;
  if (((uintptr_t)y_nhwc) & 3) return JDET_E_BADARG;
  const long M = (long)N * H * W;
  if (M * (Cin > Cout ? Cin : Cout) >= (1L << 30)) return JDET_E_UNSUPPORTED;     // 32-bit byte offsets
  if ((long)Cout * 9 * Cin >= (1L << 30)) return JDET_E_UNSUPPORTED;
  SplitConvArgs a{x_nhwc, w_krsc, bias, rowmask, y_nhwc, N, H, W, Cin, Cout, relu ? 1 : 0};
  const long tiles = ((M + kBT - 1) / kBT) * ((Cout + kBT - 1) / kBT);
  hipLaunchKernelGGL(conv3x3_bf16x3_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, a);
  return jdet_launch_status();
}
