// The kernel of the conv_bn family (see conv_bn.hip for what it computes and why): a header so that the product library
// (conv_bn.hip: STAMPS = false only) and the profiling build outside it (experimental/conv_bn_stamps.hip) compile the same
// text.  The tile loop is conv_mfma.h / conv_mfma_loop.inc, shared with conv_igemm.hip; what is this kernel's own is the
// run-time (R, stride) tap geometry, the neighbour-tile prefetch, the three epilogue modes and the column sums.
#pragma once
#include "conv_mfma.h"

namespace {

struct CbArgs {
  const float* x;        // (N, H, W, Cin)
  const float* w;        // (Cout, R, R, Cin)
  float* y;              // (N, Ho, Wo, Cout)
  float* partial;        // cross-workgroup K split: (ksplit, M, Cout) partial sums (no epilogue), else null
  jdet_conv_epilogue_t ep;
  int N, H, W, Cin, Cout, R, stride, Ho, Wo, ksplit;
};

// The argument checks of the entry points (jdet_conv_bn_forward and the stamps build), in one place: fills `a` for an
// unsplit launch (no partial planes).  JDET_OK with N == 0 means "nothing to do".
inline int cb_check_args(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout, int R,
                         int stride, const jdet_conv_epilogue_t* epilogue, float* y_nhwc, CbArgs& a) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !epilogue) return JDET_E_BADARG;
  if (!jdet_conv_bn_supported(Cin, Cout, R, stride)) return JDET_E_UNSUPPORTED;
  if (N == 0) return JDET_OK;
  if (!x_nhwc || !w_krsc || !y_nhwc) return JDET_E_BADARG;
  if ((((uintptr_t)x_nhwc) | ((uintptr_t)w_krsc)) & 15) return JDET_E_BADARG;
  const jdet_conv_epilogue_t& ep = *epilogue;
  if (ep.mode != JDET_EPI_FORWARD && ep.mode != JDET_EPI_ADD && ep.mode != JDET_EPI_MASK) return JDET_E_BADARG;
  if (ep.mode == JDET_EPI_ADD && (!ep.grad_out || !ep.act)) return JDET_E_BADARG;
  if (ep.mode == JDET_EPI_MASK && !ep.act) return JDET_E_BADARG;
  if (ep.bn.var && !ep.bn.mean) return JDET_E_BADARG;
  const int Ho = out_dim(H, R, stride), Wo = out_dim(W, R, stride);
  const long M = (long)N * Ho * Wo, Min = (long)N * H * W;
  if (Min * Cin >= (1L << 30) || M * Cout >= (1L << 30) || (long)Cout * R * R * Cin >= (1L << 30))
    return JDET_E_UNSUPPORTED;     // 32-bit byte offsets
  a = CbArgs{x_nhwc, w_krsc, y_nhwc, nullptr, ep, N, H, W, Cin, Cout, R, stride, Ho, Wo, 1};
  return JDET_OK;
}

// a = gamma * rsqrt(var + eps), sh = beta - mean * a (frozen_bn.hip's affine4, the same operation order); without
// statistics (var == null) the map is a = gamma (1), sh = beta (0): a plain bias
__device__ __forceinline__ void bn_affine(const jdet_bn_params_t& p, int n, float& a, float& sh) {
  const float w = p.weight ? p.weight[n] : 1.f, b = p.bias ? p.bias[n] : 0.f;
  if (p.var) {
    const float is = 1.0f / sqrtf(p.var[n] + p.eps);
    a = w * is;
    sh = b - p.mean[n] * (w * is);
  } else {
    a = w;
    sh = b;
  }
}

// DEPTH: operand tiles requested this many K steps ahead (conv_mfma_loop.inc); conv_bn.hip launches 2 for BT = 64, 1 for
// BT = 128.  STAMPS: a profiling build (csrc/experimental/conv_bn_stamps.hip, scripts/r6_conv_stamps.py) -- every workgroup
// writes time stamps and its placement over the first 16 words of its tile's first output row.
template <int BT, int BK, int KG, int DEPTH, bool STAMPS = false>
__global__ __launch_bounds__(256 * KG)
__attribute__((amdgpu_waves_per_eu(BT == 128 ? (KG == 2 ? 4 : (BK == 32 ? 2 : 4)) : 4)))
void conv_bn_kernel(CbArgs a) {
  using TL = MfmaTile<BT, BK, KG>;
  constexpr int T = TL::T, CH = TL::CH, RPP = TL::RPP, PASSES = TL::PASSES, TILE = TL::TILE, QN = TL::QN;
  __shared__ __attribute__((aligned(16))) char s_raw[4 * TILE];     // [buffer][A | B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // STAMPS: start, K loop entered / left, end, placement -- written over the first words of the tile's first output row
  // (that row is garbage afterwards)
  long long stamp[4] = {0, 0, 0, 0}, stamp_x[3] = {0, 0, 0};     // _x: requests issued | first tile landed | epilogue operands read
  if constexpr (STAMPS) stamp[0] = wall_clock64();
  const long M = (long)a.N * a.Ho * a.Wo;
  const long Min = (long)a.N * a.H * a.W;
  const int taps = a.R * a.R, pad = a.R >> 1;
  const int NT = (a.Cout + BT - 1) / BT;
  const int logical = xcd_logical();
  const int mtile = (int)((unsigned)logical / (unsigned)NT);
  const long m0 = (long)mtile * BT;
  const int n0 = (logical - mtile * NT) * BT;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)(Min * a.Cin * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, (unsigned)((long)a.Cout * taps * a.Cin * 4), 0x00020000);
  // ---- loader role: pass p covers row p * RPP + tid / CH, chunk tid % CH (4 channels of the BK of a K step) ----
  const int lchunk = tid % CH, lrow = tid / CH;
  int img[PASSES], py[PASSES], px[PASSES];   // image, and the input pixel of tap (0, 0) WITHOUT the padding shift
  bool m_ok[PASSES];
  unsigned wv[PASSES];
  int st_off[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; p++) {
    const int row = p * RPP + lrow;
    row_pixel(m0 + row, M, a.Ho, a.Wo, a.stride, m_ok[p], img[p], py[p], px[p]);
    wv[p] = n0 + row < a.Cout ? ((unsigned)((n0 + row) * taps * a.Cin + lchunk * 4)) * 4u : kOob;
    st_off[p] = swz_bytes<BK>(row, lchunk);
  }
  const int spt = a.Cin / BK;               // K steps per tap (host: BK = 32 only when Cin % 32 == 0)
  const int all_steps = taps * spt;
  const int step0 = (int)((unsigned)all_steps * blockIdx.y / (unsigned)a.ksplit);
  const int nsteps = (int)((unsigned)all_steps * (blockIdx.y + 1u) / (unsigned)a.ksplit) - step0;

  unsigned av[PASSES];
  auto set_tap = [&](int tap) {
    // branch-free (round 6: the predicated form was eight exec-mask branches per call, inside the K loop at every tap change;
    // R is 1 or 3: tap / R = (tap * 11) >> 5 for tap < 9)
    const int r = a.R == 1 ? tap : (tap * 11) >> 5, s = tap - r * a.R;
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      const int yy = py[p] + r - pad, xx = px[p] + s - pad;
      const bool in = m_ok[p] && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      const unsigned off = ((unsigned)(((img[p] * a.H + yy) * a.W + xx) * a.Cin + lchunk * 4)) * 4u;
      av[p] = in ? off : kOob;
    }
  };
  constexpr int SETS = DEPTH;
  v4f ra[SETS][PASSES], rb[SETS][PASSES];
  auto load_set = [&](auto setc, int tap, int c) {
    constexpr int S = decltype(setc)::value;
    const unsigned sa = (unsigned)(c * 4), sb = (unsigned)((tap * a.Cin + c) * 4);
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      ra[S][p] = buf_load(rx, av[p], sa);
      rb[S][p] = buf_load(rw, wv[p], sb);
    }
  };
  auto store_set = [&](auto setc, int buf) {
    constexpr int S = decltype(setc)::value;
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      *reinterpret_cast<v4f*>(s_raw + buf * 2 * TILE + st_off[p]) = ra[S][p];
      *reinterpret_cast<v4f*>(s_raw + buf * 2 * TILE + TILE + st_off[p]) = rb[S][p];
    }
  };
  // (the one-set forms conv_mfma_loop.inc calls at DEPTH = 1)
  auto load_step = [&](int tap, int c) { load_set(Set0{}, tap, c); };
  auto store_step = [&](int buf) { store_set(Set0{}, buf); };

  // ---- compute role ----
  const int kg = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;
  const int frow = lane & 31, fhalf = lane >> 5;
  int fa_off[QN], fb_off[QN];
#pragma unroll
  for (int qq = 0; qq < QN; qq++) {
    const int chunk = (qq * KG + kg) * 2 + fhalf;
    fa_off[qq] = swz_bytes<BK>(wm * (BT / 2) + frow, chunk);
    fb_off[qq] = TILE + swz_bytes<BK>(wn * (BT / 2) + frow, chunk);
  }
  v16f acc[T][T];
#pragma unroll
  for (int i = 0; i < T; i++)
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

  // ---- the neighbour tile(s) of the epilogue (residual | grad_out + act | act): with one 32 x 32 tile per wave (BT = 64)
  // they are requested HERE, ahead of the K loop -- the 1x1 layers of the big maps run two to eight K steps, and a
  // tile fetched only after them costs as much again as the loop (64 -> 256 channels at 2 x 256^2 with a residual:
  // 133 us against 80 us without one, profiles/r05_conv_bn.md)
  const jdet_conv_epilogue_t& ep = a.ep;
  const int mode = ep.mode;
  const float* p0 = mode == JDET_EPI_FORWARD ? ep.residual : (mode == JDET_EPI_ADD ? ep.grad_out : ep.act);
  const float* p1 = mode == JDET_EPI_ADD ? ep.act : nullptr;
  constexpr bool PRE = T == 1;
  float pre0[PRE ? 16 : 1], pre1[PRE ? 16 : 1];
  // Round 6 (workgroup time stamps, scripts/r6_conv_stamps.py): ~900 instructions ran between a workgroup's start and its
  // first operand request -- 6-8 us with sixteen waves per CU issuing them at once -- most of them this block's 32 predicated
  // loads with 64-bit addresses.  A tile that lies inside the map (every tile but the last of a ragged M) now takes raw buffer
  // loads: one 32-bit lane offset, the 16 row offsets in SGPRs, one lane predicate (the column) around the lot.
  const bool full_tile = !a.partial && m0 + BT <= M;        // uniform
  const unsigned ybytes = (unsigned)(M * a.Cout * 4);         // (host: M * Cout < 2^30)
  if (PRE && full_tile && kg == 0) {
    const int n = n0 + wn * (BT / 2) + (lane & 31);
    const unsigned base = ((unsigned)(m0 + wm * (BT / 2) + 4 * (lane >> 5)) * (unsigned)a.Cout + (unsigned)n) * 4u;
#pragma unroll
    for (int e = 0; e < 16; e++) pre0[e] = pre1[e] = 0.f;
    if (n < a.Cout) {
      if (p0) {
        const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)p0, 0, ybytes, 0x00020000);
#pragma unroll
        for (int e = 0; e < 16; e++)
          pre0[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                  r0, base, (unsigned)(cd_row(e) * a.Cout * 4), 0));
      }
      if (p1) {
        const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)p1, 0, ybytes, 0x00020000);
#pragma unroll
        for (int e = 0; e < 16; e++)
          pre1[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                  r1, base, (unsigned)(cd_row(e) * a.Cout * 4), 0));
      }
    }
  } else if (PRE && !a.partial && kg == 0) {
    const long mrow = m0 + wm * (BT / 2) + 4 * (lane >> 5);
    const int n = n0 + wn * (BT / 2) + (lane & 31);
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const long m = mrow + (e & 3) + 8 * (e >> 2);
      const bool ok = n < a.Cout && m < M;
      pre0[e] = (p0 && ok) ? p0[(size_t)m * a.Cout + n] : 0.f;
      pre1[e] = (p1 && ok) ? p1[(size_t)m * a.Cout + n] : 0.f;
    }
  }

  int tap = step0 / spt, c = (step0 - tap * spt) * BK;
  set_tap(tap);
  auto advance = [&]() {          // the load cursor: next K step (next 32 / 16 channels, then the next tap)
    c += BK;
    if (c == a.Cin) {
      c = 0;
      tap++;
      set_tap(tap);
    }
  };
  auto mfma_step = [&](int buf) { ::mfma_step<BT, BK, KG>(s_raw, buf, fa_off, fb_off, acc); };
  if constexpr (STAMPS) stamp_x[0] = wall_clock64();              // index arithmetic done
#define CONV_MFMA_AFTER_REQUESTS                                                                         \
  if constexpr (STAMPS) {                                                                                \
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); /* (set 0 = the four oldest of eight loads) */      \
    asm volatile("" : "+v"(ra[0][0]), "+v"(rb[0][0]));                                                   \
    stamp_x[1] = wall_clock64(); /* first tile in registers */                                           \
  }
#define CONV_MFMA_AFTER_FIRST_TILE \
  if constexpr (STAMPS) stamp[1] = wall_clock64();
#include "conv_mfma_loop.inc"
#undef CONV_MFMA_AFTER_REQUESTS
#undef CONV_MFMA_AFTER_FIRST_TILE

  if constexpr (STAMPS) {
    asm volatile("" : "+v"(acc[0][0]));          // (the stamp stays behind the last MFMA's result)
    stamp[2] = wall_clock64();
  }
  if (KG == 2) {
    float* red = reinterpret_cast<float*>(s_raw);
    if (kg == 1) {
#pragma unroll
      for (int i = 0; i < T; i++)
#pragma unroll
        for (int j = 0; j < T; j++)
#pragma unroll
          for (int e = 0; e < 16; e++) red[red_index<T>(wave, lane, i, j, e)] = acc[i][j][e];
    }
    __syncthreads();
    if (kg == 1) return;
  }

  // ---- epilogue.  C/D layout of the 32x32 MFMA: column = lane & 31, row = cd_row(reg) + 4 * (lane >> 5).
  // The neighbour tiles (residual | grad_out + act_out | act) are fetched 8 rows at a time BEFORE the stores of those
  // rows: the loads are in flight together instead of one per dependent store.
  float cs1[T], cs2[T];
#pragma unroll
  for (int j = 0; j < T; j++) cs1[j] = cs2[j] = 0.f;
  bool stored = false;
  if constexpr (T == 1) {
    if (a.partial && m0 + BT <= M) {          // K split over workgroups: the plain sums to this part's plane, same store form
      stored = true;
      const int n = n0 + wn * (BT / 2) + (lane & 31);
      if (n < a.Cout) {
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.partial + (size_t)blockIdx.y * M * a.Cout), 0, ybytes, 0x00020000);
        const unsigned base = ((unsigned)(m0 + wm * (BT / 2) + 4 * (lane >> 5)) * (unsigned)a.Cout + (unsigned)n) * 4u;
        const float* red = reinterpret_cast<const float*>(s_raw) + (size_t)(wave & 3) * 16 * 64 + lane;
#pragma unroll
        for (int e = 0; e < 16; e++) {
          float v = acc[0][0][e];
          if (KG == 2) v += red[e * 64];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rp, base,
                                                (unsigned)(cd_row(e) * a.Cout * 4), 0);
        }
      }
    }
    // a tile inside the map (round 6): the 16 rows leave by raw buffer stores -- one 32-bit lane offset, the row offsets in
    // SGPRs, the mode decided once -- instead of 16 predicated stores with 64-bit addresses.  Same operations on the same
    // values in the same order as the general path below.
    if (full_tile) {
      stored = true;
      const int n = n0 + wn * (BT / 2) + (lane & 31);
      const bool nok = n < a.Cout;
      float sa = 1.f, sh = 0.f, beta = 0.f;
      if (nok && (mode != JDET_EPI_ADD)) {
        // (measured: read and folded ahead of the K loop instead, riding in pre1 -- 1.3-2.2 us leave the epilogue, 0.6-1.8 us
        //  join the prologue: no gain; requested behind the first barrier and folded here -- epilogue 6.5 -> 5.6 us, nothing
        //  on the layer sums or the step, and the kernel at 128 VGPRs: not kept either)
        bn_affine(ep.bn, n, sa, sh);
        beta = ep.bn.bias ? ep.bn.bias[n] : 0.f;
      }
      if constexpr (STAMPS) {
        asm volatile("" : "+v"(sa), "+v"(sh));
        stamp_x[2] = wall_clock64();
      }
      if (nok) {
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, ybytes, 0x00020000);
        const unsigned base = ((unsigned)(m0 + wm * (BT / 2) + 4 * (lane >> 5)) * (unsigned)a.Cout + (unsigned)n) * 4u;
        const float* red = reinterpret_cast<const float*>(s_raw) + (size_t)(wave & 3) * 16 * 64 + lane;
        auto rows = [&](auto modec) {
          constexpr int MODE = decltype(modec)::value;
          float c1 = 0.f, c2 = 0.f;
#pragma unroll
          for (int e = 0; e < 16; e++) {
            float v = acc[0][0][e];
            if (KG == 2) v += red[e * 64];
            if constexpr (MODE == JDET_EPI_FORWARD) {
              if (ep.affine) v = v * sa + sh;
              v += pre0[e];                          // residual (0 without one)
              if (ep.relu) v = fmaxf(v, 0.f);
            } else if constexpr (MODE == JDET_EPI_ADD) {
              v += pre1[e] > 0.f ? pre0[e] : 0.f;
            } else {
              v = pre0[e] > 0.f ? v : 0.f;
              c1 += v;
              c2 += v * (pre0[e] - beta);
              v *= sa;
            }
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, base,
                                                  (unsigned)(cd_row(e) * a.Cout * 4), 0);
          }
          cs1[0] = c1;
          cs2[0] = c2;
        };
        if (mode == JDET_EPI_FORWARD) rows(std::integral_constant<int, JDET_EPI_FORWARD>{});
        else if (mode == JDET_EPI_ADD) rows(std::integral_constant<int, JDET_EPI_ADD>{});
        else rows(std::integral_constant<int, JDET_EPI_MASK>{});
      }
    }
  }
  if (!stored)
#pragma unroll
  for (int i = 0; i < T; i++) {
    const long mrow = m0 + wm * (BT / 2) + i * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < T; j++) {
      const int n = n0 + wn * (BT / 2) + j * 32 + (lane & 31);
      const bool nok = n < a.Cout;
      float sa = 1.f, sh = 0.f, beta = 0.f;
      if (nok && !a.partial && (mode != JDET_EPI_ADD)) {
        bn_affine(ep.bn, n, sa, sh);
        beta = ep.bn.bias ? ep.bn.bias[n] : 0.f;
      }
      if constexpr (STAMPS) {
        asm volatile("" : "+v"(sa), "+v"(sh));
        stamp_x[2] = wall_clock64();                               // the column's BatchNorm parameters read and folded
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {          // 8 rows at a time: their neighbour loads are in flight together
        float t0[8], t1[8];
        if (PRE) {
#pragma unroll
          for (int u = 0; u < 8; u++) {
            t0[u] = pre0[h * 8 + u];
            t1[u] = pre1[h * 8 + u];
          }
        } else if (!a.partial) {
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int e = h * 8 + u;
            const long m = mrow + (e & 3) + 8 * (e >> 2);
            const bool ok = nok && m < M;
            t0[u] = (p0 && ok) ? p0[(size_t)m * a.Cout + n] : 0.f;
            t1[u] = (p1 && ok) ? p1[(size_t)m * a.Cout + n] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int e = h * 8 + u;
          const long m = mrow + (e & 3) + 8 * (e >> 2);
          if (m < M && nok) {
            float v = acc[i][j][e];
            if (KG == 2)
              v += reinterpret_cast<const float*>(s_raw)[red_index<T>(wave, lane, i, j, e)];
            if (a.partial) {
              a.partial[((size_t)blockIdx.y * M + m) * a.Cout + n] = v;
              continue;
            }
            if (mode == JDET_EPI_FORWARD) {
              if (ep.affine) v = v * sa + sh;
              v += t0[u];                          // residual (0 without one)
              if (ep.relu) v = fmaxf(v, 0.f);
            } else if (mode == JDET_EPI_ADD) {
              v += t1[u] > 0.f ? t0[u] : 0.f;
            } else {
              v = t0[u] > 0.f ? v : 0.f;
              cs1[j] += v;
              cs2[j] += v * (t0[u] - beta);
              v *= sa;
            }
            a.y[(size_t)m * a.Cout + n] = v;
          }
        }
      }
    }
  }
  if (mode == JDET_EPI_MASK && ep.sums && !a.partial) {
    // the two half waves hold the same columns (rows 4 apart): combine, then one partial row per (M tile, wave row)
#pragma unroll
    for (int j = 0; j < T; j++) {
      const float s1 = cs1[j] + __shfl_xor(cs1[j], 32);
      const float s2 = cs2[j] + __shfl_xor(cs2[j], 32);
      const int n = n0 + wn * (BT / 2) + j * 32 + (lane & 31);
      if (lane < 32 && n < a.Cout) {
        float* row = ep.sums + (size_t)(mtile * 2 + wm) * 2 * a.Cout;
        row[n] = s1;
        row[a.Cout + n] = s2;
      }
    }
  }
  if constexpr (STAMPS) {
    __syncthreads();
    if (threadIdx.x == 0 && !a.partial && m0 < M && n0 + 16 <= a.Cout) {
      stamp[3] = wall_clock64();
      int* d = reinterpret_cast<int*>(a.y + (size_t)m0 * a.Cout + n0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        d[2 * k] = (int)(stamp[k] & 0xffffffff);
        d[2 * k + 1] = (int)(stamp[k] >> 32);
      }
      d[8] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_ID
      d[9] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // XCC_ID
      d[10] = (int)blockIdx.x;
      d[11] = 0x5741;
      d[12] = (int)(stamp_x[0] - stamp[0]);
      d[13] = (int)(stamp_x[1] - stamp[0]);
      d[14] = (int)(stamp_x[2] - stamp[2]);
      d[15] = 0;
    }
  }
}

}  // namespace
