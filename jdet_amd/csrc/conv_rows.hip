// Row-sparse backward of the 3x3 / stride 1 / pad 1 convolutions of a regression tower, channels-last.
//
// Reference: the gradients Jittor's autograd derives for nn.Conv inside ConvModule (python/jdet/models/utils/modules.py:
// L91-175) in the regression towers of models/roi_heads/s2anet_head.py:L127-205.  Those towers are trained by a smooth-L1
// loss whose weight is zero for every anchor that is not positive (L300-340): the gradient entering a tower is exactly
// zero on almost every position row, and a 3x3 data gradient widens the set of non-zero rows by one pixel only.  The
// dense kernels (the library's data gradient, conv_wgrad.hip) multiply all those zeros; the kernels here take the rows
// that hold anything from a list made on the device:
//
//   jdet_rows_nonzero        one pass over g (P, C): a flag byte per row, the ascending list of flagged rows, the
//                            ascending list of their 3x3 dilation (inside each image), both counts -- all on the device
//   jdet_conv3x3_wgrad_rows  gW[co, tap, ci] += sum_{r in list} g[r, co] * x[nbr(r, tap), ci]
//                            = conv_wgrad.hip's kernel (its LDS layout, fragments and epilogue) with the K index taken
//                            from the list: both operands are K-major rows already, as with the deformable form's
//                            gathered operand
//   jdet_conv3x3_dgrad_rows  gx[r, ci] = sum_{tap, co} g[nbr(r, tap), co] * Wd[ci, tap, co]   for r in the dilated list
//                            = conv_igemm.hip's 64 x 64 tile (conv_mfma.h, conv_mfma_loop.inc) with the 64 rows of an M
//                            tile taken from the list and an epilogue that scatters rows; Wd = the flipped weights of
//                            jdet_conv_dgrad_weights
//
// and, for the FORWARD of a tower whose output only that loss reads (include/jdet_hip.h; in training the ODM
// regression tower, whose prediction bbox_decode / AlignConv do not read):
//
//   jdet_rows_from_flags       a flag byte per position -> the ascending lists of the flagged rows, of their 3x3 dilation
//                              and of the dilation of that, with their counts (the dilation / list launches above, twice)
//   jdet_conv3x3_rows_forward  y[r] = [relu](sum_tap x[nbr(r, tap)] . w[tap] + bias) * rowmask[r] for r in a list
//                              = the data gradient's tile with conv_igemm.hip's epilogue, on the (Cout, 3, 3, Cin) weights
//
// Nothing is read back to the host and no launch shape depends on device data: the grids are fixed by CAPACITY (all P
// rows), the counts are read by the kernels, and workgroups past a count leave at once.  A fully dense gradient is
// computed correctly, only slower than by the dense kernels.  List entries past a count are -1 and never read.
// Results equal the dense computation with the exact zeros left out of the sums.
#include "conv_mfma.h"
#include "jdet_hip.h"

namespace {

constexpr int kBlk = 256;        // rows per workgroup of the count / list launches
constexpr int kFlagRows = 64;    // rows per workgroup of the flag pass (one wave per row, 16 rows per wave)

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// ---- jdet_rows_nonzero, launch 1: flags[p] = any element of row p has (bits & 0x7fffffff) != 0 ----
__global__ __launch_bounds__(256) void rows_flag_kernel(const float* __restrict__ g, long P, int C4,
                                                        uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long base = (long)blockIdx.x * kFlagRows + wave * (kFlagRows / 4);
  const v4u* g4 = reinterpret_cast<const v4u*>(g);
  for (int r = 0; r < kFlagRows / 4; r += 4) {
    unsigned acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < 4; u++) {       // four rows in flight
      const long row = base + r + u;
      if (row < P)
        for (int c = lane; c < C4; c += 64) {
          const v4u v = g4[row * C4 + c];
          acc[u] |= (v[0] | v[1] | v[2] | v[3]) & 0x7fffffffu;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long row = base + r + u;
      const bool any = __ballot(acc[u] != 0u) != 0ull;
      if (lane == 0 && row < P) flags[row] = any ? 1 : 0;
    }
  }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- launch 2: the 3x3 dilation of the flags inside each image, and both counts per block of kBlk rows ----
__global__ __launch_bounds__(256) void rows_dilate_kernel(const uint8_t* __restrict__ flags, int H, int W, long P,
                                                          uint8_t* __restrict__ dflags, int* __restrict__ cnt,
                                                          int* __restrict__ dcnt) {
  __shared__ int s_sum[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p = (long)blockIdx.x * kBlk + tid;
  bool f = false, d = false;
  if (p < P) {
    f = flags[p] != 0;
    const unsigned hw = (unsigned)(H * W), up = (unsigned)p;
    const unsigned rem = up - (up / hw) * hw;
    const int y = (int)(rem / (unsigned)W), x = (int)(rem - (unsigned)y * (unsigned)W);
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
        if ((unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W) d |= flags[p + dy * W + dx] != 0;
    dflags[p] = d ? 1 : 0;
  }
  const int nf = __popcll(__ballot(f)), nd = __popcll(__ballot(d));
  if (lane == 0) {
    s_sum[0][wave] = nf;
    s_sum[1][wave] = nd;
  }
  __syncthreads();
  if (tid == 0) {
    cnt[blockIdx.x] = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
    dcnt[blockIdx.x] = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
  }
}

// ---- launch 3: both ascending lists, -1 in every entry past a list's end, and the counts.  Block b starts at the sum of
// the counts of the blocks before it (each workgroup sums the per-block counts itself: blocks / 256 additions per thread) ----
__global__ __launch_bounds__(256) void rows_list_kernel(const uint8_t* __restrict__ flags,
                                                        const uint8_t* __restrict__ dflags, long P,
                                                        const int* __restrict__ cnt, const int* __restrict__ dcnt,
                                                        int* __restrict__ rows, int* __restrict__ drows,
                                                        int* __restrict__ counts) {
  __shared__ int s_sum[4][4], s_loc[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, nb = gridDim.x;
  int o0 = 0, o1 = 0, t0 = 0, t1 = 0;
  for (int j = tid; j < nb; j += 256) {
    const int c0 = cnt[j], c1 = dcnt[j];
    t0 += c0;
    t1 += c1;
    o0 += j < b ? c0 : 0;
    o1 += j < b ? c1 : 0;
  }
  o0 = wave_sum(o0);
  o1 = wave_sum(o1);
  t0 = wave_sum(t0);
  t1 = wave_sum(t1);
  const long p = (long)b * kBlk + tid;
  const bool f = p < P && flags[p] != 0, d = p < P && dflags[p] != 0;
  const unsigned long long mf = __ballot(f), md = __ballot(d);
  if (lane == 0) {
    s_sum[0][wave] = o0;
    s_sum[1][wave] = o1;
    s_sum[2][wave] = t0;
    s_sum[3][wave] = t1;
    s_loc[0][wave] = __popcll(mf);
    s_loc[1][wave] = __popcll(md);
  }
  __syncthreads();
  int base0 = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
  int base1 = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
  const int tot0 = s_sum[2][0] + s_sum[2][1] + s_sum[2][2] + s_sum[2][3];
  const int tot1 = s_sum[3][0] + s_sum[3][1] + s_sum[3][2] + s_sum[3][3];
#pragma unroll
  for (int w = 0; w < 4; w++)
    if (w < wave) {
      base0 += s_loc[0][w];
      base1 += s_loc[1][w];
    }
  const unsigned long long below = (1ull << lane) - 1ull;
  if (f) rows[base0 + __popcll(mf & below)] = (int)p;
  if (d) drows[base1 + __popcll(md & below)] = (int)p;
  if (p < P && p >= tot0) rows[p] = -1;        // (entries below a total belong to the list writers)
  if (p < P && p >= tot1) drows[p] = -1;
  if (b == 0 && tid == 0) {
    counts[0] = tot0;
    counts[1] = tot1;
  }
}

// =====================================================================================================================
// jdet_conv3x3_wgrad_rows: conv_wgrad.hip's plain kernel, one register set, K index from the list.  Worker w of a
// (Cout tile, Cin tile, tap) takes the K steps w, w + kw, w + 2 kw, ... (16 list entries each) while they start below
// the count.
struct WgradRowsArgs {
  const float* x;        // (N, H, W, Cin)
  const float* gy;       // (N, H, W, Cout)
  const int* rows;       // ascending positions, [0, *count)
  const int* count;
  float* gw;             // (Cout, 3, 3, Cin), accumulated into
  int N, H, W, Cin, Cout, kw;
};

constexpr int BKW = 16;

template <int TM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
void conv3x3_wgrad_rows_kernel(WgradRowsArgs a) {
  constexpr int TN = 1, BK = BKW;
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int SA = BM + 32, SB = BN + 32;             // LDS row strides in floats (conv_wgrad.hip)
  constexpr int TILE_A = BK * SA * 4, TILE_B = BK * SB * 4;
  constexpr int CA = BM / 4, CB = BN / 4;
  constexpr int PA = BK * CA / 256, PB = BK * CB / 256;
  static_assert(PA >= 1 && PB >= 1, "tile shape");
  __shared__ __attribute__((aligned(16))) char s_raw[2 * (TILE_A + TILE_B)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.N * a.H * a.W;                        // (host: (P + BK) * channels < 2^30)
  int cnt = a.count[0];
  cnt = cnt < 0 ? 0 : (cnt > P ? P : cnt);
  const int all_steps = (cnt + BK - 1) / BK;
  const int mt = (a.Cout + BM - 1) / BM, nt = (a.Cin + BN - 1) / BN;
  const int tiles = mt * nt * 9;
  const int worker = (int)((unsigned)blockIdx.x / (unsigned)tiles), tile = blockIdx.x - worker * tiles;
  if (worker >= all_steps) return;
  const int nsteps = (all_steps - worker + a.kw - 1) / a.kw;
  const int rest = (int)((unsigned)tile / 9u), tap = tile - rest * 9;
  const int mq = (int)((unsigned)rest / (unsigned)nt);
  const int n0 = (rest - mq * nt) * BN, m0 = mq * BM;
  const int tr = (tap * 11) >> 5;
  const int dy = tr - 1, dx = tap - tr * 3 - 1;

  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (unsigned)((long)P * a.Cin * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rg =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.gy, 0, (unsigned)((long)P * a.Cout * 4), 0x00020000);

  // ---- loader role: A (gY) pass p covers K row p * (256 / CA) + tid / CA, chunk tid % CA; B (X) likewise.  The list
  // entries of the NEXT step's rows are fetched behind the loads of this one: a step opens with its positions ready.
  const int a_chunk = tid % CA, a_row = tid / CA;
  const int b_chunk = tid % CB, b_row = tid / CB;
  const bool a_cok = m0 + a_chunk * 4 < a.Cout, b_cok = n0 + b_chunk * 4 < a.Cin;
  int a_st[PA], b_st[PB], a_pos[PA], b_pos[PB];
#pragma unroll
  for (int p = 0; p < PA; p++) a_st[p] = ((p * (256 / CA) + a_row) * SA + a_chunk * 4) * 4;
#pragma unroll
  for (int p = 0; p < PB; p++) b_st[p] = TILE_A + ((p * (256 / CB) + b_row) * SB + b_chunk * 4) * 4;
  int next = worker;                                    // the K step whose list entries are fetched next
  auto fetch_pos = [&]() {
#pragma unroll
    for (int p = 0; p < PA; p++) {
      const int li = next * BK + p * (256 / CA) + a_row;
      a_pos[p] = li < cnt ? a.rows[li] : -1;
    }
#pragma unroll
    for (int p = 0; p < PB; p++) {
      const int li = next * BK + p * (256 / CB) + b_row;
      b_pos[p] = li < cnt ? a.rows[li] : -1;
    }
    next += a.kw;
  };
  v4f ra[PA], rb[PB];
  const unsigned hw = (unsigned)(a.H * a.W);
  auto load_step = [&]() {
#pragma unroll
    for (int p = 0; p < PA; p++) {
      const bool ok = a_cok && (unsigned)a_pos[p] < (unsigned)P;
      ra[p] = buf_load(rg, ok ? ((unsigned)(a_pos[p] * a.Cout + m0 + a_chunk * 4)) * 4u : kOob, 0);
    }
#pragma unroll
    for (int p = 0; p < PB; p++) {
      const unsigned up = (unsigned)b_pos[p];
      const unsigned rem = up - (up / hw) * hw;
      const int y = (int)(rem / (unsigned)a.W), x = (int)(rem - (unsigned)y * (unsigned)a.W);
      const bool in = b_cok && up < (unsigned)P && (unsigned)(y + dy) < (unsigned)a.H && (unsigned)(x + dx) < (unsigned)a.W;
      rb[p] = buf_load(rx, in ? ((unsigned)((b_pos[p] + dy * a.W + dx) * a.Cin + n0 + b_chunk * 4)) * 4u : kOob, 0);
    }
    fetch_pos();
  };
  auto store_step = [&](int buf) {
    char* base = s_raw + buf * (TILE_A + TILE_B);
#pragma unroll
    for (int p = 0; p < PA; p++) *reinterpret_cast<v4f*>(base + a_st[p]) = ra[p];
#pragma unroll
    for (int p = 0; p < PB; p++) *reinterpret_cast<v4f*>(base + b_st[p]) = rb[p];
  };

  // ---- compute role (conv_wgrad.hip) ----
  const int wm = wave >> 1, wn = wave & 1;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int fa_off = (fhalf * SA + wm * 32 * TM + frow) * 4;
  const int fb_off = TILE_A + (fhalf * SB + wn * 32 * TN + frow) * 4;
  v16f acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

  fetch_pos();
  load_step();
  store_step(0);
  __syncthreads();
  // every step loads its successor's rows (the step past the worker's last too: its list entries are not read, its rows
  // come back as zeros and are stored and never used)
  for (int step = 0; step < nsteps; step++) {
    const int buf = step & 1;
    load_step();
    const char* sb = s_raw + buf * (TILE_A + TILE_B);
    float fa[2][TM], fb[2][TN];
    auto frags = [&](int q) {
#pragma unroll
      for (int i = 0; i < TM; i++) fa[q & 1][i] = *reinterpret_cast<const float*>(sb + fa_off + (2 * q * SA + i * 32) * 4);
#pragma unroll
      for (int j = 0; j < TN; j++) fb[q & 1][j] = *reinterpret_cast<const float*>(sb + fb_off + (2 * q * SB + j * 32) * 4);
    };
    frags(0);
#pragma unroll
    for (int q = 0; q < BK / 2; q++) {
      if (q + 1 < BK / 2) frags(q + 1);
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q & 1][i], fb[q & 1][j], acc[i][j], 0, 0, 0);
    }
    store_step(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue (conv_wgrad.hip): a register's 32 lanes add to 128 contiguous bytes of gW[co, tap, :] ----
  const long gw_bytes = (long)a.Cout * 9 * a.Cin * 4;
  if (m0 + BM <= a.Cout && n0 + BN <= a.Cin && gw_bytes < (1L << 32)) {
    const __amdgpu_buffer_rsrc_t rgw = __builtin_amdgcn_make_buffer_rsrc((void*)a.gw, 0, (unsigned)gw_bytes, 0x00020000);
    const unsigned row_bytes = (unsigned)(9 * a.Cin * 4);
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const unsigned ci = (unsigned)(n0 + wn * 32 * TN + j * 32 + (lane & 31));
        const unsigned co = (unsigned)(m0 + wm * 32 * TM + i * 32 + 4 * (lane >> 5));
        const unsigned base = ((co * 9u + (unsigned)tap) * (unsigned)a.Cin + ci) * 4u;
#pragma unroll
        for (int e = 0; e < 16; e++)
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc[i][j][e], rgw, (int)base, (int)(cd_row(e) * row_bytes), 0);
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int ci = n0 + wn * 32 * TN + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int co = m0 + wm * 32 * TM + i * 32 + cd_row(e) + 4 * (lane >> 5);
        if (co < a.Cout && ci < a.Cin) unsafeAtomicAdd(a.gw + ((size_t)co * 9 + tap) * a.Cin + ci, acc[i][j][e]);
      }
    }
}

// =====================================================================================================================
// jdet_conv3x3_dgrad_rows: conv_igemm.hip's 64 x 64 tile.  "Input" = g with KC = Cout channels, "weights" = Wd
// (Cin, 3, 3, Cout), outputs = NO = Cin channels of gx.  M tile t holds the list entries [64 t, 64 t + 64).
//
// jdet_conv3x3_rows_forward (FWD) is the same tile read the other way round: out[r] = sum_tap in[nbr(r, tap)] . w[tap] is
// a forward convolution whose (NO, 3, 3, KC) weights are the (Cout, 3, 3, Cin) layout of the dense forward -- "input" = x
// (the `Cout` field holds ITS channel count), outputs = the `Cin` field's channels of y -- and whose epilogue is
// conv_igemm.hip's: + bias, ReLU, times the row's mask.  One body; the epilogue is selected at compile time.
struct DgradRowsArgs {
  const float* g;        // (N, H, W, Cout)
  const float* wd;       // (Cin, 3, 3, Cout): flipped taps (jdet_conv_dgrad_weights)
  const int* rows;       // ascending positions, [0, *count)
  const int* count;
  float* gx;             // (N, H, W, Cin); only the listed rows are written
  int N, H, W, Cin, Cout;
  const float* bias;     // FWD only: (Cin field) or null
  const float* rowmask;  // FWD only: (N*H*W) or null, multiplies the finished row (after bias / ReLU)
  int relu;              // FWD only
};

template <int BK, int KG, bool FWD>
__global__ __launch_bounds__(256 * KG) __attribute__((amdgpu_waves_per_eu(4)))
void conv3x3_dgrad_rows_kernel(DgradRowsArgs a) {
  constexpr int BT = 64;
  constexpr int DEPTH = KG >= 1 ? 1 : 2;      // one register set (value-dependent: conv_mfma_loop.inc's other branch is discarded)
  using TL = MfmaTile<BT, BK, KG>;
  constexpr int T = TL::T, CH = TL::CH, RPP = TL::RPP, PASSES = TL::PASSES, TILE = TL::TILE, QN = TL::QN;
  static_assert(T == 1, "64 x 64 tile");
  __shared__ __attribute__((aligned(16))) char s_raw[4 * TILE];     // [buffer][A | B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.N * a.H * a.W;                                     // (host: P * channels < 2^30)
  const int KC = a.Cout, NO = a.Cin;
  int cnt = a.count[0];
  cnt = cnt < 0 ? 0 : (cnt > P ? P : cnt);
  const int NT = (NO + BT - 1) / BT;
  // plain workgroup order: the tiles below the count are the FIRST ids, round-robin over the 8 XCDs
  const int mtile = (int)((unsigned)blockIdx.x / (unsigned)NT);
  const int m0 = mtile * BT;
  if (m0 >= cnt) return;
  const int n0 = (blockIdx.x - mtile * NT) * BT;
  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.g, 0, (unsigned)((long)P * KC * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.wd, 0, (unsigned)((long)NO * 9 * KC * 4), 0x00020000);
  // ---- loader role: pass p covers tile row p * RPP + tid / CH, chunk tid % CH ----
  const int lchunk = tid % CH, lrow = tid / CH;
  int img[PASSES], py[PASSES], px[PASSES];
  bool m_ok[PASSES];
  unsigned wv[PASSES];
  int st_off[PASSES];
  const unsigned hw = (unsigned)(a.H * a.W);
#pragma unroll
  for (int p = 0; p < PASSES; p++) {
    const int row = p * RPP + lrow;
    const int li = m0 + row;
    const unsigned pos = li < cnt ? (unsigned)a.rows[li] : 0xFFFFFFFFu;
    m_ok[p] = pos < (unsigned)P;
    const unsigned im = m_ok[p] ? pos / hw : 0u, rem = m_ok[p] ? pos - im * hw : 0u, oy = rem / (unsigned)a.W;
    img[p] = (int)im;
    py[p] = (int)oy;
    px[p] = (int)(rem - oy * (unsigned)a.W);
    wv[p] = n0 + row < NO ? ((unsigned)((n0 + row) * 9 * KC + lchunk * 4)) * 4u : kOob;
    st_off[p] = swz_bytes<BK>(row, lchunk);
  }
  const int nsteps = 9 * (KC / BK);

  unsigned av[PASSES];
  auto set_tap = [&](int tap) {
    const int r = (tap * 11) >> 5, s = tap - r * 3;
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      const int yy = py[p] + r - 1, xx = px[p] + s - 1;
      const bool in = m_ok[p] && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      const unsigned off = ((unsigned)(((img[p] * a.H + yy) * a.W + xx) * KC + lchunk * 4)) * 4u;
      av[p] = in ? off : kOob;
    }
  };

  v4f ra[DEPTH][PASSES], rb[DEPTH][PASSES];
  auto load_set = [&](auto setc, int tap, int c) {
    constexpr int S = decltype(setc)::value;
    const unsigned sa = (unsigned)(c * 4), sb = (unsigned)((tap * KC + c) * 4);
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
  auto load_step = [&](int tap, int c) { load_set(Set0{}, tap, c); };
  auto store_step = [&](int buf) { store_set(Set0{}, buf); };

  // ---- compute role (conv_igemm.hip) ----
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
  for (int e = 0; e < 16; e++) acc[0][0][e] = 0.f;

  int tap = 0, c = 0;
  set_tap(0);
  auto advance = [&]() {
    c += BK;
    if (c == KC) {
      c = 0;
      tap++;
      set_tap(tap);
    }
  };
  auto mfma_step = [&](int buf) { ::mfma_step<BT, BK, KG>(s_raw, buf, fa_off, fb_off, acc); };
#include "conv_mfma_loop.inc"
  if (KG == 2) {      // the second wave group hands its partial tile over through LDS (the operand buffers are free now)
    float* red = reinterpret_cast<float*>(s_raw);
    if (kg == 1) {
#pragma unroll
      for (int e = 0; e < 16; e++) red[red_index<T>(wave, lane, 0, 0, e)] = acc[0][0][e];
    }
    __syncthreads();
    if (kg == 1) return;
  }

  // ---- epilogue: C/D layout of the 32 x 32 MFMA: column = lane & 31, row = cd_row(reg) + 4 * (lane >> 5); a tile row
  // goes to the list entry's row of gx (rows past the count: an out-of-range offset, the store is dropped) ----
  const __amdgpu_buffer_rsrc_t ry =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.gx, 0, (unsigned)((long)P * NO * 4), 0x00020000);
  const int lrow0 = m0 + wm * (BT / 2) + 4 * (lane >> 5);
  const int n = n0 + wn * (BT / 2) + (lane & 31);
  unsigned dst[16];
  float mk[16];
  float b = 0.f;
  if constexpr (FWD) b = (a.bias && n < NO) ? a.bias[n] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int li = lrow0 + cd_row(e);
    const unsigned pos = li < cnt ? (unsigned)a.rows[li] : 0xFFFFFFFFu;
    dst[e] = (pos < (unsigned)P && n < NO) ? (pos * (unsigned)NO + (unsigned)n) * 4u : kOob;
    if constexpr (FWD) mk[e] = (a.rowmask && pos < (unsigned)P) ? a.rowmask[pos] : 1.f;      // all 16 loads in flight together
  }
#pragma unroll
  for (int e = 0; e < 16; e++) {
    float v = acc[0][0][e];
    if (KG == 2) v += reinterpret_cast<const float*>(s_raw)[red_index<T>(wave, lane, 0, 0, e)];
    if constexpr (FWD) {      // conv_igemm.hip's epilogue, in its order
      v += b;
      if (a.relu) v = fmaxf(v, 0.f);
      if (a.rowmask) v *= mk[e];
    }
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, dst[e], 0u, 0);
  }
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// K workers per (Cout tile, Cin tile, tap): ~1150 workgroups in all, as the dense kernel's split aims at
inline int wgrad_rows_workers(int Cin, int Cout) {
  const int tm = Cout > 64 ? 2 : 1;
  const long tiles = (long)((Cout + 64 * tm - 1) / (64 * tm)) * ((Cin + 63) / 64) * 9;
  long kw = 1152 / tiles;
  return (int)(kw < 8 ? 8 : (kw > 64 ? 64 : kw));
}

}  // namespace

JDET_API size_t jdet_rows_nonzero_workspace(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const long P = (long)N * H * W;
  const long nb = (P + kBlk - 1) / kBlk;
  return align16((size_t)P) + sizeof(int32_t) * 2 * (size_t)nb;
}

JDET_API int jdet_rows_nonzero(const float* g_nhwc, int N, int H, int W, int C, uint8_t* flags, int32_t* rows,
                               int32_t* rows_dilated, int32_t* counts, void* workspace, size_t workspace_bytes,
                               jdet_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return JDET_E_BADARG;
  if (C % 4 != 0) return JDET_E_UNSUPPORTED;
  const long P = (long)N * H * W;
  if (P * C >= (1L << 30)) return JDET_E_UNSUPPORTED;                 // 32-bit byte offsets, as the convolutions
  if (!g_nhwc || !flags || !rows || !rows_dilated || !counts) return JDET_E_BADARG;
  if (((uintptr_t)g_nhwc & 15) || (((uintptr_t)rows | (uintptr_t)rows_dilated | (uintptr_t)counts) & 3))
    return JDET_E_BADARG;
  if (!workspace || workspace_bytes < jdet_rows_nonzero_workspace(N, H, W)) return JDET_E_WORKSPACE;
  if ((uintptr_t)workspace & 3) return JDET_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((P + kBlk - 1) / kBlk);
  uint8_t* dflags = (uint8_t*)workspace;
  int* cnt = (int*)((char*)workspace + align16((size_t)P));
  int* dcnt = cnt + nb;
  hipLaunchKernelGGL(rows_flag_kernel, dim3((unsigned)((P + kFlagRows - 1) / kFlagRows)), dim3(256), 0, st, g_nhwc, P,
                     C / 4, flags);
  hipLaunchKernelGGL(rows_dilate_kernel, dim3(nb), dim3(256), 0, st, flags, H, W, P, dflags, cnt, dcnt);
  hipLaunchKernelGGL(rows_list_kernel, dim3(nb), dim3(256), 0, st, flags, dflags, P, cnt, dcnt, rows, rows_dilated,
                     counts);
  return jdet_launch_status();
}

JDET_API int jdet_conv3x3_rows_supported(int Cin, int Cout) {
  return Cin > 0 && Cout > 0 && Cin % 4 == 0 && Cout % 16 == 0;
}

JDET_API int jdet_conv3x3_wgrad_rows_workers(int Cin, int Cout) {
  return jdet_conv3x3_rows_supported(Cin, Cout) ? wgrad_rows_workers(Cin, Cout) : 0;
}

JDET_API int jdet_conv3x3_wgrad_rows(const float* x_nhwc, const float* gy_nhwc, const int32_t* rows,
                                     const int32_t* count, int N, int H, int W, int Cin, int Cout, float* gw_krsc,
                                     jdet_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return JDET_E_BADARG;
  if (!jdet_conv3x3_rows_supported(Cin, Cout)) return JDET_E_UNSUPPORTED;
  const long P = (long)N * H * W;
  if ((P + BKW) * (Cin > Cout ? Cin : Cout) >= (1L << 30)) return JDET_E_UNSUPPORTED;      // 32-bit byte offsets
  if (!x_nhwc || !gy_nhwc || !rows || !count || !gw_krsc) return JDET_E_BADARG;
  if ((((uintptr_t)x_nhwc) | ((uintptr_t)gy_nhwc)) & 15 || (((uintptr_t)rows | (uintptr_t)count) & 3)) return JDET_E_BADARG;
  const int tm = Cout > 64 ? 2 : 1;
  const int kw = wgrad_rows_workers(Cin, Cout);
  const unsigned grid = (unsigned)(((Cout + 64 * tm - 1) / (64 * tm)) * ((Cin + 63) / 64) * 9 * kw);
  WgradRowsArgs a{x_nhwc, gy_nhwc, rows, count, gw_krsc, N, H, W, Cin, Cout, kw};
  hipStream_t st = (hipStream_t)stream;
  if (tm == 2) hipLaunchKernelGGL((conv3x3_wgrad_rows_kernel<2>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((conv3x3_wgrad_rows_kernel<1>), dim3(grid), dim3(256), 0, st, a);
  return jdet_launch_status();
}

JDET_API int jdet_conv3x3_dgrad_rows(const float* gy_nhwc, const float* wd_crsk, const int32_t* rows,
                                     const int32_t* count, int N, int H, int W, int Cin, int Cout, int zero_first,
                                     float* gx_nhwc, jdet_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return JDET_E_BADARG;
  if (!jdet_conv3x3_rows_supported(Cin, Cout)) return JDET_E_UNSUPPORTED;
  const long P = (long)N * H * W;
  if (P * (Cin > Cout ? Cin : Cout) >= (1L << 30)) return JDET_E_UNSUPPORTED;               // 32-bit byte offsets
  if (!gy_nhwc || !wd_crsk || !rows || !count || !gx_nhwc) return JDET_E_BADARG;
  if ((((uintptr_t)gy_nhwc) | ((uintptr_t)wd_crsk)) & 15 || (((uintptr_t)rows | (uintptr_t)count | (uintptr_t)gx_nhwc) & 3))
    return JDET_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_first) {
    const int e = jdet_zero_async(gx_nhwc, sizeof(float) * (size_t)P * Cin, st);
    if (e) return e;
  }
  DgradRowsArgs a{gy_nhwc, wd_crsk, rows, count, gx_nhwc, N, H, W, Cin, Cout, nullptr, nullptr, 0};
  const unsigned grid = (unsigned)(((P + 63) / 64) * ((Cin + 63) / 64));
  if (Cout % 32 == 0) hipLaunchKernelGGL((conv3x3_dgrad_rows_kernel<32, 2, false>), dim3(grid), dim3(512), 0, st, a);
  else hipLaunchKernelGGL((conv3x3_dgrad_rows_kernel<16, 1, false>), dim3(grid), dim3(256), 0, st, a);
  return jdet_launch_status();
}

// =====================================================================================================================
// the row-sparse forward

JDET_API size_t jdet_rows_from_flags_workspace(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const long P = (long)N * H * W;
  const long nb = (P + kBlk - 1) / kBlk;
  return 2 * align16((size_t)P) + sizeof(int32_t) * 4 * (size_t)nb;
}

JDET_API int jdet_rows_from_flags(const uint8_t* flags, int N, int H, int W, int32_t* rows, int32_t* rows_dilated,
                                  int32_t* rows_dilated2, int32_t* counts, void* workspace, size_t workspace_bytes,
                                  jdet_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0) return JDET_E_BADARG;
  const long P = (long)N * H * W;
  if (P >= (1L << 30)) return JDET_E_UNSUPPORTED;                     // positions are int32 list entries
  if (!flags || !rows || !rows_dilated || !rows_dilated2 || !counts) return JDET_E_BADARG;
  if (((uintptr_t)rows | (uintptr_t)rows_dilated | (uintptr_t)rows_dilated2 | (uintptr_t)counts) & 3) return JDET_E_BADARG;
  if (!workspace || workspace_bytes < jdet_rows_from_flags_workspace(N, H, W)) return JDET_E_WORKSPACE;
  if ((uintptr_t)workspace & 3) return JDET_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((P + kBlk - 1) / kBlk);
  uint8_t* d1 = (uint8_t*)workspace;
  uint8_t* d2 = d1 + align16((size_t)P);
  int* c0 = (int*)(d2 + align16((size_t)P));
  int* c1 = c0 + nb;
  int* c1b = c1 + nb;       // the count of d1 once more (the second dilation's "flag" count)
  int* c2 = c1b + nb;
  hipLaunchKernelGGL(rows_dilate_kernel, dim3(nb), dim3(256), 0, st, flags, H, W, P, d1, c0, c1);
  hipLaunchKernelGGL(rows_dilate_kernel, dim3(nb), dim3(256), 0, st, (const uint8_t*)d1, H, W, P, d2, c1b, c2);
  hipLaunchKernelGGL(rows_list_kernel, dim3(nb), dim3(256), 0, st, flags, (const uint8_t*)d1, P, (const int*)c0,
                     (const int*)c1, rows, rows_dilated, counts);
  // (writes rows_dilated and counts[1] a second time, with the same values: the kernels stay the two of jdet_rows_nonzero)
  hipLaunchKernelGGL(rows_list_kernel, dim3(nb), dim3(256), 0, st, (const uint8_t*)d1, (const uint8_t*)d2, P,
                     (const int*)c1b, (const int*)c2, rows_dilated, rows_dilated2, counts + 1);
  return jdet_launch_status();
}

JDET_API int jdet_conv3x3_rows_forward_supported(int Cin, int Cout) {
  return Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 16 == 0;
}

JDET_API int jdet_conv3x3_rows_forward(const float* x_nhwc, const float* w_krsc, const float* bias, int relu,
                                       const float* rowmask, const int32_t* rows, const int32_t* count, int N, int H,
                                       int W, int Cin, int Cout, int zero_first, float* y_nhwc, jdet_stream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return JDET_E_BADARG;
  if (!jdet_conv3x3_rows_forward_supported(Cin, Cout)) return JDET_E_UNSUPPORTED;
  const long P = (long)N * H * W;
  if (P * (Cin > Cout ? Cin : Cout) >= (1L << 30)) return JDET_E_UNSUPPORTED;               // 32-bit byte offsets
  if (!x_nhwc || !w_krsc || !rows || !count || !y_nhwc) return JDET_E_BADARG;
  if ((((uintptr_t)x_nhwc) | ((uintptr_t)w_krsc)) & 15) return JDET_E_BADARG;
  if (((uintptr_t)rows | (uintptr_t)count | (uintptr_t)y_nhwc | (uintptr_t)bias | (uintptr_t)rowmask) & 3) return JDET_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_first) {
    const int e = jdet_zero_async(y_nhwc, sizeof(float) * (size_t)P * Cout, st);
    if (e) return e;
  }
  // the tile's "Cin" field = its output channels, its "Cout" field = the K channels (see DgradRowsArgs)
  DgradRowsArgs a{x_nhwc, w_krsc, rows, count, y_nhwc, N, H, W, Cout, Cin, bias, rowmask, relu ? 1 : 0};
  const unsigned grid = (unsigned)(((P + 63) / 64) * ((Cout + 63) / 64));
  if (Cin % 32 == 0) hipLaunchKernelGGL((conv3x3_dgrad_rows_kernel<32, 2, true>), dim3(grid), dim3(512), 0, st, a);
  else hipLaunchKernelGGL((conv3x3_dgrad_rows_kernel<16, 1, true>), dim3(grid), dim3(256), 0, st, a);
  return jdet_launch_status();
}
