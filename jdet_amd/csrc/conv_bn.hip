// The ResNet bottleneck convolutions as ONE fp32-MFMA implicit-GEMM family with the layer's neighbours in the epilogue,
// channels-last: 1x1 and 3x3, stride 1 and 2, forward AND data gradient.
//
// Reference: Bottleneck.execute (python/jdet/models/backbones/resnet.py:L61-93: conv1x1 -> bn -> relu, conv3x3(stride)
// -> bn -> relu, conv1x1 -> bn -> (+identity | downsample) -> relu), the layers of ResNet._make_layer (L131-154), with
// every BatchNorm in eval mode while training (`norm_eval`, L177-185) -- i.e. a per-channel affine map whose weight / bias
// still train -- and the gradients Jittor's autograd derives for that chain.
//
//   Y[m, n] = epilogue( sum_{tap, c} X[pixel(m) * stride + tap - pad, c] * Wt[n, tap, c] )      m = (image, oy, ox)
//
// The kernel is conv_bn_kernel.h; its main loop is the tiling of conv_igemm.hip, shared with it through conv_mfma.h /
// conv_mfma_loop.inc (v_mfma_f32_32x32x2_f32, 2 x 2 waves [x 2 K groups], 128^2 / 64^2 output
// tiles, XOR-swizzled 16-byte LDS chunks so that ONE ds_read_b128 per operand tile feeds four MFMAs, raw buffer loads
// with out-of-range = zero for the halo, double-buffered LDS, XCD-aware tile order) with the tap geometry a run-time
// (R, stride).  What is new is what happens to the accumulators -- a library convolution has no epilogue the caller
// controls, which is why every conv of the backbone used to be followed by an elementwise BatchNorm pass (forward) and
// preceded by one (backward):
//   mode FORWARD : y = [relu]( acc * a[n] + sh[n] [+ residual[m, n]] )        a = gamma * rsqrt(var + eps), sh = beta - mean * a
//   mode ADD     : gx = acc + grad_out[m, n] * [act_out[m, n] > 0]            the data gradient of conv1 of a block PLUS the
//                                                                             identity branch's gradient (the block's true grad_x)
//   mode MASK    : g = acc * [act[m, n] > 0];  partial column sums of g and g * (act - beta[n]);  y = g * a[n]
//                                                                             the data gradient w.r.t. the layer below's
//                                                                             activation act = relu(bn(conv)), turned straight
//                                                                             into the gradient w.r.t. that conv's output, with
//                                                                             the sums its BatchNorm weight / bias gradients need
//                                                                             (dbeta = sum g, dgamma = sum g * xhat,
//                                                                             xhat = (act - beta) / gamma wherever act > 0)
// The data gradient itself is this same kernel run on the flipped / transposed weights (jdet_conv_dgrad_weights: one
// launch per step for the whole backbone).  Column sums leave the workgroup as one partial row per (M tile, wave row)
// -- deterministic, no atomics -- and are finished by jdet_bn_sums_finish (frozen_bn.hip).
// Bound: the matrix pipe at the 3x3 layers (2 * M * N * K flop at 157 TFLOP/s); HBM at the 1x1 layers of the big maps
// (64 <-> 256 channels at 2 x 256^2: ~170-300 MB per layer, where the fused epilogue saves the separate pass's 2-3 tensor
// round trips).
#include "conv_bn_kernel.h"

namespace {

// Second stage of the cross-workgroup K split: sum of the partial planes in a fixed order + the same epilogue.
// Workgroup = 64 rows x 64 columns: thread (ty, tx) owns the column quad tx of rows ty, ty + 16, ty + 32, ty + 48; the
// column sums of mode MASK meet in LDS (fixed order) and leave as one partial row per 64-row block.
__global__ __launch_bounds__(256) void conv_bn_finish_kernel(CbArgs a) {
  __shared__ float s_sum[16][64][2];
  const long M = (long)a.N * a.Ho * a.Wo;
  const jdet_conv_epilogue_t& ep = a.ep;
  const int mode = ep.mode;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int n = blockIdx.y * 64 + tx * 4;
  const bool nok = n < a.Cout;          // Cout % 4 == 0: the whole quad is in or out
  v4f sa = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f}, beta = {0.f, 0.f, 0.f, 0.f};
  if (nok && mode != JDET_EPI_ADD) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float x, y;
      bn_affine(ep.bn, n + k, x, y);
      sa[k] = x;
      sh[k] = y;
      beta[k] = ep.bn.bias ? ep.bn.bias[n + k] : 0.f;
    }
  }
  v4f c1 = {0.f, 0.f, 0.f, 0.f}, c2 = {0.f, 0.f, 0.f, 0.f};
  const size_t plane = (size_t)M * a.Cout;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const long m = (long)blockIdx.x * 64 + ty + 16 * r;
    if (m >= M || !nok) continue;
    const size_t idx = (size_t)m * a.Cout + n;
    v4f v = *reinterpret_cast<const v4f*>(a.partial + idx);
    for (int k = 1; k < a.ksplit; k++) v += *reinterpret_cast<const v4f*>(a.partial + (size_t)k * plane + idx);
    if (mode == JDET_EPI_FORWARD) {
      if (ep.affine) v = v * sa + sh;
      if (ep.residual) v += *reinterpret_cast<const v4f*>(ep.residual + idx);
      if (ep.relu)
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = fmaxf(v[k], 0.f);
    } else if (mode == JDET_EPI_ADD) {
      const v4f g = *reinterpret_cast<const v4f*>(ep.grad_out + idx), y = *reinterpret_cast<const v4f*>(ep.act + idx);
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] += y[k] > 0.f ? g[k] : 0.f;
    } else {
      const v4f y = *reinterpret_cast<const v4f*>(ep.act + idx);
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = y[k] > 0.f ? v[k] : 0.f;
      c1 += v;
      c2 += v * (y - beta);
      v *= sa;
    }
    *reinterpret_cast<v4f*>(a.y + idx) = v;
  }
  if (mode == JDET_EPI_MASK && ep.sums) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      s_sum[ty][tx * 4 + k][0] = c1[k];
      s_sum[ty][tx * 4 + k][1] = c2[k];
    }
    __syncthreads();
    if (threadIdx.x < 128) {
      const int col = threadIdx.x & 63, which = threadIdx.x >> 6;
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) t += s_sum[r][col][which];
      const int nn = blockIdx.y * 64 + col;
      if (nn < a.Cout) ep.sums[((size_t)blockIdx.x * 2 + which) * a.Cout + nn] = t;
    }
  }
}

// operand tiles TWO K steps ahead on the 64 x 64 tile (both KG), one on the 128 x 128 tile
template <int BT, int BK, int KG>
int launch(const CbArgs& a, hipStream_t st) {
  const long M = (long)a.N * a.Ho * a.Wo;
  const long tiles = ((M + BT - 1) / BT) * ((a.Cout + BT - 1) / BT);
  hipLaunchKernelGGL((conv_bn_kernel<BT, BK, KG, BT == 64 ? 2 : 1>), dim3((unsigned)tiles, a.ksplit), dim3(256 * KG), 0, st, a);
  return jdet_launch_status();
}

// ---- the launch plan: one function decides tile / K split for the launch, the workspace query and the sums geometry ----
struct Plan {
  int bt, bk, kg, ksplit;
  long sums_rows;
};

Plan make_plan(long M, int Cin, int Cout, int taps, int tile, bool workspace) {
  Plan p;
  const int edge = tile & ~3;
  const long tiles128 = ((M + 127) / 128) * ((Cout + 127) / 128);
  const long tiles64 = ((M + 63) / 64) * ((Cout + 63) / 64);
  // 128^2 tiles only for the long reductions (3x3 from 256 input channels up) on maps whose 128-tiles alone fill the
  // chip: measured at the ResNet-50 shapes of a 2 x 1024^2 step (scripts/conv_bn_timing.py tiles, profiles/
  // r05_conv_bn.md), the 64^2 tile without the intra-workgroup K split wins or ties everywhere else (64 -> 256 at
  // 2 x 256^2: 80 vs 103 us; 128 -> 512 at 2 x 128^2: 59 vs 70; 256 -> 256 3x3 at 2 x 64^2: 92 vs 171)
  const bool big = tile ? edge == 128 : (tiles128 >= 512 && Cout > 64 && (long)taps * Cin >= 2304);
  // 16-deep K steps for the 1x1 layers of at most 128 input channels: four to eight short steps instead of two to four
  // (and half the LDS per workgroup): 64 -> 256 + residual at 2 x 256^2 89 vs 97 us, 128 -> 512 + residual at 2 x 128^2
  // 58 vs 65 us; equal elsewhere (scripts/conv_bn_timing.py tiles, profiles/r05_conv_bn.md)
  const bool k32 = Cin % 32 == 0 && !(tile & 1) && !(tile == 0 && taps == 1 && Cin <= 128);
  const int steps = taps * (Cin / (k32 ? 32 : 16));
  // intra-workgroup K split (8 waves): conv_igemm.hip's rule; not for a K loop of one or two steps (the hand-over
  // through LDS then costs as much as the loop)
  const bool split = k32 && !(tile & 2) && (big || tile || tiles64 < 512) && steps >= 4;
  p.bt = big ? 128 : 64;
  p.bk = k32 ? 32 : 16;
  p.kg = split ? 2 : 1;
  p.ksplit = 1;
  // K steps split over workgroups (conv_mfma.h's rule)
  if (tile == 0 && !big && workspace && Cout % 4 == 0) {
    const int k = ksplit_rule(tiles64, steps);
    if (k >= 2) {
      p.ksplit = k;
      p.kg = 1;
    }
  }
  p.sums_rows = p.ksplit > 1 ? (M + 63) / 64 : 2 * ((M + p.bt - 1) / p.bt);
  return p;
}

// flipped / transposed weights for the data gradient: dst[ci][R*R-1-tap][co] = src[co][tap][ci]
struct WtJob {
  const float* src;
  float* dst;
  int Cout, Cin, taps, tile_begin;
};

__global__ __launch_bounds__(256) void dgrad_weights_kernel(const WtJob* __restrict__ jobs, int njobs) {
  __shared__ float s[32][33];
  int j = 0;
  while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].tile_begin) j++;
  const WtJob job = jobs[j];
  int t = blockIdx.x - job.tile_begin;
  const int ct = (job.Cin + 31) / 32, ot = (job.Cout + 31) / 32;
  const int tap = t % job.taps;
  t /= job.taps;
  const int ci0 = (t % ct) * 32, co0 = (t / ct) * 32;
  if (t / ct >= ot) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int co = co0 + ty + 8 * r, ci = ci0 + tx;
    s[ty + 8 * r][tx] = (co < job.Cout && ci < job.Cin) ? job.src[((size_t)co * job.taps + tap) * job.Cin + ci] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int ci = ci0 + ty + 8 * r, co = co0 + tx;
    if (ci < job.Cin && co < job.Cout)
      job.dst[((size_t)ci * job.taps + (job.taps - 1 - tap)) * job.Cout + co] = s[tx][ty + 8 * r];
  }
}

}  // namespace

// Supported: R in {1, 3} (pad R / 2), stride in {1, 2}, Cin % 16 == 0, 16-byte aligned tensors,
// positions * max(Cin, Cout) < 2^30 on both sides.
JDET_API int jdet_conv_bn_supported(int Cin, int Cout, int R, int stride) {
  return Cin > 0 && Cin % 16 == 0 && Cout > 0 && (R == 1 || R == 3) && (stride == 1 || stride == 2);
}

JDET_API size_t jdet_conv_bn_workspace(int N, int H, int W, int Cin, int Cout, int R, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || !jdet_conv_bn_supported(Cin, Cout, R, stride)) return 0;
  const long M = (long)N * out_dim(H, R, stride) * out_dim(W, R, stride);
  const Plan p = make_plan(M, Cin, Cout, R * R, 0, true);
  return p.ksplit > 1 ? sizeof(float) * (size_t)p.ksplit * M * Cout : 0;
}

JDET_API size_t jdet_conv_bn_sums_rows(int N, int H, int W, int Cin, int Cout, int R, int stride, int tile,
                                     int with_workspace) {
  if (N <= 0 || H <= 0 || W <= 0 || !jdet_conv_bn_supported(Cin, Cout, R, stride)) return 0;
  const long M = (long)N * out_dim(H, R, stride) * out_dim(W, R, stride);
  return (size_t)make_plan(M, Cin, Cout, R * R, tile, with_workspace != 0).sums_rows;
}

JDET_API int jdet_conv_bn_forward(const float* x_nhwc, int N, int H, int W, int Cin, const float* w_krsc, int Cout,
                                  int R, int stride, const jdet_conv_epilogue_t* epilogue, int tile, float* y_nhwc,
                                  void* workspace, size_t workspace_bytes, jdet_stream_t stream) {
  CbArgs a{};
  const int bad = cb_check_args(x_nhwc, N, H, W, Cin, w_krsc, Cout, R, stride, epilogue, y_nhwc, a);
  if (bad || N == 0) return bad;
  const jdet_conv_epilogue_t& ep = a.ep;
  const long M = (long)N * a.Ho * a.Wo;
  const int edge = tile & ~3;
  if (tile != 0 && edge != 64 && edge != 128) return JDET_E_BADARG;
  const size_t need_ws = jdet_conv_bn_workspace(N, H, W, Cin, Cout, R, stride);
  // a workspace that is offered but too small is refused, not ignored: without the K split a MASK launch writes twice
  // the partial-sum rows, past the end of a `sums` the caller sized with jdet_conv_bn_sums_rows(..., with_workspace = 1)
  if (tile == 0 && workspace && workspace_bytes && workspace_bytes < need_ws) return JDET_E_WORKSPACE;
  bool ws_ok = workspace && need_ws && workspace_bytes >= need_ws;
  // the finish kernel moves float4s
  if (ws_ok && ((((uintptr_t)y_nhwc) | ((uintptr_t)workspace) | ((uintptr_t)ep.residual) | ((uintptr_t)ep.grad_out) |
                 ((uintptr_t)ep.act)) & 15)) {
    // dropping the K split here changes the number of partial-sum rows (jdet_conv_bn_sums_rows was asked WITH a
    // workspace): a caller that sized `sums` for the split plan would be written past its end -- refuse instead
    if (ep.sums) return JDET_E_BADARG;
    ws_ok = false;
  }
  const Plan p = make_plan(M, Cin, Cout, R * R, tile, ws_ok);
  a.ksplit = p.ksplit;
  hipStream_t st = (hipStream_t)stream;
  if (p.ksplit > 1) {
    a.partial = (float*)workspace;
    int e = p.bk == 32 ? launch<64, 32, 1>(a, st) : launch<64, 16, 1>(a, st);
    if (e) return e;
    hipLaunchKernelGGL(conv_bn_finish_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((Cout + 63) / 64)), dim3(256), 0,
                       st, a);
    return jdet_launch_status();
  }
  if (p.bt == 128)
    return p.bk == 32 ? (p.kg == 2 ? launch<128, 32, 2>(a, st) : launch<128, 32, 1>(a, st)) : launch<128, 16, 1>(a, st);
  return p.bk == 32 ? (p.kg == 2 ? launch<64, 32, 2>(a, st) : launch<64, 32, 1>(a, st)) : launch<64, 16, 1>(a, st);
}

// jobs: DEVICE array of njobs records {src (Cout, R, R, Cin), dst (Cin, R, R, Cout), Cout, Cin, taps, tile_begin} with
// tile_begin the running sum of ceil(Cout / 32) * ceil(Cin / 32) * taps; total_tiles = that sum over all jobs.
JDET_API int jdet_conv_dgrad_weights(const void* jobs_device, int njobs, int total_tiles, jdet_stream_t stream) {
  if (njobs < 0 || total_tiles < 0) return JDET_E_BADARG;
  if (njobs == 0 || total_tiles == 0) return JDET_OK;
  if (!jobs_device) return JDET_E_BADARG;
  static_assert(sizeof(WtJob) == 32, "record layout of the ABI");
  hipLaunchKernelGGL(dgrad_weights_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                     (const WtJob*)jobs_device, njobs);
  return jdet_launch_status();
}
