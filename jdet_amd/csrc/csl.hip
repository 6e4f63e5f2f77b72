// Circular Smooth Label (include/jdet_hip_csl.h): the angle branch of CSLRRetinaHead.
//
//   jdet_csl_encode             CSLCoder.encode: angle deltas -> (n, L) smooth labels
//   jdet_csl_decode             CSLCoder.decode of chosen rows of a level's (rows, L) logits: first argmax -> angle
//   jdet_csl_angle_loss_level   SmoothFocalLoss of a level on labels that are never stored + d / d logits, one pass
//
// The reference materialises (anchors, L) labels for every anchor through a 180-entry scatter, compacts logits and
// labels by a boolean mask (a host synchronisation per level) and runs a dozen element-wise passes over the rest.  Here
// a workgroup owns a tile of kTileRows rows: it reads column 4 of the tile's weight rows (and of the target rows that
// are selected), zeroes the unselected part of the tile's contiguous gradient span with wide stores, and works each
// selected row with one wave, lanes striding over L.  Logits are read at selected rows only.  It is a write-bandwidth
// kernel: what it costs is the dense gradient, written once.
//
// Row arithmetic and sums are double, rounded once; the order of every addition is fixed: a lane adds its own elements
// in (tile, row, bin) order, then reduce.h's wave / workgroup sums, one double partial per workgroup in the loss
// workspace, one finishing launch.
#include "jdet_hip_csl.h"
#include "reduce.h"

namespace {

constexpr int kTileRows = 64;
// the loss workspace (reduce.h: kJdetLossWorkspaceBytes) as double partial sums
constexpr int kSumGridCap = (int)(kJdetLossWorkspaceBytes / sizeof(double));
static_assert(kSumGridCap == 512 && kSumGridCap <= kJdetLossGridCap, "4 KiB of double partials");

struct Label {
  int window, L, radius;   // radius: RECT / TRIANGLE
  double scale;            // GAUSSIAN: 1 / (2 radius^2)
  float omega;             // the float32 the bin is evaluated with
};

// bin of a target (the rule of include/jdet_hip_csl.h); -ffp-contract=off keeps the three float32 operations apart
__device__ __forceinline__ int csl_bin(float a, const Label& c) {
  const float v = ((a * (float)(180.0 / M_PI)) + 45.f) / c.omega;
  if (!(fabsf(v) < 2e9f)) return 0;
  const int m = (int)v % c.L;
  return m < 0 ? m + c.L : m;
}

// label of bin j for the target bin t (both in [0, L)), in double
__device__ __forceinline__ double csl_label(const Label& c, int t, int j) {
  int d = j - t;
  if (d < 0) d += c.L;
  switch (c.window) {
    case JDET_CSL_PULSE:
      return d == 0 ? 1.0 : 0.0;
    case JDET_CSL_RECT:
      return d < c.radius || d >= c.L - c.radius ? 1.0 : 0.0;
    case JDET_CSL_TRIANGLE: {
      const int b = d < c.radius ? d : c.L - d;   // |b|
      return b <= c.radius ? 1.0 - (double)b / (double)c.radius : 0.0;
    }
    default: {
      const int cd = d < c.L - d ? d : c.L - d;
      return exp(-(double)(cd * cd) * c.scale);
    }
  }
}

__global__ __launch_bounds__(256) void csl_encode_kernel(const float* __restrict__ angle, int n_el, Label c,
                                                         float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long)gridDim.x * 256) {   // n_el < 2^31; i + step not
    const int row = (int)(i / c.L);
    out[i] = (float)csl_label(c, csl_bin(angle[row], c), (int)(i - (long)row * c.L));
  }
}

// one wave per output row: lane-local first maximum over lane, lane + 64, ..., then the butterfly with ties to the
// smaller index
__global__ __launch_bounds__(256) void csl_decode_kernel(const float* __restrict__ logits, long rows,
                                                         const int64_t* __restrict__ index, long n, int L, double omega,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (long)gridDim.x * 4) {
    const long r = index ? (long)index[i] : i;
    if (r < 0 || r >= rows) {   // wave-uniform
      if (lane == 0) out[i] = __int_as_float(0x7FC00000);
      continue;
    }
    const float* x = logits + r * L;
    float best = -INFINITY;
    int at = L;
    for (int j = lane; j < L; j += 64) {
      const float v = x[j];
      if (v > best || (v == best && j < at)) { best = v; at = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oa = __shfl_xor(at, off, 64);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) {
      const int idx = at < L ? at : 0;
      out[i] = (float)((fmod(((double)idx + 0.5) * omega, 180.0) - 45.0) * (M_PI / 180.0));
    }
  }
}

__global__ __launch_bounds__(256) void csl_loss_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                       Blocked tb, const float* __restrict__ weight, Blocked wb,
                                                       long rows, Label c, float gamma_f, float alpha_f,
                                                       float* __restrict__ grad, double* __restrict__ partial) {
  __shared__ int s_bin[kTileRows];   // the target bin of a selected row, -1 of the others
  __shared__ double s_part[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, L = c.L;
  const double gamma = (double)gamma_f, alpha = (double)alpha_f;
  const long n_tiles = (rows + kTileRows - 1) / kTileRows;
  const bool vec = ((uintptr_t)grad & 15) == 0;   // a tile starts a multiple of 256 bytes behind `grad`
  double acc = 0.0;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long row0 = tile * kTileRows;
    const int n_rows = (int)(rows - row0 < kTileRows ? rows - row0 : kTileRows);
    int bin = -1;
    if (t < n_rows) {
      const long r = row0 + t;
      if (weight[blocked_row(wb, r) * 5 + 4] > 0.f) bin = csl_bin(target[blocked_row(tb, r) * 5 + 4], c);
    }
    if (t < kTileRows) s_bin[t] = bin;
    const bool any = __syncthreads_or(bin >= 0) != 0;
    // ---- zeros of the unselected rows over the tile's contiguous span
    float* g = grad + row0 * L;
    const int n_el = n_rows * L, n4 = vec ? n_el >> 2 : 0;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!any) {
      for (int i = t; i < n4; i += 256) reinterpret_cast<float4*>(g)[i] = z4;
      for (int e = n4 * 4 + t; e < n_el; e += 256) g[e] = 0.f;
    } else {
      for (int i = t; i < n4; i += 256) {
        int r = (i * 4) / L, rem = i * 4 - r * L, n_sel = 0;
        bool sel[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          sel[k] = s_bin[r] >= 0;
          n_sel += sel[k];
          if (++rem == L) {
            rem = 0;
            r = r + 1 < kTileRows ? r + 1 : r;   // behind the tile's last element: never looked at again
          }
        }
        if (n_sel == 0) {
          reinterpret_cast<float4*>(g)[i] = z4;
        } else {
#pragma unroll
          for (int k = 0; k < 4; k++)
            if (!sel[k]) g[i * 4 + k] = 0.f;
        }
      }
      for (int e = n4 * 4 + t; e < n_el; e += 256)
        if (s_bin[e / L] < 0) g[e] = 0.f;
      // ---- the selected rows: one wave each, lanes over the bins
      for (int r = wave; r < n_rows; r += 4) {
        const int tbin = s_bin[r];
        if (tbin < 0) continue;
        const float* x = logits + (row0 + r) * L;
        float* gr = g + r * L;
        for (int j = lane; j < L; j += 64) {
          const double xv = (double)x[j], y = csl_label(c, tbin, j);
          const double e = exp(-fabs(xv)), inv = 1.0 / (1.0 + e);
          const double p = xv >= 0.0 ? inv : e * inv, q = xv >= 0.0 ? e * inv : inv;
          const double bce = (xv > 0.0 ? xv : 0.0) - xv * y + log1p(e);
          const double pt = q * y + p * (1.0 - y), aw = alpha * y + (1.0 - alpha) * (1.0 - y);
          double ptg = 1.0, ptg1 = 0.0;   // pt^gamma, pt^(gamma - 1); gamma == 0: the first gradient term is absent
          if (gamma_f == 1.f) {
            ptg = pt, ptg1 = 1.0;
          } else if (gamma_f == 2.f) {
            ptg = pt * pt, ptg1 = pt;
          } else if (gamma_f != 0.f) {
            ptg1 = pow(pt, gamma - 1.0), ptg = ptg1 * pt;
          }
          acc += bce * aw * ptg;
          gr[j] = (float)(aw * (gamma * ptg1 * p * q * (1.0 - 2.0 * y) * bce + ptg * (p * (1.0 - y) - q * y)));
        }
      }
    }
    __syncthreads();   // s_bin is rewritten by the next tile
  }
  const double sum = jdet_block_sum4(acc, s_part);
  if (t == 0) partial[blockIdx.x] = sum;
}

// second stage: thread t adds partial[t], partial[t + 256], ...; (sum / *avg_factor) * loss_weight, rounded once
__global__ __launch_bounds__(256) void csl_finish_kernel(const double* __restrict__ partial, int n,
                                                         const float* __restrict__ avg_factor, float loss_weight,
                                                         float* __restrict__ out) {
  __shared__ double s_part[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const double total = jdet_block_sum4(acc, s_part);
  if (threadIdx.x == 0) out[0] = (float)((total / (double)avg_factor[0]) * (double)loss_weight);
}

bool finite_d(double v) { return v == v && v - v == 0.0; }

// the label parameters -> status and the kernels' form of them; radius is ignored by PULSE
int make_label(int L, double omega, int window, double radius, Label* out) {
  if (L < 1 || !finite_d(omega) || !(omega > 0.0) || !((float)omega > 0.f)) return JDET_E_BADARG;
  Label c{window, L, 0, 0.0, (float)omega};
  switch (window) {
    case JDET_CSL_PULSE:
      break;
    case JDET_CSL_RECT:
    case JDET_CSL_TRIANGLE:
      if (!finite_d(radius) || radius < 1.0 || radius != (double)(int)radius || 2.0 * radius > (double)L)
        return JDET_E_BADARG;
      c.radius = (int)radius;
      break;
    case JDET_CSL_GAUSSIAN:
      if (!finite_d(radius) || !(radius > 0.0)) return JDET_E_BADARG;
      c.scale = 1.0 / (2.0 * radius * radius);
      break;
    default:
      return JDET_E_BADARG;
  }
  if (L > JDET_CSL_MAX_BINS) return JDET_E_UNSUPPORTED;
  *out = c;
  return JDET_OK;
}

}  // namespace

JDET_API int jdet_csl_encode(const float* angle, long n, int coding_len, double omega, int window, double radius,
                             float* labels_out, jdet_stream_t stream) {
  Label c;
  if (n < 0) return JDET_E_BADARG;
  if (int e = make_label(coding_len, omega, window, radius, &c)) return e;
  if (n == 0) return JDET_OK;
  if (!angle || !labels_out) return JDET_E_BADARG;
  if (n * coding_len >= 2147483647L) return JDET_E_UNSUPPORTED;
  const int n_el = (int)(n * coding_len);
  const int grid = jdet_cdiv(n_el, 256) > 4096 ? 4096 : jdet_cdiv(n_el, 256);
  hipLaunchKernelGGL(csl_encode_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, angle, n_el, c, labels_out);
  return jdet_launch_status();
}

JDET_API int jdet_csl_decode(const float* logits, long rows, const int64_t* index, long n, int coding_len, double omega,
                             float* angle_out, jdet_stream_t stream) {
  Label c;
  if (n < 0 || rows < 0 || (!index && n > rows)) return JDET_E_BADARG;
  if (int e = make_label(coding_len, omega, JDET_CSL_PULSE, 0.0, &c)) return e;
  if (n == 0) return JDET_OK;
  if (!logits || !angle_out) return JDET_E_BADARG;
  if (n >= 2147483647L) return JDET_E_UNSUPPORTED;
  const int grid = jdet_cdiv(n, 4) > 4096 ? 4096 : jdet_cdiv(n, 4);
  hipLaunchKernelGGL(csl_decode_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, rows, index, n, coding_len,
                     omega, angle_out);
  return jdet_launch_status();
}

JDET_API int jdet_csl_angle_loss_level(const float* logits, const float* target, long target_rows_per_block,
                                       long target_block_stride, const float* weight, long weight_rows_per_block,
                                       long weight_block_stride, long rows, int coding_len, double omega, int window,
                                       double radius, float gamma, float alpha, const float* avg_factor,
                                       float loss_weight, float* loss, float* grad_logits, void* workspace,
                                       size_t workspace_bytes, jdet_stream_t stream) {
  Label c;
  if (rows < 0 || !loss || !finite_d(gamma) || gamma < 0.f || !finite_d(alpha) || !finite_d(loss_weight))
    return JDET_E_BADARG;
  if (int e = make_label(coding_len, omega, window, radius, &c)) return e;
  if (gamma > 0.f && gamma < 1.f) return JDET_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) return jdet_zero_async(loss, sizeof(float), st);
  if (!logits || !target || !weight || !avg_factor || !grad_logits || !workspace) return JDET_E_BADARG;
  if (target_rows_per_block <= 0 || target_block_stride < 0 || weight_rows_per_block <= 0 || weight_block_stride < 0)
    return JDET_E_BADARG;
  if (rows > (1L << 40) / coding_len) return JDET_E_UNSUPPORTED;
  if (workspace_bytes < kJdetLossWorkspaceBytes) return JDET_E_WORKSPACE;
  if ((uintptr_t)workspace & 7) return JDET_E_BADARG;
  const long tiles = (rows + kTileRows - 1) / kTileRows;
  const int grid = (int)(tiles > kSumGridCap ? kSumGridCap : tiles);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(csl_loss_kernel, dim3(grid), dim3(256), 0, st, logits, target,
                     Blocked{target_rows_per_block, target_block_stride}, weight,
                     Blocked{weight_rows_per_block, weight_block_stride}, rows, c, gamma, alpha, grad_logits, partial);
  if (int e = jdet_launch_status()) return e;
  hipLaunchKernelGGL(csl_finish_kernel, dim3(1), dim3(256), 0, st, partial, grid, avg_factor, loss_weight, loss);
  return jdet_launch_status();
}
