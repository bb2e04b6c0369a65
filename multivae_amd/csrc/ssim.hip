// Structural similarity and squared error of image batches (multivae/metrics/reconstruction/reconstruction.py hands the SSIM to
// torchmetrics.image.StructuralSimilarityIndexMeasure and sums (output - data)^2 in torch).  The definition is in DESIGN.md
// ("Metrics: the SSIM definition") and include/mvk.h: a per-update data range R, c1 = (0.01 R)^2, c2 = (0.03 R)^2, an 11-tap
// Gaussian (sigma 1.5) applied per channel as an outer product, only the (H - 10) x (W - 10) positions whose window lies inside the
// image, no clamping of the variances, the mean over C (H - 10) (W - 10) positions per image.
//
// Layout of the work
//  * Range: a capped grid strides over both tensors (16-byte loads when both are aligned), every workgroup leaves {min p, max p,
//    min t, max t} in caller-owned scratch and a one-wave kernel folds them into R.  Minimum and maximum do not depend on the order;
//    a NaN anywhere makes R NaN, as torch's max() and min() do.
//  * Rows: one workgroup per (image, channel, tile).  A tile is up to SSIM_T x SSIM_T window positions; its (h + 10) x (w + 10)
//    pixels of both images are staged in LDS once (a plane that fits one tile -- every shipped dataset -- is one contiguous copy),
//    and the squared differences of the pixels the tile owns are summed in fp64 on the way.  The filter is separable and is applied
//    in two passes through LDS, horizontal then vertical.
//  * Precision.  E[x^2] - mu^2 in fp32 loses the variance of a flat bright region (it is the difference of two numbers near 0.5
//    that agree to 1e-8), so no raw second moment is ever formed.  The weighted variance of a window is split by rows,
//        var = sum_y g_y [ v_y + (m_y - mu)^2 ],   m_y = sum_x g_x x_yx,   v_y = sum_x g_x (x_yx - m_y)^2,   mu = sum_y g_y m_y
//    (the law of total variance; exact for weights that sum to 1), and likewise the covariance.  The horizontal pass leaves m_y, v_y
//    and the row covariance per (row, window column), centred on the row's own mean; the vertical pass centres the row means on the
//    window mean.  Every mean is taken as first tap + sum g (x - first tap): a constant window has deviations that are exactly zero,
//    so R = 0 gives 0 / 0 = NaN as the formula does, without a special case.
//  * Determinism: per-thread sums in a fixed order, a fixed-order fp64 workgroup sum, one partial per workgroup in scratch, and one
//    wave per image that adds the partials in a fixed order.  No floating-point atomics.
//  * Accumulate: one workgroup adds the rows of an update, in index order and in fp64, into the caller's {ssim_sum, sse_sum, rows}.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int SSIM_T = 32;                // window positions per tile edge
constexpr int SSIM_IN = SSIM_T + 10;      // pixels per tile edge, halo included
constexpr int SSIM_TPB = 256;
constexpr int RANGE_GRID_CAP = 256;       // range partials: 4 floats per workgroup, the first 4 KiB of the scratch
constexpr long long RANGE_BYTES = (long long)RANGE_GRID_CAP * 4 * sizeof(float);

struct SsimTaps {
  float g[11];
};

// fixed-order fp64 workgroup sum (thread 0 adds the per-wave sums in wave order); valid in thread 0
__device__ __forceinline__ double ssim_block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < SSIM_TPB / 64; ++w) s += lds[w];
  __syncthreads();
  return s;
}

struct MinMax {
  float lo, hi;
  bool nan;
  __device__ __forceinline__ void add(float v) {
    nan |= v != v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
};

// part[block] = {min p, max p, min t, max t}; a NaN input makes the workgroup's four values NaN
__global__ __launch_bounds__(SSIM_TPB) void ssim_range_kernel(const float* __restrict__ p, const float* __restrict__ t, long long n,
                                                              int vec, float* __restrict__ part) {
  __shared__ float red[4][SSIM_TPB / 64];
  __shared__ int rnan[SSIM_TPB / 64];
  MinMax a{INFINITY, -INFINITY, false}, b{INFINITY, -INFINITY, false};
  const long long stride = (long long)gridDim.x * SSIM_TPB;
  long long i = (long long)blockIdx.x * SSIM_TPB + threadIdx.x;
  if (vec) {
    const long long n4 = n >> 2;
    for (long long e = i; e < n4; e += stride) {
      const float4 x = reinterpret_cast<const float4*>(p)[e], y = reinterpret_cast<const float4*>(t)[e];
      a.add(x.x), a.add(x.y), a.add(x.z), a.add(x.w);
      b.add(y.x), b.add(y.y), b.add(y.z), b.add(y.w);
    }
    i += n4 << 2;  // the tail of fewer than four elements
  }
  for (long long e = i; e < n; e += stride) {
    a.add(p[e]);
    b.add(t[e]);
  }
  float v[4] = {a.lo, -a.hi, b.lo, -b.hi};  // four minima
  int bad = (a.nan || b.nan) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fminf(v[k], __shfl_xor(v[k], off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = v[k];
    rnan[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float m = red[threadIdx.x][0];
    int any = rnan[0];
    for (int w = 1; w < SSIM_TPB / 64; ++w) {
      m = fminf(m, red[threadIdx.x][w]);
      any |= rnan[w];
    }
    if (threadIdx.x & 1) m = -m;
    part[blockIdx.x * 4 + threadIdx.x] = any ? NAN : m;
  }
}

// R = max(max p - min p, max t - min t) in fp32 (one wave)
__global__ __launch_bounds__(64) void ssim_range_finish_kernel(const float* __restrict__ part, int G, float* __restrict__ range) {
  float v[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int bad = 0;
  for (int g = threadIdx.x; g < G; g += 64) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = part[g * 4 + k];
      bad |= x != x;
      v[k] = fminf(v[k], (k & 1) ? -x : x);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fminf(v[k], __shfl_xor(v[k], off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  if (threadIdx.x == 0) range[0] = bad ? NAN : fmaxf(-v[1] - v[0], -v[3] - v[2]);
}

// One workgroup per (image b, channel c, tile): part[(b C + c) ntiles + tile] = {sum of the tile's SSIM positions, sum of the
// squared differences of the pixels the tile owns}.
__global__ __launch_bounds__(SSIM_TPB) void ssim_tile_kernel(const float* __restrict__ preds, const float* __restrict__ target,
                                                             int H, int W, int tiles_x, int ntiles, SsimTaps taps,
                                                             const float* __restrict__ range_dev, float range_val,
                                                             double* __restrict__ part) {
  __shared__ float P[SSIM_IN * SSIM_IN], Tg[SSIM_IN * SSIM_IN];
  __shared__ float MP[SSIM_IN * SSIM_T], MT[SSIM_IN * SSIM_T], VP[SSIM_IN * SSIM_T], VT[SSIM_IN * SSIM_T], CV[SSIM_IN * SSIM_T];
  __shared__ double red[SSIM_TPB / 64];
  const int tid = threadIdx.x;
  const long long plane = (long long)blockIdx.x / ntiles;  // b C + c
  const int tile = (int)((long long)blockIdx.x - plane * ntiles);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * SSIM_T, x0 = tx * SSIM_T;
  const int oh = min(SSIM_T, H - 10 - y0), ow = min(SSIM_T, W - 10 - x0);  // window positions of this tile
  const int ih = oh + 10, iw = ow + 10;                                    // its pixels
  const bool last_y = y0 + oh == H - 10, last_x = x0 + ow == W - 10;       // the last tile of a direction owns its halo
  const float* gp = preds + plane * H * W;
  const float* gt = target + plane * H * W;

  // stage the tile (LDS row stride iw) and sum the squared differences of the owned pixels
  double sse = 0.0;
  const int npix = ih * iw;
  if (iw == W) {  // the tile spans whole rows: one contiguous run
    const long long base = (long long)y0 * W;
    for (int e = tid; e < npix; e += SSIM_TPB) {
      const float a = gp[base + e], b = gt[base + e];
      P[e] = a;
      Tg[e] = b;
      if (last_y || e < SSIM_T * iw) {
        const double d = (double)a - (double)b;
        sse = fma(d, d, sse);
      }
    }
  } else {
    for (int e = tid; e < npix; e += SSIM_TPB) {
      const int r = e / iw, c = e - r * iw;
      const long long o = (long long)(y0 + r) * W + x0 + c;
      const float a = gp[o], b = gt[o];
      P[e] = a;
      Tg[e] = b;
      if ((last_y || r < SSIM_T) && (last_x || c < SSIM_T)) {
        const double d = (double)a - (double)b;
        sse = fma(d, d, sse);
      }
    }
  }
  __syncthreads();

  // horizontal pass: per (row r, window column x) the row mean, the row variance and the row covariance, centred on the row mean
  for (int e = tid; e < ih * ow; e += SSIM_TPB) {
    const int r = e / ow, x = e - r * ow;
    const float* pr = &P[r * iw + x];
    const float* tr = &Tg[r * iw + x];
    const float p0 = pr[0], t0 = tr[0];
    float dp[11], dt[11];
    float sp = 0.f, st = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      dp[k] = pr[k] - p0;
      dt[k] = tr[k] - t0;
      sp = fmaf(taps.g[k], dp[k], sp);
      st = fmaf(taps.g[k], dt[k], st);
    }
    float vp = 0.f, vt = 0.f, cv = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float a = dp[k] - sp, b = dt[k] - st;
      vp = fmaf(taps.g[k] * a, a, vp);
      vt = fmaf(taps.g[k] * b, b, vt);
      cv = fmaf(taps.g[k] * a, b, cv);
    }
    MP[e] = p0 + sp;
    MT[e] = t0 + st;
    VP[e] = vp;
    VT[e] = vt;
    CV[e] = cv;
  }
  __syncthreads();

  // vertical pass and the SSIM of every position
  const float R = range_dev ? range_dev[0] : range_val;
  const float k1 = 0.01f * R, k2 = 0.03f * R;
  const float c1 = k1 * k1, c2 = k2 * k2;
  float acc = 0.f;
  for (int e = tid; e < oh * ow; e += SSIM_TPB) {
    const int y = e / ow, x = e - y * ow;
    const int o = y * ow + x;
    const float p0 = MP[o], t0 = MT[o];
    float dp[11], dt[11];
    float sp = 0.f, st = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      dp[k] = MP[o + k * ow] - p0;
      dt[k] = MT[o + k * ow] - t0;
      sp = fmaf(taps.g[k], dp[k], sp);
      st = fmaf(taps.g[k], dt[k], st);
    }
    float vp = 0.f, vt = 0.f, cv = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float a = dp[k] - sp, b = dt[k] - st;
      vp = fmaf(taps.g[k], fmaf(a, a, VP[o + k * ow]), vp);
      vt = fmaf(taps.g[k], fmaf(b, b, VT[o + k * ow]), vt);
      cv = fmaf(taps.g[k], fmaf(a, b, CV[o + k * ow]), cv);
    }
    const float mp = p0 + sp, mt = t0 + st;
    const float num = (2.f * mp * mt + c1) * (2.f * cv + c2);
    const float den = (mp * mp + mt * mt + c1) * (vp + vt + c2);
    acc += num / den;
  }
  const double s_ssim = ssim_block_sum((double)acc, red);
  const double s_sse = ssim_block_sum(sse, red);
  if (tid == 0) {
    part[2 * (long long)blockIdx.x] = s_ssim;
    part[2 * (long long)blockIdx.x + 1] = s_sse;
  }
}

// one wave per image: the partials of its C ntiles workgroups in a fixed order
__global__ __launch_bounds__(64) void ssim_rows_kernel(const double* __restrict__ part, int per_image, double positions,
                                                       float* __restrict__ ssim_rows, float* __restrict__ sse_rows) {
  const double* p = part + 2 * (long long)blockIdx.x * per_image;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < per_image; i += 64) {
    a += p[2 * i];
    b += p[2 * i + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if (threadIdx.x == 0) {
    ssim_rows[blockIdx.x] = (float)(a / positions);
    sse_rows[blockIdx.x] = (float)b;
  }
}

// the squared-error-only path: one workgroup per row of D elements, no windows
__global__ __launch_bounds__(SSIM_TPB) void sse_rows_kernel(const float* __restrict__ preds, const float* __restrict__ target,
                                                            long long D, float* __restrict__ sse_rows) {
  __shared__ double red[SSIM_TPB / 64];
  const float* p = preds + (long long)blockIdx.x * D;
  const float* t = target + (long long)blockIdx.x * D;
  double s = 0.0;
  for (long long e = threadIdx.x; e < D; e += SSIM_TPB) {
    const double d = (double)p[e] - (double)t[e];
    s = fma(d, d, s);
  }
  s = ssim_block_sum(s, red);
  if (threadIdx.x == 0) sse_rows[blockIdx.x] = (float)s;
}

// acc = {ssim_sum, sse_sum, rows} += the rows of one update, in index order (one workgroup; thread 0 adds from LDS)
__global__ __launch_bounds__(SSIM_TPB) void ssim_accumulate_kernel(const float* __restrict__ ssim_rows,
                                                                   const float* __restrict__ sse_rows, int B,
                                                                   double* __restrict__ acc) {
  __shared__ float a[SSIM_TPB], b[SSIM_TPB];
  double s0 = 0.0, s1 = 0.0;
  for (int r0 = 0; r0 < B; r0 += SSIM_TPB) {
    const int n = min(SSIM_TPB, B - r0);
    __syncthreads();
    if ((int)threadIdx.x < n) {
      a[threadIdx.x] = ssim_rows ? ssim_rows[r0 + threadIdx.x] : 0.f;
      b[threadIdx.x] = sse_rows[r0 + threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) {
        s0 += (double)a[i];
        s1 += (double)b[i];
      }
  }
  if (threadIdx.x == 0) {
    if (ssim_rows) acc[MVK_SSIM_ACC_SSIM] += s0;
    acc[MVK_SSIM_ACC_SSE] += s1;
    acc[MVK_SSIM_ACC_ROWS] += (double)B;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
bool ssim_shape_ok(int B, int C, int H, int W) { return B > 0 && C > 0 && H >= 11 && W >= 11; }

int ssim_tiles(int n) { return (n - 10 + SSIM_T - 1) / SSIM_T; }

// workgroups of the rows kernel; 0 when the grid does not fit 31 bits
long long ssim_blocks(int B, int C, int H, int W) {
  const long long n = (long long)B * C * ssim_tiles(H) * ssim_tiles(W);
  return n <= 0x7fffffffLL ? n : 0;
}

SsimTaps ssim_taps() {
  SsimTaps t;
  double g[11], s = 0.0;
  for (int i = 0; i < 11; ++i) {
    const double d = (i - 5) / 1.5;
    g[i] = exp(-0.5 * d * d);
    s += g[i];
  }
  for (int i = 0; i < 11; ++i) t.g[i] = (float)(g[i] / s);
  return t;
}

}  // namespace

extern "C" {

int mvk_ssim_tile(void) { return SSIM_T; }

int mvk_ssim_scratch_bytes(int B, int C, int H, int W, int64_t* bytes) {
  if (!bytes || !ssim_shape_ok(B, C, H, W)) return MVK_EINVAL;
  const long long blocks = ssim_blocks(B, C, H, W);
  if (!blocks) return MVK_EINVAL;
  *bytes = RANGE_BYTES + blocks * 2 * (int64_t)sizeof(double);
  return MVK_OK;
}

int mvk_ssim_range(const float* preds, const float* target, int64_t n, float* range, void* scratch, void* stream) {
  if (!preds || !target || !range || !scratch || n <= 0) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  float* part = static_cast<float*>(scratch);
  const long long want = (n / 4 + SSIM_TPB - 1) / SSIM_TPB;
  const int G = (int)(want < 1 ? 1 : (want < RANGE_GRID_CAP ? want : RANGE_GRID_CAP));
  const int vec = mvk_aligned16(preds) && mvk_aligned16(target);
  hipLaunchKernelGGL(ssim_range_kernel, dim3(G), dim3(SSIM_TPB), 0, s, preds, target, (long long)n, vec, part);
  MVK_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_range_finish_kernel, dim3(1), dim3(64), 0, s, part, G, range);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_ssim_rows(const float* preds, const float* target, int B, int C, int H, int W, const float* range_dev, float range_val,
                  int mse_only, float* ssim_rows, float* sse_rows, void* scratch, void* stream) {
  if (!preds || !target || !sse_rows || B <= 0 || C <= 0 || H <= 0 || W <= 0) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  if (mse_only) {
    hipLaunchKernelGGL(sse_rows_kernel, dim3(B), dim3(SSIM_TPB), 0, s, preds, target, (long long)C * H * W, sse_rows);
    MVK_CHECK_LAUNCH();
    return MVK_OK;
  }
  if (!ssim_rows || !scratch || !ssim_shape_ok(B, C, H, W)) return MVK_EINVAL;
  const long long blocks = ssim_blocks(B, C, H, W);
  if (!blocks) return MVK_EINVAL;
  const int tiles_x = ssim_tiles(W), ntiles = tiles_x * ssim_tiles(H);
  double* part = reinterpret_cast<double*>(static_cast<char*>(scratch) + RANGE_BYTES);
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)blocks), dim3(SSIM_TPB), 0, s, preds, target, H, W, tiles_x, ntiles,
                     ssim_taps(), range_dev, range_val, part);
  MVK_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_rows_kernel, dim3(B), dim3(64), 0, s, part, C * ntiles, (double)C * (H - 10) * (W - 10), ssim_rows,
                     sse_rows);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_ssim_accumulate(const float* ssim_rows, const float* sse_rows, int B, double* acc, void* stream) {
  if (!sse_rows || !acc || B <= 0) return MVK_EINVAL;
  hipLaunchKernelGGL(ssim_accumulate_kernel, dim3(1), dim3(SSIM_TPB), 0, mvk_stream(stream), ssim_rows, sse_rows, B, acc);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
