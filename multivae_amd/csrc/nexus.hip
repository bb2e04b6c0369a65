// Nexus (Vasco et al. 2022; multivae/models/nexus/nexus_model.py): the two pieces of new math of the two-level model.
//  * the aggregation of the modality messages (:209-254): a per-row mean over the kept modalities, the keep set coming from the
//    dataset masks, an explicit keep matrix or -- forced perceptual dropout (FPD) -- decided here from uniforms, so that a
//    captured training step draws fresh dropout subsets at every replay;
//  * the top-level likelihood -log N(z_m | r_m, s_m) of the detached first-level latents (:153-168), s_m = 1 or the adapted
//    scale sqrt(mean((z_m - r_m)^2)) over the whole [B, D_m] block, with the gradient through s_m.  The block reductions are
//    fixed-order two-stage sums (no floating-point atomics): the step is bit-reproducible.
#include <math.h>

#include "common.hpp"

namespace {

struct NexusPtrs {
  const float* p[MVK_MAX_MODALITIES];
};
struct NexusOutPtrs {
  float* p[MVK_MAX_MODALITIES];
};
struct NexusMasks {
  const uint8_t* p[MVK_MAX_MODALITIES];
};

// The keep set of row b (1.f kept, 0.f dropped / missing) from one of the three sources.
__device__ __forceinline__ void nexus_keep(const NexusMasks& masks, const float* keep_in, const float* u, float p, int M,
                                           int b, float* keep) {
#pragma unroll
  for (int m = 0; m < MVK_MAX_MODALITIES; ++m) keep[m] = m < M ? 1.f : 0.f;
  if (keep_in) {
    for (int m = 0; m < M; ++m) keep[m] = keep_in[(long long)b * M + m] != 0.f ? 1.f : 0.f;
  } else if (masks.p[0]) {
    for (int m = 0; m < M; ++m) keep[m] = masks.p[m][b] ? 1.f : 0.f;
  } else if (u) {
    // u[b] = {u0, u1, u2 .. u_M}: dropped when u0 < p; subset size 1 + floor(u1 (M - 1)) on [1, M - 1]; the kept modalities are
    // the first `size` entries of a partial Fisher-Yates shuffle of 0 .. M-1 driven by u2 ...
    const float* ub = u + (long long)b * (M + 1);
    if (ub[0] < p && M > 1) {
      int size = 1 + (int)floorf(ub[1] * (float)(M - 1));
      size = size < 1 ? 1 : (size > M - 1 ? M - 1 : size);
      int perm[MVK_MAX_MODALITIES];
#pragma unroll
      for (int m = 0; m < MVK_MAX_MODALITIES; ++m) perm[m] = m;
      for (int i = 0; i < size; ++i) {
        int j = i + (int)floorf(ub[2 + i] * (float)(M - i));
        j = j > M - 1 ? M - 1 : j;
        const int t = perm[i];
        perm[i] = perm[j];
        perm[j] = t;
      }
      for (int m = 0; m < M; ++m) keep[m] = 0.f;
      for (int i = 0; i < size; ++i) keep[perm[i]] = 1.f;
    }
  }
}

// One wave per row: agg[b] = sum_m keep[b,m] msg_m[b] / count[b] (0 for a row with nothing kept), keep_out[b] = the keep set.
__global__ __launch_bounds__(256) void nexus_aggregate_fwd_kernel(NexusPtrs msgs, NexusMasks masks, const float* keep_in,
                                                                  const float* u, float p, int M, int B, int D,
                                                                  float* __restrict__ agg, float* __restrict__ keep_out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  float keep[MVK_MAX_MODALITIES];
  nexus_keep(masks, keep_in, u, p, M, b, keep);
  float count = 0.f;
  for (int m = 0; m < M; ++m) count += keep[m];
  const float inv = count > 0.f ? 1.f / count : 0.f;
  for (int d = lane; d < D; d += 64) {
    float s = 0.f;
    for (int m = 0; m < M; ++m)
      if (keep[m] != 0.f) s += msgs.p[m][(long long)b * D + d];
    agg[(long long)b * D + d] = s * inv;
  }
  if (lane < M) keep_out[(long long)b * M + lane] = keep[lane];
}

// d msg_m[b, d] = keep[b, m] / count[b] * g[b, d]: exactly 0 for a dropped or missing modality.
__global__ __launch_bounds__(256) void nexus_aggregate_bwd_kernel(const float* __restrict__ keep, const float* __restrict__ g,
                                                                  int M, int B, int D, NexusOutPtrs dmsgs) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= (long long)B * D) return;
  const int b = (int)(o / D);
  float count = 0.f;
  for (int m = 0; m < M; ++m) count += keep[(long long)b * M + m];
  const float gi = count > 0.f ? g[o] / count : 0.f;
  for (int m = 0; m < M; ++m) dmsgs.p[m][o] = keep[(long long)b * M + m] != 0.f ? gi : 0.f;
}

struct NexusTop {
  const float* z[MVK_MAX_MODALITIES];
  const float* r[MVK_MAX_MODALITIES];
  const uint8_t* mask[MVK_MAX_MODALITIES];
  float* rows[MVK_MAX_MODALITIES];
  const float* grows[MVK_MAX_MODALITIES];
  float* dr[MVK_MAX_MODALITIES];
  int D[MVK_MAX_MODALITIES];
  float gamma[MVK_MAX_MODALITIES];
  int adapt[MVK_MAX_MODALITIES];
};

// 256 values of a workgroup -> their sum, in a fixed order (LDS tree); every thread returns it.
__device__ __forceinline__ float block_sum_fixed(float v, float* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  const float r = lds[0];
  __syncthreads();
  return r;
}

// Stage 1 (grid: row blocks x modalities): q[m][b] = sum_d (z - r)^2, one wave per row; part[m][blk] = the sum over the block's
// four rows in row order.
__global__ __launch_bounds__(256) void nexus_top_rows_kernel(NexusTop t, int B, float* __restrict__ q, float* __restrict__ part) {
  __shared__ float wsum[4];
  const int m = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  const int D = t.D[m];
  float s = 0.f;
  if (b < B) {
    const float* z = t.z[m] + (long long)b * D;
    const float* r = t.r[m] + (long long)b * D;
    for (int d = lane; d < D; d += 64) {
      const float e = z[d] - r[d];
      s += e * e;
    }
  }
  s = wave_sum(s);
  if (lane == 0) {
    wsum[w] = s;
    if (b < B) q[(long long)m * B + b] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) part[(long long)m * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// Stage 2 (one workgroup per modality): s2[m] = mean (z - r)^2 over the block (adapted) or 1, then
// rows[m][b] = gamma mask (q / (2 s2) + D/2 ln s2 + D/2 ln 2 pi).
__global__ __launch_bounds__(256) void nexus_top_finish_kernel(NexusTop t, int B, int nparts, const float* __restrict__ q,
                                                               const float* __restrict__ part, float* __restrict__ s2out) {
  __shared__ float lds[256];
  const int m = blockIdx.x;
  const int D = t.D[m];
  float s2 = 1.f;
  if (t.adapt[m]) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[(long long)m * nparts + i];
    s2 = block_sum_fixed(s, lds) / ((float)B * (float)D);
  }
  if (threadIdx.x == 0) s2out[m] = s2;
  const float half_log = 0.5f * (float)D * (logf(s2) + 1.8378770664093453f);  // ln(2 pi)
  const float inv = 0.5f / s2;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float w = t.mask[m] && !t.mask[m][b] ? 0.f : t.gamma[m];
    t.rows[m][b] = w * (q[(long long)m * B + b] * inv + half_log);
  }
}

// Backward stage 1 (grid: row blocks of 256 x modalities, adapted modalities only): part[m][blk] = the block's share of
// C_m = sum_b g_b mask_b (D / (2 s2) - q_b / (2 s2^2)), d loss / d s2 = gamma C_m.
__global__ __launch_bounds__(256) void nexus_top_bwd_part_kernel(NexusTop t, int B, const float* __restrict__ q,
                                                                 const float* __restrict__ s2v, float* __restrict__ part) {
  __shared__ float lds[256];
  const int m = blockIdx.y;
  if (!t.adapt[m]) return;
  const int b = blockIdx.x * 256 + threadIdx.x;
  const float s2 = s2v[m];
  float c = 0.f;
  if (b < B && t.grows[m] && !(t.mask[m] && !t.mask[m][b]))
    c = t.grows[m][b] * (0.5f * (float)t.D[m] / s2 - 0.5f * q[(long long)m * B + b] / (s2 * s2));
  c = block_sum_fixed(c, lds);
  if (threadIdx.x == 0) part[(long long)m * gridDim.x + blockIdx.x] = c;
}

// Backward stage 2 (grid: element blocks x modalities): every workgroup adds the partials of C_m in the same order, then
// dr = -gamma (z - r) (g_b mask_b / s2 + 2 C_m / (B D)).
__global__ __launch_bounds__(256) void nexus_top_bwd_kernel(NexusTop t, int B, int nparts, const float* __restrict__ s2v,
                                                            const float* __restrict__ part) {
  __shared__ float lds[256];
  const int m = blockIdx.y;
  const int D = t.D[m];
  const long long n = (long long)B * D;
  if ((long long)blockIdx.x * 256 >= n) return;  // uniform per workgroup: the grid is sized for the widest modality
  float cterm = 0.f;
  if (t.adapt[m]) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[(long long)m * nparts + i];
    cterm = 2.f * block_sum_fixed(s, lds) / ((float)B * (float)D);
  }
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  const int b = (int)(o / D);
  const float gb = (t.grows[m] && !(t.mask[m] && !t.mask[m][b])) ? t.grows[m][b] : 0.f;
  t.dr[m][o] = -t.gamma[m] * (t.z[m][o] - t.r[m][o]) * (gb / s2v[m] + cterm);
}

}  // namespace

extern "C" {

int mvk_nexus_aggregate_fwd(const float* const* msgs, const uint8_t* const* masks, const float* keep_in, const float* u,
                            float dropout_rate, int M, int B, int D, float* agg, float* keep_out, void* stream) {
  if (B == 0) return MVK_OK;
  if (!msgs || !agg || !keep_out || M < 1 || M > MVK_MAX_MODALITIES || B < 0 || D < 1) return MVK_EINVAL;
  NexusPtrs mp{};
  NexusMasks mk{};
  for (int m = 0; m < M; ++m) {
    if (!msgs[m]) return MVK_EINVAL;
    mp.p[m] = msgs[m];
    if (masks) {
      if (!masks[m]) return MVK_EINVAL;
      mk.p[m] = masks[m];
    }
  }
  hipLaunchKernelGGL(nexus_aggregate_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, mvk_stream(stream), mp, mk, keep_in, u,
                     dropout_rate, M, B, D, agg, keep_out);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_nexus_aggregate_bwd(const float* keep, const float* g, int M, int B, int D, float* const* dmsgs, void* stream) {
  if (B == 0) return MVK_OK;
  if (!keep || !g || !dmsgs || M < 1 || M > MVK_MAX_MODALITIES || B < 0 || D < 1) return MVK_EINVAL;
  NexusOutPtrs op{};
  for (int m = 0; m < M; ++m) {
    if (!dmsgs[m]) return MVK_EINVAL;
    op.p[m] = dmsgs[m];
  }
  const long long n = (long long)B * D;
  hipLaunchKernelGGL(nexus_aggregate_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, mvk_stream(stream), keep,
                     g, M, B, D, op);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

static int nexus_top_fill(NexusTop& t, const float* const* z, const float* const* r, const uint8_t* const* masks,
                          const int* D, const float* gamma, const int* adapt, int M) {
  if (!z || !r || !D || !gamma || !adapt || M < 1 || M > MVK_MAX_MODALITIES) return MVK_EINVAL;
  for (int m = 0; m < M; ++m) {
    if (!z[m] || !r[m] || D[m] < 1) return MVK_EINVAL;
    t.z[m] = z[m];
    t.r[m] = r[m];
    t.mask[m] = masks ? masks[m] : nullptr;
    t.D[m] = D[m];
    t.gamma[m] = gamma[m];
    t.adapt[m] = adapt[m];
  }
  return MVK_OK;
}

int mvk_nexus_top_nll_fwd(const float* const* z, const float* const* r, const uint8_t* const* masks, const int* D,
                          const float* gamma, const int* adapt, int M, int B, float* const* rows, float* q, float* s2,
                          float* work, void* stream) {
  if (B == 0) return MVK_OK;
  NexusTop t{};
  int rc = nexus_top_fill(t, z, r, masks, D, gamma, adapt, M);
  if (rc != MVK_OK) return rc;
  if (!rows || !q || !s2 || !work || B < 0) return MVK_EINVAL;
  for (int m = 0; m < M; ++m) {
    if (!rows[m]) return MVK_EINVAL;
    t.rows[m] = rows[m];
  }
  const int nb = (B + 3) / 4;
  hipLaunchKernelGGL(nexus_top_rows_kernel, dim3(nb, M), dim3(256), 0, mvk_stream(stream), t, B, q, work);
  MVK_CHECK_LAUNCH();
  hipLaunchKernelGGL(nexus_top_finish_kernel, dim3(M), dim3(256), 0, mvk_stream(stream), t, B, nb, q, work, s2);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_nexus_top_nll_bwd(const float* const* z, const float* const* r, const uint8_t* const* masks, const int* D,
                          const float* gamma, const int* adapt, int M, int B, const float* const* grows, const float* q,
                          const float* s2, float* work, float* const* dr, void* stream) {
  if (B == 0) return MVK_OK;
  NexusTop t{};
  int rc = nexus_top_fill(t, z, r, masks, D, gamma, adapt, M);
  if (rc != MVK_OK) return rc;
  if (!grows || !q || !s2 || !work || !dr || B < 0) return MVK_EINVAL;
  int Dmax = 1, any_adapt = 0;
  for (int m = 0; m < M; ++m) {
    if (!dr[m]) return MVK_EINVAL;
    t.grows[m] = grows[m];
    t.dr[m] = dr[m];
    Dmax = D[m] > Dmax ? D[m] : Dmax;
    any_adapt |= adapt[m];
  }
  const int nb = (B + 255) / 256;
  if (any_adapt) {
    hipLaunchKernelGGL(nexus_top_bwd_part_kernel, dim3(nb, M), dim3(256), 0, mvk_stream(stream), t, B, q, s2, work);
    MVK_CHECK_LAUNCH();
  }
  const long long n = (long long)B * Dmax;
  hipLaunchKernelGGL(nexus_top_bwd_kernel, dim3((unsigned)((n + 255) / 256), M), dim3(256), 0, mvk_stream(stream), t, B, nb,
                     s2, work);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
