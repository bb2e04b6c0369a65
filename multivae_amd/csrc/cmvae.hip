// CMVAE (models/cmvae/cmvae_model.py): MMVAE+ whose shared-latent prior is a learnable mixture over C clusters.
// The reference takes an explicit expectation of lw under q(c|u) = softmax_c(log pi_c + log p(u|c)) (:292-337); up to its 1e-20
// that expectation is  sum_c q_c (a_c - log q_c) = logsumexp_c a_c  with  a_c = log pi_c + log p(u|c),  so the latent stage is the
// one of mmvae.hip (same launch shape, same per-row ownership) with the shared part of lpz replaced by the log-density of the
// mixture and the private part of the prior fixed at (0, wprior_std).  d lw / d a_c = beta q_c: the forward launch leaves the
// responsibilities q_c behind for the backward launch.  predict_clusters (:546-619) runs on cm_assign_kernel.
// That shared stage (mixture-of-experts posterior, its backward, pointer tables, common argument checks) is latent.hpp's; what is
// here is the mixture prior: the cluster table in LDS, the per-wave u, the cluster scores and the parameter rows of the backward.
// Like mmvae.hip these kernels are latency-bound (rows of 20-64 floats): few launches, deterministic reductions, no atomics.
#include "common.hpp"
#include "latent.hpp"

namespace {

constexpr int MAXC = MVK_CMVAE_MAX_CLUSTERS;
constexpr int CPL = (MAXC + 63) / 64;  // clusters per lane

// ---- the cluster table in LDS: mean [C][Lsp], sd [C][Lsp], log pi [C]; Lsp = Ls | 1 (an odd row stride: the lanes of a wave read
// one column of 64 different rows) -------------------------------------------------------------------------------------------------
__host__ __device__ inline int cm_stride(int Ls) { return Ls | 1; }
__host__ __device__ inline long long cm_table_floats(int C, int Ls) { return (long long)C * (2 * cm_stride(Ls) + 1); }

// all threads of the workgroup; ends with a barrier.  assign = 0: log pi = log_softmax(logits) (a logit of -inf gives -inf: the
// cluster is absent); assign = 1: log(softmax(logits) + 1e-20), the form of predict_clusters (:575).
__device__ __forceinline__ void cm_stage(float* tab, const float* __restrict__ cmean, const float* __restrict__ csd,
                                         const float* __restrict__ clogit, int C, int Ls, int assign) {
  const int Lsp = cm_stride(Ls);
  float* tm = tab;
  float* ts = tab + C * Lsp;
  float* tl = ts + C * Lsp;
  for (int i = threadIdx.x; i < C * Ls; i += blockDim.x) {
    const int j = i / Ls, l = i - j * Ls;
    tm[j * Lsp + l] = cmean[i];
    ts[j * Lsp + l] = csd[i];
  }
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    float mx = -INFINITY;
    for (int j = lane; j < C; j += 64) mx = fmaxf(mx, clogit[j]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int j = lane; j < C; j += 64) s += expf(clogit[j] - mx);
    s = wave_sum(s);
    const float ls = logf(s);
    for (int j = lane; j < C; j += 64)
      tl[j] = assign ? logf(expf(clogit[j] - mx) / s + 1e-20f) : (clogit[j] - mx) - ls;
  }
  __syncthreads();
}

// a[q] = log pi_j + sum_{l < Ls} log p(u_l; mean_jl, sd_jl) for the lane's clusters j = lane + 64 q (-inf beyond C): the sum over l
// runs in a fixed order inside one lane, no cross-lane step.  Returns the wave's max and sum of exp(a - max) in mx, s.
__device__ __forceinline__ void cm_scores(int family, const float* u, const float* tab, int C, int Ls, int lane, float a[CPL],
                                          float& mx, float& s) {
  const int Lsp = cm_stride(Ls);
  const float* tm = tab;
  const float* ts = tab + C * Lsp;
  const float* tl = ts + C * Lsp;
  mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int j = lane + 64 * q;
    a[q] = -INFINITY;
    if (j < C) {
      float acc = 0.f, lost = 0.f;  // compensated: one lane adds all Ls terms, a plain run would grow its error with Ls
      for (int l = 0; l < Ls; ++l) {
        const float y = lat_logp(family, u[l], tm[j * Lsp + l], ts[j * Lsp + l]) - lost;
        const float t = acc + y;
        lost = (t - acc) - y;
        acc = t;
      }
      a[q] = tl[j] + acc;
    }
    mx = fmaxf(mx, a[q]);
  }
  mx = wave_max(mx);
  s = 0.f;
#pragma unroll
  for (int q = 0; q < CPL; ++q)
    if (lane + 64 * q < C) s += expf(a[q] - mx);
  s = wave_sum(s);
}

// ---- forward: samples, mixture-prior log-density, responsibilities, mixture-of-experts posterior -----------------------------------
// one wave per (c, k, b); lanes over l for the posterior terms (latent.hpp), over the clusters for the prior
__global__ __launch_bounds__(256) void cm_latent_fwd_kernel(const LatFwdPtrs p, const float* __restrict__ cmean,
                                                            const float* __restrict__ csd,
                                                            const float* __restrict__ clogit,
                                                            const float* __restrict__ wsd, int M, int K, int B, int D,
                                                            int Ls, int C, int family) {
  extern __shared__ float cm_lds[];
  float* ubuf = cm_lds + cm_table_floats(C, Ls) + (threadIdx.x >> 6) * Ls;  // this wave's u
  cm_stage(cm_lds, cmean, csd, clogit, C, Ls, 0);
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool active = row < (long long)M * K * B;
  const int c = active ? (int)(row / ((long long)K * B)) : 0;
  const int kb = active ? (int)(row % ((long long)K * B)) : 0;
  const int b = kb % B;
  float lpw = 0.f, lqw;
  float lq[MAXM];
  if (active)  // shared dims: u for cm_scores; private dims: the fixed prior p(w) = family(0, wsd)
    lat_fwd_dims(p, M, D, Ls, family, c, kb, b, lane, lq, lqw, [&](int l, float z) {
      if (l < Ls)
        ubuf[l] = z;
      else
        lpw += lat_logp(family, z, 0.f, wsd[l - Ls]);
    });
  __syncthreads();  // ubuf
  if (!active) return;
  float a[CPL], amx, asum;
  cm_scores(family, ubuf, cm_lds, C, Ls, lane, a, amx, asum);
  lpw = wave_sum(lpw);
  lqw = wave_sum(lqw);
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    if (m == c) {
#pragma unroll
      for (int q = 0; q < CPL; ++q) {
        const int j = lane + 64 * q;
        if (j < C) p.resp[m][(long long)kb * C + j] = expf(a[q] - amx) / asum;
      }
    }
  }
  lat_fwd_finish(p, M, K, B, c, kb, b, lane, lq, [&](int m) {
    p.lpz[m][kb] = (amx + logf(asum)) + lpw;
    p.lqw[m][kb] = lqw;
  });
}

// ---- backward on the latent side ----------------------------------------------------------------------------------------------------
// one wave per batch row b, as latent_bwd_kernel of mmvae.hip: lat_bwd_dim (latent.hpp) runs the sums over c and k in a fixed order
// inside one lane.
// dparams [B, C Ls + C]: row b holds this row's terms of d loss / d cluster means ([C, Ls]) and d loss / d logits ([C]); the caller
// sums the rows (mvk_colsum_acc).  Their weight is g = d loss / d lw times beta, once, IWAE and DReG alike (as dprior_sd in
// latent_bwd_kernel): only the path through the reparameterised sample is scaled by w a second time under DReG.
__global__ __launch_bounds__(256) void cm_latent_bwd_kernel(const LatBwdPtrs p, const float* __restrict__ cmean,
                                                            const float* __restrict__ csd,
                                                            const float* __restrict__ clogit,
                                                            const float* __restrict__ wsd, int M, int K, int B, int D,
                                                            int Ls, int C, float beta, int family, int dreg,
                                                            const float* __restrict__ gscale,
                                                            float* __restrict__ dparams) {
  extern __shared__ float cm_lds[];
  cm_stage(cm_lds, cmean, csd, clogit, C, Ls, 0);
  const int Lsp = cm_stride(Ls);
  const float* tm = cm_lds;
  const float* ts = tm + C * Lsp;
  const float* tl = ts + C * Lsp;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // no barrier below
  const float gs = gscale ? *gscale : 1.0f;
  bool avail[MAXM];
  const int navail = lat_avail(p.mask, M, b, avail);
  const float inv_n = 1.0f / (float)navail;
  for (int l = lane; l < D; l += 64) {
    const float ws = l >= Ls ? wsd[l - Ls] : 1.f;
    // prior: the mixture's pull on u (sum_j q_j d log p(u|j) / du), the fixed prior of w
    lat_bwd_dim(p, M, K, B, D, Ls, beta, family, dreg, gs, inv_n, navail, avail, b, l,
                [&](int c, long long kb, float g, float z) {
                  if (l >= Ls) return g * lat_dlogp_dz(family, z, 0.f, ws);
                  const float* r = p.resp[c] + kb * C;
                  float pull = 0.f;
                  for (int j = 0; j < C; ++j) pull += r[j] * lat_dlogp_dz(family, z, tm[j * Lsp + l], ts[j * Lsp + l]);
                  return g * pull;
                });
  }
  // parameter rows: d lw / d mean_jl = beta q_j (-d log p(u_l|j) / du_l),  d lw / d logit_i = beta (q_i - pi_i)
  float* prow = dparams + (long long)b * ((long long)C * Ls + C);
  for (int l = lane; l < Ls; l += 64) {
    for (int j = 0; j < C; ++j) {
      const float mj = tm[j * Lsp + l], sj = ts[j * Lsp + l];
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < MAXM; ++c) {
        if (c < M && avail[c]) {
          for (int k = 0; k < K; ++k) {
            const long long kb = (long long)k * B + b;
            const float g = -gs * inv_n * p.w[c][kb] * beta;
            acc += g * p.resp[c][kb * C + j] * (-lat_dlogp_dz(family, p.z[c][kb * D + l], mj, sj));
          }
        }
      }
      prow[(long long)j * Ls + l] = acc;
    }
  }
  for (int j = lane; j < C; j += 64) {
    const float pi = expf(tl[j]);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < MAXM; ++c) {
      if (c < M && avail[c]) {
        for (int k = 0; k < K; ++k) {
          const long long kb = (long long)k * B + b;
          const float g = -gs * inv_n * p.w[c][kb] * beta;
          acc += g * (p.resp[c][kb * C + j] - pi);
        }
      }
    }
    prow[(long long)C * Ls + j] = acc;
  }
}

// ---- cluster assignment (predict_clusters) ------------------------------------------------------------------------------------------
// one wave per row of z; lanes over the clusters.  pc_z [C, R] = softmax_j(log(pi_j + 1e-20) + log p(z|j)); argmax [R]: its first
// maximum; norm_llik [R] (nullable) = sum_j pc_j (lpz_j + lpc_j - log pc_j) / Ls = logsumexp_j(lpc_j + lpz_j) / Ls.
__global__ __launch_bounds__(256) void cm_assign_kernel(const float* __restrict__ z, const float* __restrict__ cmean,
                                                        const float* __restrict__ csd, const float* __restrict__ clogit,
                                                        long long R, int Ls, int C, int family, float* __restrict__ pc,
                                                        long long* __restrict__ amax, float* __restrict__ nll) {
  extern __shared__ float cm_lds[];
  cm_stage(cm_lds, cmean, csd, clogit, C, Ls, 1);
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  float a[CPL], mx, s;
  cm_scores(family, z + r * Ls, cm_lds, C, Ls, lane, a, mx, s);
  float bv = -1.f;
  int bj = 0x7fffffff;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int j = lane + 64 * q;
    if (j < C) {
      const float v = expf(a[q] - mx) / s;
      pc[(long long)j * R + r] = v;
      if (v > bv) {
        bv = v;
        bj = j;
      }
    }
  }
  const float top = wave_max(bv);
  int cand = bv == top ? bj : 0x7fffffff;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(cand, off, 64);
    cand = o < cand ? o : cand;
  }
  if (lane == 0) {
    amax[r] = cand;
    if (nll) nll[r] = (mx + logf(s)) / (float)Ls;
  }
}

// LDS of one launch, in floats (extra: the per-wave u rows of the forward launch); 0 = over the cap
long long cm_lds_floats(int C, int Ls, int extra) {
  const long long n = cm_table_floats(C, Ls) + extra;
  return n <= MVK_CMVAE_MAX_LDS_FLOATS ? n : 0;
}

}  // namespace

extern "C" {

int mvk_cmvae_latent_fwd(const float* const* mu, const float* const* sd, const float* const* noise,
                         const uint8_t* const* masks, const float* cluster_mean, const float* cluster_std,
                         const float* cluster_logits, const float* wprior_std, int M, int K, int B, int D, int family,
                         int C, float* const* z, float* const* lpz, float* const* lqz, float* const* lq_all,
                         int shared_dims, float* const* lqw, float* const* resp, void* stream) {
  if (!cluster_mean || !cluster_std || !cluster_logits || !wprior_std || D < 2 || shared_dims < 1 || shared_dims >= D ||
      C < 1 || C > MAXC)
    return MVK_EINVAL;
  const long long lds = cm_lds_floats(C, shared_dims, 4 * shared_dims);
  if (!lds) return MVK_EINVAL;
  const int rc = lat_check(mu && sd && noise && z && lpz && lqz && lq_all && lqw && resp, M, K, B, family);
  if (rc != LAT_LAUNCH) return rc;
  LatFwdPtrs p{};
  if (!lat_fill(p.mu, mu, M) || !lat_fill(p.sd, sd, M) || !lat_fill(p.noise, noise, M) || !lat_fill(p.z, z, M) ||
      !lat_fill(p.lpz, lpz, M) || !lat_fill(p.lqz, lqz, M) || !lat_fill(p.lq_all, lq_all, M) ||
      !lat_fill(p.lqw, lqw, M) || !lat_fill(p.resp, resp, M))
    return MVK_EINVAL;
  lat_fill(p.mask, masks, M, false);
  const long long rows = (long long)M * K * B;
  hipLaunchKernelGGL(cm_latent_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), (size_t)lds * sizeof(float),
                     mvk_stream(stream), p, cluster_mean, cluster_std, cluster_logits, wprior_std, M, K, B, D,
                     shared_dims, C, family);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_cmvae_latent_bwd(const float* const* mu, const float* const* sd, const float* const* noise,
                         const float* const* z, const uint8_t* const* masks, const float* cluster_mean,
                         const float* cluster_std, const float* cluster_logits, const float* wprior_std,
                         const float* const* w, const float* const* lq_all, const float* const* lqz,
                         const float* const* resp, const float* const* dz_dec, int M, int K, int B, int D, int family,
                         int dreg, int C, const float* gscale, float* const* dmu, float* const* dsd, float* dparams,
                         int shared_dims, float beta, void* stream) {
  if (!cluster_mean || !cluster_std || !cluster_logits || !wprior_std || !dparams || D < 2 || shared_dims < 1 ||
      shared_dims >= D || C < 1 || C > MAXC)
    return MVK_EINVAL;
  const long long lds = cm_lds_floats(C, shared_dims, 0);
  if (!lds) return MVK_EINVAL;
  const int rc = lat_check(mu && sd && noise && z && w && lq_all && lqz && resp && dz_dec && dmu && dsd, M, K, B, family);
  if (rc != LAT_LAUNCH) return rc;
  LatBwdPtrs p{};
  if (!lat_fill(p.mu, mu, M) || !lat_fill(p.sd, sd, M) || !lat_fill(p.noise, noise, M) || !lat_fill(p.z, z, M) ||
      !lat_fill(p.w, w, M) || !lat_fill(p.lq_all, lq_all, M) || !lat_fill(p.lqz, lqz, M) || !lat_fill(p.resp, resp, M) ||
      !lat_fill(p.dz_dec, dz_dec, M) || !lat_fill(p.dmu, dmu, M) || !lat_fill(p.dsd, dsd, M))
    return MVK_EINVAL;
  lat_fill(p.mask, masks, M, false);
  hipLaunchKernelGGL(cm_latent_bwd_kernel, dim3((B + 3) / 4), dim3(256), (size_t)lds * sizeof(float), mvk_stream(stream),
                     p, cluster_mean, cluster_std, cluster_logits, wprior_std, M, K, B, D, shared_dims, C, beta, family,
                     dreg, gscale, dparams);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_cmvae_assign(const float* z, const float* cluster_mean, const float* cluster_std, const float* cluster_logits,
                     int64_t R, int Ls, int family, int C, float* pc_z, int64_t* argmax, float* norm_llik,
                     void* stream) {
  if (!z || !cluster_mean || !cluster_std || !cluster_logits || !pc_z || !argmax || R < 0 || R > 0x7fffffffLL ||
      Ls < 1 || family < 0 || family > 1 || C < 1 || C > MAXC)
    return MVK_EINVAL;
  const long long lds = cm_lds_floats(C, Ls, 0);
  if (!lds) return MVK_EINVAL;
  if (R == 0) return MVK_OK;
  hipLaunchKernelGGL(cm_assign_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), (size_t)lds * sizeof(float),
                     mvk_stream(stream), z, cluster_mean, cluster_std, cluster_logits, (long long)R, Ls, C, family, pc_z,
                     reinterpret_cast<long long*>(argmax), norm_llik);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
