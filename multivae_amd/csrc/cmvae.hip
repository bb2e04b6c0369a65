// CMVAE (models/cmvae/cmvae_model.py): MMVAE+ whose shared-latent prior is a learnable mixture over C clusters.
// The reference takes an explicit expectation of lw under q(c|u) = softmax_c(log pi_c + log p(u|c)) (:292-337); up to its 1e-20
// that expectation is  sum_c q_c (a_c - log q_c) = logsumexp_c a_c  with  a_c = log pi_c + log p(u|c),  so the latent stage is the
// one of mmvae.hip (same launch shape, same per-row ownership) with the shared part of lpz replaced by the log-density of the
// mixture and the private part of the prior fixed at (0, wprior_std).  d lw / d a_c = beta q_c: the forward launch leaves the
// responsibilities q_c behind for the backward launch.  predict_clusters (:546-619) runs on cm_assign_kernel.
// Like mmvae.hip these kernels are latency-bound (rows of 20-64 floats): few launches, deterministic reductions, no atomics.
#include "common.hpp"
#include "latent.hpp"

namespace {

constexpr int MAXM = MVK_MAX_MODALITIES;
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
struct CmFwdPtrs {
  const float* mu[MAXM];
  const float* sd[MAXM];
  const float* noise[MAXM];
  const uint8_t* mask[MAXM];
  float* z[MAXM];
  float* lpz[MAXM];
  float* lqz[MAXM];
  float* lq_all[MAXM];
  float* lqw[MAXM];
  float* resp[MAXM];
};

// one wave per (c, k, b); lanes over l for the posterior terms, over the clusters for the prior
__global__ __launch_bounds__(256) void cm_latent_fwd_kernel(const CmFwdPtrs p, const float* __restrict__ cmean,
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
  float lpw = 0.f, lqw = 0.f;
  float lq[MAXM];
#pragma unroll
  for (int m = 0; m < MAXM; ++m) lq[m] = 0.f;
  if (active) {
    const float* mu_c = nullptr;
    const float* sd_c = nullptr;
    const float* nz_c = nullptr;
    float* z_c = nullptr;
#pragma unroll
    for (int m = 0; m < MAXM; ++m)
      if (m == c) {
        mu_c = p.mu[m];
        sd_c = p.sd[m];
        nz_c = p.noise[m];
        z_c = p.z[m];
      }
    for (int l = lane; l < D; l += 64) {
      const long long o = (long long)b * D + l;
      const long long zo = (long long)kb * D + l;
      const float z = mu_c[o] + sd_c[o] * lat_t(family, nz_c[zo]);
      z_c[zo] = z;
      if (l < Ls) {  // shared dims: every modality's posterior enters the mixture of experts
        ubuf[l] = z;
#pragma unroll
        for (int m = 0; m < MAXM; ++m)
          if (m < M) lq[m] += lat_logp(family, z, p.mu[m][o], p.sd[m][o]);
      } else {  // private dims: the fixed prior p(w) = family(0, wsd) and the conditioning modality's own posterior
        lpw += lat_logp(family, z, 0.f, wsd[l - Ls]);
        lqw += lat_logp(family, z, mu_c[o], sd_c[o]);
      }
    }
  }
  __syncthreads();  // ubuf
  if (!active) return;
  float a[CPL], amx, asum;
  cm_scores(family, ubuf, cm_lds, C, Ls, lane, a, amx, asum);
  lpw = wave_sum(lpw);
  lqw = wave_sum(lqw);
  int navail = 0;
  float mx = -INFINITY;
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    if (m < M) {
      lq[m] = wave_sum(lq[m]);
      const bool av = p.mask[m] ? p.mask[m][b] != 0 : true;
      if (!av) lq[m] = -INFINITY;
      navail += av ? 1 : 0;
      mx = fmaxf(mx, lq[m]);
    }
  }
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    if (m == c) {
#pragma unroll
      for (int q = 0; q < CPL; ++q) {
        const int j = lane + 64 * q;
        if (j < C) p.resp[m][(long long)kb * C + j] = expf(a[q] - amx) / asum;
      }
      if (lane == 0) {
        float s = 0.f;
#pragma unroll
        for (int mm = 0; mm < MAXM; ++mm)
          if (mm < M) s += expf(lq[mm] - mx);
        p.lpz[m][kb] = (amx + logf(asum)) + lpw;
        p.lqz[m][kb] = (mx + logf(s)) - logf((float)navail);
        p.lqw[m][kb] = lqw;
        for (int mm = 0; mm < M; ++mm) {
          float v = 0.f;
#pragma unroll
          for (int q = 0; q < MAXM; ++q)
            if (q == mm) v = lq[q];
          p.lq_all[m][(long long)mm * K * B + kb] = v;
        }
      }
    }
  }
}

// ---- backward on the latent side ----------------------------------------------------------------------------------------------------
struct CmBwdPtrs {
  const float* mu[MAXM];
  const float* sd[MAXM];
  const float* noise[MAXM];
  const float* z[MAXM];
  const uint8_t* mask[MAXM];
  const float* w[MAXM];
  const float* lq_all[MAXM];
  const float* lqz[MAXM];
  const float* resp[MAXM];
  const float* dz_dec[MAXM];
  float* dmu[MAXM];
  float* dsd[MAXM];
};

// one wave per batch row b, as latent_bwd_kernel of mmvae.hip: the sums over c and k run in a fixed order inside one lane.
// dparams [B, C Ls + C]: row b holds this row's terms of d loss / d cluster means ([C, Ls]) and d loss / d logits ([C]); the caller
// sums the rows (mvk_colsum_acc).  Their weight is g = d loss / d lw times beta, once, IWAE and DReG alike (as dprior_sd in
// latent_bwd_kernel): only the path through the reparameterised sample is scaled by w a second time under DReG.
__global__ __launch_bounds__(256) void cm_latent_bwd_kernel(const CmBwdPtrs p, const float* __restrict__ cmean,
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
  int navail = 0;
  bool avail[MAXM];
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    avail[m] = (m < M) && (p.mask[m] ? p.mask[m][b] != 0 : true);
    navail += avail[m] ? 1 : 0;
  }
  const float inv_n = 1.0f / (float)navail;
  for (int l = lane; l < D; l += 64) {
    const long long o = (long long)b * D + l;
    float mu[MAXM], sd[MAXM], dmu[MAXM], dsd[MAXM];
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
      mu[m] = (m < M) ? p.mu[m][o] : 0.f;
      sd[m] = (m < M) ? p.sd[m][o] : 1.f;
      dmu[m] = 0.f;
      dsd[m] = 0.f;
    }
    const float ws = l >= Ls ? wsd[l - Ls] : 1.f;
#pragma unroll
    for (int c = 0; c < MAXM; ++c) {
      if (c < M && avail[c]) {  // rows with mask_c == 0 have lw == 0 identically: no gradient
        for (int k = 0; k < K; ++k) {
          const long long kb = (long long)k * B + b;
          const long long zo = kb * D + l;
          const float wk = p.w[c][kb];
          const float g = -gs * inv_n * wk * beta;  // d loss / d lw[c][k,b] times the weight of the latent terms
          const float z = p.z[c][zo];
          // prior: the mixture's pull on u (sum_j q_j d log p(u|j) / du), the fixed prior of w
          float gz;
          if (l < Ls) {
            const float* r = p.resp[c] + kb * C;
            float pull = 0.f;
            for (int j = 0; j < C; ++j) pull += r[j] * lat_dlogp_dz(family, z, tm[j * Lsp + l], ts[j * Lsp + l]);
            gz = g * pull;
          } else {
            gz = g * lat_dlogp_dz(family, z, 0.f, ws);
          }
          // mixture posterior: lqz = LSE_m s_m - log n ; lw -= lqz
          const float lse = p.lqz[c][kb] + logf((float)navail);
#pragma unroll
          for (int m = 0; m < MAXM; ++m) {
            const bool own = (m == c);
            if (m < M && avail[m] && (l < Ls || own)) {
              const float r = (l < Ls) ? expf(p.lq_all[c][(long long)m * K * B + kb] - lse) : 1.0f;
              const float dz_q = lat_dlogp_dz(family, z, mu[m], sd[m]);
              gz -= g * r * dz_q;
              if (!dreg) {  // IWAE differentiates the q parameters directly as well
                dmu[m] += -g * r * (-dz_q);
                dsd[m] += -g * r * lat_dlogp_dsd(family, z, mu[m], sd[m]);
              }
            }
          }
          float gtot = gz + p.dz_dec[c][zo];
          if (dreg) gtot *= wk;  // gradient hook on u and w (cmvae_model.py:386-392)
          const float t = lat_t(family, p.noise[c][zo]);
#pragma unroll
          for (int m = 0; m < MAXM; ++m) {
            if (m == c) {
              dmu[m] += gtot;
              dsd[m] += gtot * t;
            }
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
      if (m < M) {
        p.dmu[m][o] = dmu[m];
        p.dsd[m][o] = dsd[m];
      }
    }
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
  if (!mu || !sd || !noise || !cluster_mean || !cluster_std || !cluster_logits || !wprior_std || !z || !lpz || !lqz ||
      !lq_all || !lqw || !resp || M < 1 || M > MAXM || K < 1 || D < 2 || family < 0 || family > 1 || shared_dims < 1 ||
      shared_dims >= D || C < 1 || C > MAXC)
    return MVK_EINVAL;
  const long long lds = cm_lds_floats(C, shared_dims, 4 * shared_dims);
  if (!lds) return MVK_EINVAL;
  if (B <= 0) return B == 0 ? MVK_OK : MVK_EINVAL;
  if ((long long)M * K * B > 0x7fffffffLL) return MVK_EINVAL;  // row indices are int: M*K*B < 2^31 (include/mvk.h)
  CmFwdPtrs p{};
  for (int m = 0; m < M; ++m) {
    if (!mu[m] || !sd[m] || !noise[m] || !z[m] || !lpz[m] || !lqz[m] || !lq_all[m] || !lqw[m] || !resp[m])
      return MVK_EINVAL;
    p.mu[m] = mu[m];
    p.sd[m] = sd[m];
    p.noise[m] = noise[m];
    p.mask[m] = masks ? masks[m] : nullptr;
    p.z[m] = z[m];
    p.lpz[m] = lpz[m];
    p.lqz[m] = lqz[m];
    p.lq_all[m] = lq_all[m];
    p.lqw[m] = lqw[m];
    p.resp[m] = resp[m];
  }
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
  if (!mu || !sd || !noise || !z || !cluster_mean || !cluster_std || !cluster_logits || !wprior_std || !w || !lq_all ||
      !lqz || !resp || !dz_dec || !dmu || !dsd || !dparams || M < 1 || M > MAXM || K < 1 || D < 2 || family < 0 ||
      family > 1 || shared_dims < 1 || shared_dims >= D || C < 1 || C > MAXC)
    return MVK_EINVAL;
  const long long lds = cm_lds_floats(C, shared_dims, 0);
  if (!lds) return MVK_EINVAL;
  if (B <= 0) return B == 0 ? MVK_OK : MVK_EINVAL;
  if ((long long)M * K * B > 0x7fffffffLL) return MVK_EINVAL;  // row indices are int: M*K*B < 2^31 (include/mvk.h)
  CmBwdPtrs p{};
  for (int m = 0; m < M; ++m) {
    if (!mu[m] || !sd[m] || !noise[m] || !z[m] || !w[m] || !lq_all[m] || !lqz[m] || !resp[m] || !dz_dec[m] || !dmu[m] ||
        !dsd[m])
      return MVK_EINVAL;
    p.mu[m] = mu[m];
    p.sd[m] = sd[m];
    p.noise[m] = noise[m];
    p.z[m] = z[m];
    p.mask[m] = masks ? masks[m] : nullptr;
    p.w[m] = w[m];
    p.lq_all[m] = lq_all[m];
    p.lqz[m] = lqz[m];
    p.resp[m] = resp[m];
    p.dz_dec[m] = dz_dec[m];
    p.dmu[m] = dmu[m];
    p.dsd[m] = dsd[m];
  }
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
