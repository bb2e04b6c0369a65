// MMVAE mixture-of-experts importance weights (IWAE / DReG), Normal and Laplace(softmax-scale) families.
// Follows models/mmvae/mmvae_model.py:66-74 (log_var_to_std), :95-158 (forward), :160-236 (compute_k_lws),
// :238-292 (dreg_looser / iwae_looser).
// MMVAE+ (models/mmvaePlus/mmvaePlus_model.py:110-360) runs on the same kernels: the latent of a modality is the
// concatenation [u (shared, Ls dims), w (private)], the mixture density covers the shared dims only, the private dims
// are scored by the modality's own posterior (lqw), the prior terms are weighted by beta, and the private part of a
// cross-modal decoder input is sampled from the target modality's prior (cross_latent kernels).  All tensors are small ([K,B,L], L ~ 20-64): these kernels are
// latency-bound; the design goal is few launches and deterministic reductions.
// The mixture-of-experts stage of latent_fwd_kernel / latent_bwd_kernel, their pointer tables and the entry points' common
// argument checks live in latent.hpp, shared with cmvae.hip; the two kernels here supply the learnable prior.
#include "common.hpp"
#include "latent.hpp"

namespace {

// ---- std from log-variance ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void std_fwd_kernel(const float* __restrict__ lv, int rows, int L, int family,
                                                      float* __restrict__ sd) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* x = lv + (long long)r * L;
  float* y = sd + (long long)r * L;
  if (family == MVK_FAMILY_NORMAL) {
    for (int l = lane; l < L; l += 64) y[l] = expf(0.5f * x[l]);
    return;
  }
  if (family == MVK_FAMILY_NORMAL_SOFTPLUS) {  // F.softplus (threshold 20) + 1e-6, mmvaePlus_model.py:117-118
    for (int l = lane; l < L; l += 64) y[l] = (x[l] > 20.f ? x[l] : log1pf(expf(x[l]))) + 1e-6f;
    return;
  }
  float mx = -INFINITY;
  for (int l = lane; l < L; l += 64) mx = fmaxf(mx, x[l]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int l = lane; l < L; l += 64) s += expf(x[l] - mx);
  s = wave_sum(s);
  for (int l = lane; l < L; l += 64) y[l] = expf(x[l] - mx) / s * (float)L + 1e-6f;
}

__global__ __launch_bounds__(256) void std_bwd_kernel(const float* __restrict__ lv, const float* __restrict__ sd,
                                                      const float* __restrict__ dsd, int rows, int L, int family,
                                                      float* __restrict__ dlv) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long long o = (long long)r * L;
  if (family == MVK_FAMILY_NORMAL) {
    for (int l = lane; l < L; l += 64) dlv[o + l] = dsd[o + l] * 0.5f * sd[o + l];
    return;
  }
  if (family == MVK_FAMILY_NORMAL_SOFTPLUS) {  // d softplus = sigmoid
    for (int l = lane; l < L; l += 64) {
      const float x = lv[o + l];
      dlv[o + l] = dsd[o + l] * (x > 20.f ? 1.0f : 1.0f / (1.0f + expf(-x)));
    }
    return;
  }
  // sd = softmax * L + 1e-6  ->  d lv_i = L * p_i * (dsd_i - sum_j dsd_j p_j).  p is recomputed from lv: recovering it as
  // (sd - 1e-6) / L cancels for p L below ~1e-7 and loses the relative accuracy of those entries.
  float mx = -INFINITY;
  for (int l = lane; l < L; l += 64) mx = fmaxf(mx, lv[o + l]);
  mx = wave_max(mx);
  float s = 0.f, dot = 0.f;
  for (int l = lane; l < L; l += 64) {
    const float e = expf(lv[o + l] - mx);
    s += e;
    dot += dsd[o + l] * e;
  }
  s = wave_sum(s);
  dot = wave_sum(dot) / s;
  for (int l = lane; l < L; l += 64) {
    const float p = expf(lv[o + l] - mx) / s;
    dlv[o + l] = (float)L * p * (dsd[o + l] - dot);
  }
  (void)sd;
}

// ---- forward: samples, prior log-density, mixture log-density --------------------------------------------------
// one wave per (c, k, b); lanes over l.  The mixture-of-experts stage is latent.hpp's; the prior here is one learnable
// family(prior_mean, prior_sd) over all L dims.
__global__ __launch_bounds__(256) void latent_fwd_kernel(const LatFwdPtrs p, const float* __restrict__ prior_mean,
                                                         const float* __restrict__ prior_sd, int M, int K, int B,
                                                         int L, int Ls, int family) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long total = (long long)M * K * B;
  if (row >= total) return;
  const int c = (int)(row / ((long long)K * B));
  const int kb = (int)(row % ((long long)K * B));
  const int b = kb % B;
  float lp = 0.f, lqw;
  float lq[MAXM];
  lat_fwd_dims(p, M, L, Ls, family, c, kb, b, lane, lq, lqw,
               [&](int l, float z) { lp += lat_logp(family, z, prior_mean[l], prior_sd[l]); });
  lp = wave_sum(lp);
  lqw = wave_sum(lqw);
  lat_fwd_finish(p, M, K, B, c, kb, b, lane, lq, [&](int m) {
    p.lpz[m][kb] = lp;
    if (p.lqw[m]) p.lqw[m][kb] = lqw;  // NULL for MMVAE
  });
}

// ---- objective: lw, softmax weights over K, loss -------------------------------------------------------------
struct ObjPtrs {
  const float* rows[MAXM * MAXM];  // [c][r]: rescaled NLL rows of modality r decoded from z_c
  const float* lpz[MAXM];
  const float* lqz[MAXM];
  const float* lqw[MAXM];  // MMVAE+ (may be NULL)
  const uint8_t* mask[MAXM];
  float* lw[MAXM];
  float* w[MAXM];
  float* rowcoef[MAXM];
};

__global__ __launch_bounds__(1024) void objective_kernel(const ObjPtrs p, int M, int K, int B, int dreg, float beta,
                                                         float* __restrict__ loss) {
  float local = 0.f;
  for (int idx = threadIdx.x; idx < M * B; idx += blockDim.x) {
    const int c = idx / B;
    const int b = idx % B;
    const float* lpz = nullptr;
    const float* lqz = nullptr;
    const uint8_t* mk = nullptr;
    float* lw = p.lw[c];
    float* w = p.w[c];
    float* rc = p.rowcoef[c];
    lpz = p.lpz[c];
    lqz = p.lqz[c];
    mk = p.mask[c];
    int navail = 0;
#pragma unroll
    for (int m = 0; m < MAXM; ++m)
      if (m < M) navail += (p.mask[m] ? (p.mask[m][b] != 0) : 1);
    const float mc = mk ? (mk[b] ? 1.f : 0.f) : 1.f;
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
      const long long o = (long long)k * B + b;
      float lpx = 0.f;  // sum_r log p(x_r | z_c) * mask_r  (mmvae_model.py:208-225)
      for (int r = 0; r < M; ++r) {
        const float mr = p.mask[r] ? (p.mask[r][b] ? 1.f : 0.f) : 1.f;
        lpx += -p.rows[c * MAXM + r][o] * mr;
      }
      const float lqw = p.lqw[c] ? p.lqw[c][o] : 0.f;
      const float v = (lpx + beta * (lpz[o] - lqz[o] - lqw)) * mc;  // mmvaePlus_model.py:262
      lw[o] = v;
      mx = fmaxf(mx, v);
    }
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(lw[(long long)k * B + b] - mx);
    const float lse = mx + logf(s);
    float obj = 0.f;
    for (int k = 0; k < K; ++k) {
      const long long o = (long long)k * B + b;
      const float wk = expf(lw[o] - mx) / s;  // not expf(lw - lse): rounding lse (|lw| ~ 3e3) would scale the whole column
      w[o] = wk;
      rc[o] = -wk * mc / (float)navail;  // d loss / d lw[c][k,b]
      obj += wk * lw[o];
    }
    if (!dreg) obj = lse - logf((float)K);
    local += obj / (float)navail;
  }
  __shared__ float red[16];
  local = wave_sum(local);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    *loss = -t;
  }
}

// ---- backward on the latent side ------------------------------------------------------------------------------
// one wave per batch row b; lanes over l; lat_bwd_dim (latent.hpp) loops over conditioning modality c and sample k
__global__ __launch_bounds__(256) void latent_bwd_kernel(const LatBwdPtrs p, const float* __restrict__ prior_mean,
                                                         const float* __restrict__ prior_sd, int M, int K, int B,
                                                         int L, int Ls, float beta, int family, int dreg,
                                                         const float* __restrict__ gscale,
                                                         float* __restrict__ dprior_sd) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float gs = gscale ? *gscale : 1.0f;
  bool avail[MAXM];
  const int navail = lat_avail(p.mask, M, b, avail);
  const float inv_n = 1.0f / (float)navail;
  for (int l = lane; l < L; l += 64) {
    const float pm = prior_mean[l], ps = prior_sd[l];
    float dps = 0.f;
    lat_bwd_dim(p, M, K, B, L, Ls, beta, family, dreg, gs, inv_n, navail, avail, b, l,
                [&](int, long long, float g, float z) {
                  dps += g * lat_dlogp_dsd(family, z, pm, ps);
                  return g * lat_dlogp_dz(family, z, pm, ps);
                });
    if (dprior_sd) dprior_sd[(long long)b * L + l] = dps;  // per-row term [B, L]: the caller sums the rows in a fixed order
  }
}

// ---- MMVAE+ cross-modal decoder input: [u_c (first Ls dims of z_c), w ~ prior of the target modality] ----------
// mmvaePlus_model.py:152-172.  zc[k,b,:Ls] = z[k,b,:Ls];  zc[k,b,Ls+j] = prior_sd[j] * t(noise[k,b,j])  (prior mean 0).
__global__ __launch_bounds__(256) void cross_latent_fwd_kernel(const float* __restrict__ z,
                                                               const float* __restrict__ prior_sd,
                                                               const float* __restrict__ noise, long long rows, int D,
                                                               int Ls, int family, float* __restrict__ zc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * D) return;
  const long long r = i / D;
  const int l = (int)(i - r * D);
  zc[i] = l < Ls ? z[i] : prior_sd[l - Ls] * lat_t(family, noise[r * (D - Ls) + (l - Ls)]);
}

// dz[k,b,:Ls] = dzc[k,b,:Ls], 0 elsewhere; dprior_sd[j] = sum_{k,b} dzc[k,b,Ls+j] * t(noise)   (one block per j)
__global__ __launch_bounds__(256) void cross_latent_bwd_kernel(const float* __restrict__ dzc,
                                                               const float* __restrict__ noise, long long rows, int D,
                                                               int Ls, int family, float* __restrict__ dz,
                                                               float* __restrict__ dprior_sd) {
  const int S = D - Ls;
  if ((int)blockIdx.x < S) {
    const int j = blockIdx.x;
    float acc = 0.f;
    for (long long r = threadIdx.x; r < rows; r += 256) acc += dzc[r * D + Ls + j] * lat_t(family, noise[r * S + j]);
    __shared__ float red[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && dprior_sd) dprior_sd[j] = (red[0] + red[1]) + (red[2] + red[3]);
    return;
  }
  const long long i = ((long long)blockIdx.x - S) * 256 + threadIdx.x;
  if (i >= rows * D) return;
  const int l = (int)(i % D);
  dz[i] = l < Ls ? dzc[i] : 0.f;
}

// ---- importance-sampled joint likelihood (compute_joint_nll) -------------------------------------------------
// ln p(x_b) ~= logsumexp_k [ sum_m ln p(x_m | z_kb) + ln p(z_kb) - ln q(z_kb | x_b) ] - ln K with q a uniform mixture
// of E experts (the S subset posteriors of MoPoE, mopoe_model.py:467-594; the M unimodal posteriors of MMVAE,
// mmvae_model.py:365-443; a single joint posterior for MVTCAE, mvtcae_model.py:213-291, and JMVAE,
// joint_model.py:82-154).  The reference walks data points and K-chunks in Python; here the K axis is the leading
// axis of one [K,B] problem (the decoders and mvk_recon_nll_fwd produce the likelihood rows).
constexpr int MAXE = MVK_IWAE_MAX_EXPERTS;
struct IwaePtrs {
  const float* rows[MAXM];
  const float* loc[MAXE];
  const float* sd[MAXE];
};

__global__ __launch_bounds__(256) void iwae_sample_kernel(const float* __restrict__ loc, const float* __restrict__ sd,
                                                          const float* __restrict__ noise, long long n, int BL,
                                                          int family, float* __restrict__ z) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i % BL);
  z[i] = loc[j] + sd[j] * lat_t(family, noise[i]);
}

// one thread per (k,b): the expert parameters of row b are shared by the K threads of that column (L1 / L2 hits)
__global__ __launch_bounds__(256) void iwae_logw_kernel(IwaePtrs a, const float* __restrict__ z,
                                                        const float* __restrict__ prior_loc,
                                                        const float* __restrict__ prior_sd, int K, int B, int L, int E,
                                                        int R, int family, float* __restrict__ lw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)K * B) return;
  const int b = (int)(i % B);
  const float* zr = z + i * L;
  float lpz = 0.f;
  for (int l = 0; l < L; ++l)
    lpz += lat_logp(family, zr[l], prior_loc ? prior_loc[l] : 0.f, prior_sd ? prior_sd[l] : 1.f);
  float m = -INFINITY, s = 0.f;  // running logsumexp over the experts
  for (int e = 0; e < E; ++e) {
    const float* lo = a.loc[e] + (long long)b * L;
    const float* sd = a.sd[e] + (long long)b * L;
    float lq = 0.f;
    for (int l = 0; l < L; ++l) lq += lat_logp(family, zr[l], lo[l], sd[l]);
    if (lq > m) {
      s = s * expf(m - lq) + 1.f;
      m = lq;
    } else if (lq > -INFINITY) {
      s += expf(lq - m);
    } else if (lq != lq) {
      s = lq;  // a NaN expert density fails both comparisons above: it must reach lw as torch.logsumexp would carry it
    }
  }
  const float lqz = m + logf(s) - logf((float)E);
  float lpx = 0.f;
  for (int r = 0; r < R; ++r) lpx -= a.rows[r][i];
  lw[i] = lpx + lpz - lqz;
}

// ll[b] = logsumexp over the n arrays x K samples of lw[.][k,b] - ln(n K); one wave per data point
struct IwaeLw {
  const float* lw[MAXM];
};
__global__ __launch_bounds__(256) void iwae_reduce_kernel(IwaeLw a, int n, int K, int B, float* __restrict__ ll) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  float m = -INFINITY;
  for (int j = 0; j < n; ++j)
    for (int k = lane; k < K; k += 64) m = fmaxf(m, a.lw[j][(long long)k * B + b]);
  m = wave_max(m);
  // A column maximum of -inf or +inf is not subtracted (inf - inf): all -inf gives s = 0 and ll = -inf, a +inf entry s = +inf and
  // ll = +inf, and a NaN entry, which fmaxf drops, reaches s here whatever the maximum is.
  const float mm = (m > -INFINITY && m < INFINITY) ? m : 0.f;
  float s = 0.f;
  for (int j = 0; j < n; ++j)
    for (int k = lane; k < K; k += 64) s += expf(a.lw[j][(long long)k * B + b] - mm);
  s = wave_sum(s);
  if (lane == 0) ll[b] = m + logf(s) - logf((float)n * (float)K);
}

}  // namespace

extern "C" {

int mvk_mmvaeplus_cross_latent_fwd(const float* z, const float* prior_sd, const float* noise, int64_t rows, int D,
                                   int Ls, int family, float* zc, void* stream) {
  if (!z || !prior_sd || !noise || !zc || rows < 0 || D < 2 || Ls < 1 || Ls >= D || family < 0 || family > 1)
    return MVK_EINVAL;
  if (rows == 0) return MVK_OK;
  hipLaunchKernelGGL(cross_latent_fwd_kernel, dim3((unsigned)((rows * D + 255) / 256)), dim3(256), 0,
                     mvk_stream(stream), z, prior_sd, noise, (long long)rows, D, Ls, family, zc);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mmvaeplus_cross_latent_bwd(const float* dzc, const float* noise, int64_t rows, int D, int Ls, int family,
                                   float* dz, float* dprior_sd, void* stream) {
  if (!dzc || !noise || !dz || rows < 0 || D < 2 || Ls < 1 || Ls >= D || family < 0 || family > 1) return MVK_EINVAL;
  if (rows == 0) return MVK_OK;
  const unsigned blocks = (unsigned)(D - Ls) + (unsigned)((rows * D + 255) / 256);
  hipLaunchKernelGGL(cross_latent_bwd_kernel, dim3(blocks), dim3(256), 0, mvk_stream(stream), dzc, noise,
                     (long long)rows, D, Ls, family, dz, dprior_sd);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mmvae_std_fwd(const float* lv, int rows, int L, int family, float* sd, void* stream) {
  if (!lv || !sd || rows < 0 || L < 1 || family < 0 || family > 2) return MVK_EINVAL;
  if (rows == 0) return MVK_OK;
  hipLaunchKernelGGL(std_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, mvk_stream(stream), lv, rows, L, family, sd);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mmvae_std_bwd(const float* lv, const float* sd, const float* dsd, int rows, int L, int family, float* dlv,
                      void* stream) {
  if (!lv || !sd || !dsd || !dlv || rows < 0 || L < 1 || family < 0 || family > 2) return MVK_EINVAL;
  if (rows == 0) return MVK_OK;
  hipLaunchKernelGGL(std_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, mvk_stream(stream), lv, sd, dsd, rows, L,
                     family, dlv);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mmvae_latent_fwd(const float* const* mu, const float* const* sd, const float* const* noise,
                         const uint8_t* const* masks, const float* prior_mean, const float* prior_sd, int M, int K,
                         int B, int L, int family, float* const* z, float* const* lpz, float* const* lqz,
                         float* const* lq_all, int shared_dims, float* const* lqw, void* stream) {
  if (!prior_mean || !prior_sd || L < 1 || shared_dims < 1 || shared_dims > L || (shared_dims < L && !lqw)) return MVK_EINVAL;
  const int rc = lat_check(mu && sd && noise && z && lpz && lqz && lq_all, M, K, B, family);
  if (rc != LAT_LAUNCH) return rc;
  LatFwdPtrs p{};
  if (!lat_fill(p.mu, mu, M) || !lat_fill(p.sd, sd, M) || !lat_fill(p.noise, noise, M) || !lat_fill(p.z, z, M) ||
      !lat_fill(p.lpz, lpz, M) || !lat_fill(p.lqz, lqz, M) || !lat_fill(p.lq_all, lq_all, M))
    return MVK_EINVAL;
  lat_fill(p.mask, masks, M, false);
  lat_fill(p.lqw, lqw, M, false);
  long long rows = (long long)M * K * B;
  hipLaunchKernelGGL(latent_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, mvk_stream(stream), p,
                     prior_mean, prior_sd, M, K, B, L, shared_dims, family);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mmvae_objective_fwd(const float* const* rows, const float* const* lpz, const float* const* lqz,
                            const uint8_t* const* masks, int M, int K, int B, int dreg, float* const* lw_out,
                            float* const* w, float* const* rowcoef, float* loss, const float* const* lqw, float beta,
                            void* stream) {
  if (!rows || !lpz || !lqz || !lw_out || !w || !rowcoef || !loss || M < 1 || M > MAXM || K < 1 || B < 0) return MVK_EINVAL;
  if (B == 0) return MVK_OK;  // zero rows: nothing is launched, loss included (include/mvk.h)
  if ((long long)M * K * B > 0x7fffffffLL) return MVK_EINVAL;  // row indices are int: M*K*B < 2^31 (include/mvk.h)
  ObjPtrs p{};
  for (int m = 0; m < M; ++m) {
    if (!lpz[m] || !lqz[m] || !lw_out[m] || !w[m] || !rowcoef[m]) return MVK_EINVAL;
    p.rowcoef[m] = rowcoef[m];
    for (int r = 0; r < M; ++r) {
      if (!rows[m * M + r]) return MVK_EINVAL;
      p.rows[m * MAXM + r] = rows[m * M + r];
    }
    p.lpz[m] = lpz[m];
    p.lqz[m] = lqz[m];
    p.lqw[m] = lqw ? lqw[m] : nullptr;
    p.mask[m] = masks ? masks[m] : nullptr;
    p.lw[m] = lw_out[m];
    p.w[m] = w[m];
  }
  hipLaunchKernelGGL(objective_kernel, dim3(1), dim3(1024), 0, mvk_stream(stream), p, M, K, B, dreg, beta, loss);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mmvae_latent_bwd(const float* const* mu, const float* const* sd, const float* const* noise,
                         const float* const* z, const uint8_t* const* masks, const float* prior_mean,
                         const float* prior_sd, const float* const* w, const float* const* lq_all,
                         const float* const* lqz, const float* const* dz_dec, int M, int K, int B, int L, int family,
                         int dreg, const float* gscale, float* const* dmu, float* const* dsd, float* dprior_sd,
                         int shared_dims, float beta, void* stream) {
  if (!prior_mean || !prior_sd || L < 1 || shared_dims < 1 || shared_dims > L) return MVK_EINVAL;
  const int rc = lat_check(mu && sd && noise && z && w && lq_all && lqz && dz_dec && dmu && dsd, M, K, B, family);
  if (rc != LAT_LAUNCH) return rc;
  LatBwdPtrs p{};
  if (!lat_fill(p.mu, mu, M) || !lat_fill(p.sd, sd, M) || !lat_fill(p.noise, noise, M) || !lat_fill(p.z, z, M) ||
      !lat_fill(p.w, w, M) || !lat_fill(p.lq_all, lq_all, M) || !lat_fill(p.lqz, lqz, M) ||
      !lat_fill(p.dz_dec, dz_dec, M) || !lat_fill(p.dmu, dmu, M) || !lat_fill(p.dsd, dsd, M))
    return MVK_EINVAL;
  lat_fill(p.mask, masks, M, false);
  hipStream_t s = mvk_stream(stream);
  hipLaunchKernelGGL(latent_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, s, p, prior_mean, prior_sd, M, K, B, L,
                     shared_dims, beta, family, dreg, gscale, dprior_sd);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_iwae_sample(const float* loc, const float* sd, const float* noise, int K, int B, int L, int family, float* z,
                    void* stream) {
  if (K == 0 || B == 0) return MVK_OK;
  if (!loc || !sd || !noise || !z || K < 0 || B < 0 || L < 1 || family < 0 || family > 2) return MVK_EINVAL;
  const long long n = (long long)K * B * L;
  hipLaunchKernelGGL(iwae_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, mvk_stream(stream), loc, sd,
                     noise, n, B * L, family == MVK_FAMILY_LAPLACE_SOFTMAX ? MVK_FAMILY_LAPLACE_SOFTMAX : MVK_FAMILY_NORMAL, z);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_iwae_logw(const float* z, const float* const* rows, int n_rows, const float* const* loc,
                  const float* const* sd, int E, const float* prior_loc, const float* prior_sd, int K, int B, int L,
                  int family, float* lw, void* stream) {
  if (!z || !loc || !sd || !lw || (n_rows > 0 && !rows) || n_rows < 0 || n_rows > MAXM || E < 1 || E > MAXE || K < 0 ||
      B < 0 || L < 1 || family < 0 || family > 2)
    return MVK_EINVAL;
  IwaePtrs a{};
  for (int r = 0; r < n_rows; ++r) {
    if (!rows[r]) return MVK_EINVAL;
    a.rows[r] = rows[r];
  }
  for (int e = 0; e < E; ++e) {
    if (!loc[e] || !sd[e]) return MVK_EINVAL;
    a.loc[e] = loc[e];
    a.sd[e] = sd[e];
  }
  const long long n = (long long)K * B;
  if (n == 0) return MVK_OK;
  hipLaunchKernelGGL(iwae_logw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, mvk_stream(stream), a, z,
                     prior_loc, prior_sd, K, B, L, E, n_rows,
                     family == MVK_FAMILY_LAPLACE_SOFTMAX ? MVK_FAMILY_LAPLACE_SOFTMAX : MVK_FAMILY_NORMAL, lw);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_iwae_reduce(const float* const* lw, int n, int K, int B, float* ll, void* stream) {
  if (!lw || !ll || n < 1 || n > MAXM || K < 1 || B < 0) return MVK_EINVAL;
  IwaeLw a{};
  for (int j = 0; j < n; ++j) {
    if (!lw[j]) return MVK_EINVAL;
    a.lw[j] = lw[j];
  }
  if (B == 0) return MVK_OK;
  hipLaunchKernelGGL(iwae_reduce_kernel, dim3((B + 3) / 4), dim3(256), 0, mvk_stream(stream), a, n, K, B, ll);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
