// The latent stage shared by the MMVAE / MMVAE+ kernels (mmvae.hip) and the CMVAE kernels (cmvae.hip):
//   - log-densities, their derivatives and the reparameterisation map of the latent families (Normal, Laplace with a softmax scale);
//   - the mixture-of-experts posterior of one (c, k, b) row (lat_fwd_dims, lat_fwd_finish) and its backward for one latent dim of one
//     batch row (lat_avail, lat_bwd_dim).  The prior is the caller's: a callable that the two kernels of each pair pass in, resolved at
//     compile time.  Nothing here uses LDS or a barrier; those are cmvae.hip's own;
//   - the pointer tables of the two launches and the argument checks and marshalling of their C entry points.
#pragma once
#include "common.hpp"

namespace {

constexpr int MAXM = MVK_MAX_MODALITIES;
constexpr float HALF_LOG_2PI = 0.918938533204672742f;

__device__ __forceinline__ float lat_logp(int family, float z, float loc, float sd) {
  if (family == MVK_FAMILY_NORMAL) {
    const float d = z - loc;
    return -(d * d) / (2.0f * sd * sd) - logf(sd) - HALF_LOG_2PI;
  }
  return -logf(2.0f * sd) - fabsf(z - loc) / sd;
}
// d logp / d z  (d/d loc is its negative)
__device__ __forceinline__ float lat_dlogp_dz(int family, float z, float loc, float sd) {
  const float d = z - loc;
  if (family == MVK_FAMILY_NORMAL) return -d / (sd * sd);
  return -(d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / sd;
}
__device__ __forceinline__ float lat_dlogp_dsd(int family, float z, float loc, float sd) {
  const float d = z - loc;
  if (family == MVK_FAMILY_NORMAL) return d * d / (sd * sd * sd) - 1.0f / sd;
  return -1.0f / sd + fabsf(d) / (sd * sd);
}
// z = loc + sd * t(noise)
__device__ __forceinline__ float lat_t(int family, float noise) {
  if (family == MVK_FAMILY_NORMAL) return noise;
  const float sg = noise > 0.f ? 1.f : (noise < 0.f ? -1.f : 0.f);
  return -sg * log1pf(-fabsf(noise));
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// A member that a model does not have stays nullptr: lqw for MMVAE (no private dims), resp for MMVAE and MMVAE+ (no clusters).
struct LatFwdPtrs {
  const float* mu[MAXM];
  const float* sd[MAXM];
  const float* noise[MAXM];
  const uint8_t* mask[MAXM];
  float* z[MAXM];
  float* lpz[MAXM];
  float* lqz[MAXM];
  float* lq_all[MAXM];
  float* lqw[MAXM];   // log q_c(w_c) rows
  float* resp[MAXM];  // CMVAE: q(cluster | u_c) rows [K, B, C]
};

// The per-dim loop of the wave that owns row (c, kb) (b = kb % B), lanes over l: the reparameterised sample z_c[kb], each lane's part
// of every modality's posterior sum over the shared dims (lq) and of the own posterior over the private dims (lqw).
// prior(l, z) sees every sample: the caller's prior term.
template <class Prior>
__device__ __forceinline__ void lat_fwd_dims(const LatFwdPtrs& p, int M, int D, int Ls, int family, int c, int kb, int b, int lane,
                                             float (&lq)[MAXM], float& lqw, Prior&& prior) {
  lqw = 0.f;
#pragma unroll
  for (int m = 0; m < MAXM; ++m) lq[m] = 0.f;
  // static selection of the conditioning modality's pointers
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
    prior(l, z);
    if (l < Ls) {  // shared dims: every modality's posterior enters the mixture of experts
#pragma unroll
      for (int m = 0; m < MAXM; ++m)
        if (m < M) lq[m] += lat_logp(family, z, p.mu[m][o], p.sd[m][o]);
    } else {  // private dims (MMVAE+, CMVAE): the conditioning modality's own posterior
      lqw += lat_logp(family, z, mu_c[o], sd_c[o]);
    }
  }
}

// The wave sums of lq, the availability masks (mmvae_model.py:195) and, in lane 0, the log-sum-exp over the experts and the stores
// lqz[c][kb] = LSE_m lq_m - log(available modalities) and lq_all[c][:, kb].  own(m) runs once, in lane 0, with m == c as a
// constant: the caller stores its own rows (lpz, lqw) there.
template <class Own>
__device__ __forceinline__ void lat_fwd_finish(const LatFwdPtrs& p, int M, int K, int B, int c, int kb, int b, int lane,
                                               float (&lq)[MAXM], Own&& own) {
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
  if (lane == 0) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < MAXM; ++m)
      if (m < M) s += expf(lq[m] - mx);
    const float lse = mx + logf(s);
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
      if (m == c) {
        own(m);
        p.lqz[m][kb] = lse - logf((float)navail);
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

// ---- backward -----------------------------------------------------------------------------------------------------------------------
struct LatBwdPtrs {
  const float* mu[MAXM];
  const float* sd[MAXM];
  const float* noise[MAXM];
  const float* z[MAXM];
  const uint8_t* mask[MAXM];
  const float* w[MAXM];
  const float* lq_all[MAXM];
  const float* lqz[MAXM];
  const float* resp[MAXM];  // CMVAE (nullptr otherwise)
  const float* dz_dec[MAXM];
  float* dmu[MAXM];
  float* dsd[MAXM];
};
static_assert(sizeof(LatFwdPtrs) <= 1024 && sizeof(LatBwdPtrs) <= 1024,
              "kernel arguments: 4 KiB in all; the tables leave three quarters of it to the other arguments");

// avail[m]: modality m is present in batch row b; returns their number
__device__ __forceinline__ int lat_avail(const uint8_t* const (&mask)[MAXM], int M, int b, bool (&avail)[MAXM]) {
  int navail = 0;
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    avail[m] = (m < M) && (mask[m] ? mask[m][b] != 0 : true);
    navail += avail[m] ? 1 : 0;
  }
  return navail;
}

// Latent dim l of batch row b, in one lane: the sums over the conditioning modality c and the sample k in a fixed order, then the
// dmu / dsd stores.  prior(c, kb, g, z) returns g * d log prior / d z for the sample z = z_c[kb][l], g = d loss / d lw[c][kb] times
// beta; c is a constant there.  gs: the incoming gradient of the loss; inv_n = 1 / navail.
template <class Prior>
__device__ __forceinline__ void lat_bwd_dim(const LatBwdPtrs& p, int M, int K, int B, int D, int Ls, float beta, int family,
                                            int dreg, float gs, float inv_n, int navail, const bool (&avail)[MAXM], int b, int l,
                                            Prior&& prior) {
  const long long o = (long long)b * D + l;
  float mu[MAXM], sd[MAXM], dmu[MAXM], dsd[MAXM];
#pragma unroll
  for (int m = 0; m < MAXM; ++m) {
    mu[m] = (m < M) ? p.mu[m][o] : 0.f;
    sd[m] = (m < M) ? p.sd[m][o] : 1.f;
    dmu[m] = 0.f;
    dsd[m] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < MAXM; ++c) {
    if (c < M && avail[c]) {  // rows with mask_c == 0 have lw == 0 identically: no gradient
      for (int k = 0; k < K; ++k) {
        const long long kb = (long long)k * B + b;
        const long long zo = kb * D + l;
        const float wk = p.w[c][kb];
        const float g = -gs * inv_n * wk * beta;  // d loss / d lw[c][k,b] times the weight of the latent terms
        const float z = p.z[c][zo];
        float gz = prior(c, kb, g, z);
        // mixture posterior: lqz = LSE_m s_m - log n ; lw -= lqz
        const float lse = p.lqz[c][kb] + logf((float)navail);
#pragma unroll
        for (int m = 0; m < MAXM; ++m) {
          // shared dims: responsibilities of the mixture; private dims: the own posterior with weight 1
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
        if (dreg) gtot *= wk;  // gradient hook on z (mmvae_model.py:263-266; on u and w: cmvae_model.py:386-392)
        const float t = lat_t(family, p.noise[c][zo]);
        // static accumulation into the conditioning modality's slot
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

// ---- host: the checks and the marshalling the four entry points share ------------------------------------------------------------
constexpr int LAT_LAUNCH = 1;  // lat_check: go on to the launch (anything else is the entry point's return value)

// tables: every required host pointer table is there.  B == 0 is MVK_OK without a launch, also where an entry of a table is NULL.
inline int lat_check(bool tables, int M, int K, int B, int family) {
  if (!tables || M < 1 || M > MAXM || K < 1 || family < 0 || family > 1) return MVK_EINVAL;
  if (B <= 0) return B == 0 ? MVK_OK : MVK_EINVAL;
  if ((long long)M * K * B > 0x7fffffffLL) return MVK_EINVAL;  // row indices are int: M*K*B < 2^31 (include/mvk.h)
  return LAT_LAUNCH;
}

// The first M entries of a host pointer table into a launch's table; false where a required entry is NULL.  An optional table may
// be NULL itself (its entries stay nullptr) and may hold NULL entries.
template <class T>
inline bool lat_fill(T* (&dst)[MAXM], T* const* src, int M, bool required = true) {
  for (int m = 0; m < M; ++m) {
    dst[m] = src ? src[m] : nullptr;
    if (required && !dst[m]) return false;
  }
  return true;
}

}  // namespace
