// TELBO stage two (models/telbo/telbo_model.py:101-124): for every modality m the unimodal posterior's sample and the reference's
// row "KL", which takes the JOINT encoder's log-variance in the place of the modality's own:
//
//   z[m,b,l]      = mu_m + exp(lv_m / 2) eps[m,b,l]
//   kld_rows[m,b] = -1/2 sum_l (1 + joint_lv[b,l] - mu_m^2 - exp(lv_m))
//
// ONE launch each way for all M modalities, in place of M sample launches and the torch arithmetic of the non-standard KL.
// Forward: blockIdx.y = m; a workgroup of four waves takes four rows b, one wave per (m, b) row, lanes stride over L (any L); the
// row sum is the lanes' partial sums folded by wave_sum: a fixed order, no atomics.
// Backward: blockIdx.y = m; one thread per (b, l), everything recomputed from the inputs; the workgroups of m = 0 also write
// djoint_lv (the same value along l: -1/2 sum_m gkld[m,b], added in increasing m).
#include "common.hpp"

namespace {

constexpr int MAXM = MVK_MAX_MODALITIES;

struct TelboIn {
  const float* mu[MAXM];
  const float* lv[MAXM];
};

struct TelboOut {
  float* dmu[MAXM];
  float* dlv[MAXM];
};

__global__ __launch_bounds__(256) void telbo_latent_fwd_kernel(const float* __restrict__ jlv, const TelboIn in,
                                                               const float* __restrict__ eps, int B, int L,
                                                               float* __restrict__ z, float* __restrict__ kld_rows) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.y;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* __restrict__ mu = in.mu[m];
  const float* __restrict__ lv = in.lv[m];
  const long long row = (long long)b * L, zrow = ((long long)m * B + b) * L;
  float kld = 0.f;
  for (int l = lane; l < L; l += 64) {
    const float u = mu[row + l], v = lv[row + l];
    kld += -0.5f * (1.0f + jlv[row + l] - u * u - expf(v));
    z[zrow + l] = u + expf(0.5f * v) * eps[zrow + l];
  }
  kld = wave_sum(kld);
  if (lane == 0) kld_rows[(long long)m * B + b] = kld;
}

__global__ __launch_bounds__(256) void telbo_latent_bwd_kernel(const TelboIn in, const TelboOut out,
                                                               const float* __restrict__ eps,
                                                               const float* __restrict__ dz,
                                                               const float* __restrict__ gkld, int M, int B, int L,
                                                               float* __restrict__ djlv) {
  const long long n = (long long)B * L;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int m = blockIdx.y;
  const int b = (int)(i / L);
  const float u = in.mu[m][i], v = in.lv[m][i];
  const float gk = gkld ? gkld[(long long)m * B + b] : 0.f;
  float gmu = gk * u, glv = 0.5f * gk * expf(v);
  if (dz) {
    const float g = dz[(long long)m * n + i];
    gmu += g;
    glv += 0.5f * expf(0.5f * v) * eps[(long long)m * n + i] * g;
  }
  out.dmu[m][i] = gmu;
  out.dlv[m][i] = glv;
  if (djlv && m == 0) {
    float s = 0.f;
    if (gkld)
      for (int k = 0; k < M; ++k) s += gkld[(long long)k * B + b];
    djlv[i] = -0.5f * s;
  }
}

}  // namespace

int mvk_telbo_latent_fwd(const float* joint_lv, const float* const* mu, const float* const* lv, int M, const float* eps,
                         int B, int L, float* z, float* kld_rows, void* stream) {
  if (!joint_lv || !mu || !lv || M < 1 || M > MAXM || !eps || !z || !kld_rows || L < 1 || B < 0) return MVK_EINVAL;
  TelboIn in{};
  for (int m = 0; m < M; ++m) {
    if (!mu[m] || !lv[m]) return MVK_EINVAL;
    in.mu[m] = mu[m];
    in.lv[m] = lv[m];
  }
  if (B == 0) return MVK_OK;
  hipLaunchKernelGGL(telbo_latent_fwd_kernel, dim3((B + 3) / 4, M), dim3(256), 0, mvk_stream(stream), joint_lv, in, eps, B,
                     L, z, kld_rows);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_telbo_latent_bwd(const float* const* mu, const float* const* lv, int M, const float* eps, const float* dz,
                         const float* gkld, int B, int L, float* const* dmu, float* const* dlv, float* djoint_lv,
                         void* stream) {
  if (!mu || !lv || M < 1 || M > MAXM || !eps || !dmu || !dlv || L < 1 || B < 0) return MVK_EINVAL;
  TelboIn in{};
  TelboOut out{};
  for (int m = 0; m < M; ++m) {
    if (!mu[m] || !lv[m] || !dmu[m] || !dlv[m]) return MVK_EINVAL;
    in.mu[m] = mu[m];
    in.lv[m] = lv[m];
    out.dmu[m] = dmu[m];
    out.dlv[m] = dlv[m];
  }
  if (B == 0) return MVK_OK;
  const long long n = (long long)B * L;
  if ((n + 255) / 256 > 0x7fffffffLL) return MVK_EINVAL;
  hipLaunchKernelGGL(telbo_latent_bwd_kernel, dim3((unsigned)((n + 255) / 256), M), dim3(256), 0, mvk_stream(stream), in,
                     out, eps, dz, gkld, M, B, L, djoint_lv);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}
