// Log-densities, their derivatives and the reparameterisation map of the latent families (Normal, Laplace with a softmax scale),
// shared by the MMVAE / MMVAE+ kernels (mmvae.hip) and the CMVAE kernels (cmvae.hip).
#pragma once
#include "common.hpp"

namespace {

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

}  // namespace
