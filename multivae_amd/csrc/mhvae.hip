// MHVAE level (models/mhvae/mhvae_model.py:119-184): for every subset s of the modalities, the product of the subset's available
// experts and the prior (base_utils.py:122-130, poe), one reparameterised sample and the KL to the prior (:111-119), in ONE launch
// per level of the hierarchy for all subsets, in place of ~25 elementwise / reduce launches per (subset, level).
//
//   experts j of (s, b): the e in member[s] with mask_e[b] set (no mask = set), and the prior
//   T_j = 1 / (exp(lv_j) + 1e-8);  P = sum_j T_j;  jmu = sum_j mu_j T_j / P;  jlv = log(1 / P)
//   z = jmu + exp(jlv / 2) eps  (eps NULL: z = jmu);  kl = 1/2 (plv - jlv + exp(jlv - plv) + (jmu - pmu)^2 / exp(plv) - 1)
//
// written as jlv = -log P, exp(jlv / 2) = sqrt(1 / P), exp(jlv - plv) = 1 / (P exp(plv)).  A masked-out expert is skipped: nothing
// of it is read, its gradients are zeros.  Two layouts (mvk.h): shared (each expert [B,F] serves every subset that holds it, prior
// N(0, I)) and per-subset (expert e [S_e,B,F], block index = rank of s among the subsets holding e; prior [S,B,F]).
//
// Forward: a workgroup of four waves takes four rows b (F / V <= 64: one wave per row) or one (all four waves stride over it), for
// a group of up to SG subsets (blockIdx.y).  In the shared layout a thread forms T and mu T of every expert once per element and
// reuses them for the subsets of the group.  KL row sums: per thread over its elements, over the wave by register-to-register steps
// (wave_sum_dpp), over the row's four waves through LDS, (w0 + w1) + (w2 + w3): a fixed order, no atomics.
// Backward: one thread per (b, f) unit walks the subsets in increasing order; everything is recomputed from the forward inputs; in
// the shared layout the expert gradients are accumulated in registers over the subsets and written once.
// V = 4: 16-byte loads and stores, chosen by the host only when F % 4 == 0 and every pointer is 16-byte aligned.  Contraction is off
// in both kernels, so the 16-byte and the scalar form compute every element with the same roundings.
#include "common.hpp"

namespace {

constexpr int MAXE = MVK_MAX_MODALITIES;
constexpr int MAXS = MVK_MHVAE_MAX_SUBSETS;
constexpr int SG = 8;  // subsets per workgroup of the forward: their KL partial sums live in registers
constexpr float POE_EPS = 1e-8f;

struct LevelTable {
  const float* mu[MAXE];
  const float* lv[MAXE];
  const uint8_t* mask[MAXE];
  uint8_t member[MAXS + 1];
  uint8_t rank[MAXS + 1][MAXE];  // per-subset layout: block of subset s inside expert e
};

struct GradTable {
  float* dmu[MAXE];
  float* dlv[MAXE];
};

template <int V>
struct Vec {
  float v[V];
};

template <int V>
__device__ __forceinline__ Vec<V> ld(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    r.v[0] = x.x, r.v[1] = x.y, r.v[2] = x.z, r.v[3] = x.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void st(float* p, const Vec<V>& r) {
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else
    *p = r.v[0];
}

template <int V>
__device__ __forceinline__ Vec<V> zero() {
  Vec<V> r;
#pragma unroll
  for (int i = 0; i < V; ++i) r.v[i] = 0.f;
  return r;
}

__device__ __forceinline__ unsigned available(const LevelTable& t, int E, int b) {
  unsigned a = 0;
#pragma unroll
  for (int e = 0; e < MAXE; ++e)
    if (e < E && (!t.mask[e] || t.mask[e][b])) a |= 1u << e;
  return a;
}

template <int V>
__global__ __launch_bounds__(256) void mhvae_level_fwd_kernel(const LevelTable t, int E, int S, int shared,
                                                              const float* __restrict__ pmu, const float* __restrict__ plv,
                                                              const float* __restrict__ eps, int B, int F, int wpr,
                                                              float* __restrict__ z, float* __restrict__ kl_rows) {
#pragma clang fp contract(off)
  __shared__ float red[SG][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * (4 / wpr) + wave / wpr;
  const int wsub = wave % wpr;
  const int s0 = blockIdx.y * SG;
  const int ns = S - s0 < SG ? S - s0 : SG;
  float kl[SG];
#pragma unroll
  for (int i = 0; i < SG; ++i) kl[i] = 0.f;
  if (b < B) {
    const unsigned avail = available(t, E, b);
    for (int f = (wsub * 64 + lane) * V; f < F; f += wpr * 64 * V) {
      const long long o = (long long)b * F + f;
      Vec<V> T[MAXE], mT[MAXE];
      if (shared) {
#pragma unroll
        for (int e = 0; e < MAXE; ++e) {
          if (e < E && (avail >> e & 1u)) {
            const Vec<V> m = ld<V>(t.mu[e] + o), l = ld<V>(t.lv[e] + o);
#pragma unroll
            for (int i = 0; i < V; ++i) {
              T[e].v[i] = 1.0f / (expf(l.v[i]) + POE_EPS);
              mT[e].v[i] = m.v[i] * T[e].v[i];
            }
          }
        }
      }
#pragma unroll
      for (int g = 0; g < SG; ++g) {
        if (g < ns) {
          const int s = s0 + g;
          const unsigned act = t.member[s] & avail;
          const long long so = ((long long)s * B + b) * F + f;
          Vec<V> P = zero<V>(), N = zero<V>();
#pragma unroll
          for (int e = 0; e < MAXE; ++e) {
            if (e < E && (act >> e & 1u)) {
              if (shared) {
#pragma unroll
                for (int i = 0; i < V; ++i) P.v[i] += T[e].v[i], N.v[i] += mT[e].v[i];
              } else {
                const long long eo = ((long long)t.rank[s][e] * B + b) * F + f;
                const Vec<V> m = ld<V>(t.mu[e] + eo), l = ld<V>(t.lv[e] + eo);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                  const float Te = 1.0f / (expf(l.v[i]) + POE_EPS);
                  P.v[i] += Te, N.v[i] += m.v[i] * Te;
                }
              }
            }
          }
          Vec<V> pm = zero<V>(), pl = zero<V>(), ev = zero<V>(), out;
          if (pmu) pm = ld<V>(pmu + so), pl = ld<V>(plv + so);
          if (eps) ev = ld<V>(eps + so);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            const float vp = expf(pl.v[i]);  // the prior is the last expert of the product (the 1e-8 is on the experts only)
            const float Tp = 1.0f / (vp + POE_EPS);
            const float Pi = P.v[i] + Tp;
            const float ip = 1.0f / Pi;
            const float jmu = (N.v[i] + pm.v[i] * Tp) * ip;
            const float d = jmu - pm.v[i];
            out.v[i] = jmu + sqrtf(ip) * ev.v[i];
            kl[g] += 0.5f * ((pl.v[i] + logf(Pi)) + ip / vp + d * d / vp - 1.0f);
          }
          st<V>(z + so, out);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < SG; ++g) kl[g] = wave_sum_dpp(kl[g]);
  if (wpr == 1) {
    if (b < B && lane == 0) {
#pragma unroll
      for (int g = 0; g < SG; ++g)
        if (g < ns) kl_rows[(long long)(s0 + g) * B + b] = kl[g];
    }
  } else {  // the row's four waves, in a fixed order
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < SG; ++g) red[g][wave] = kl[g];
    }
    __syncthreads();
    if ((int)threadIdx.x < ns && b < B) {
      const int g = threadIdx.x;
      kl_rows[(long long)(s0 + g) * B + b] = (red[g][0] + red[g][1]) + (red[g][2] + red[g][3]);
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void mhvae_level_bwd_kernel(const LevelTable t, const GradTable gt, int E, int S, int shared,
                                                              const float* __restrict__ pmu, const float* __restrict__ plv,
                                                              const float* __restrict__ eps, const float* __restrict__ dz,
                                                              const float* __restrict__ gkl, int B, int F,
                                                              float* __restrict__ dpmu, float* __restrict__ dplv) {
#pragma clang fp contract(off)
  const int Fu = F / V;
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= (long long)B * Fu) return;
  const int b = (int)(u / Fu);
  const int f = (int)(u - (long long)b * Fu) * V;
  const long long o = (long long)b * F + f;
  const unsigned avail = available(t, E, b);
  Vec<V> mu[MAXE], T[MAXE], ex[MAXE], amu[MAXE], alv[MAXE];
  if (shared) {
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      if (e < E) {
        amu[e] = zero<V>(), alv[e] = zero<V>();
        if (avail >> e & 1u) {
          mu[e] = ld<V>(t.mu[e] + o);
          const Vec<V> l = ld<V>(t.lv[e] + o);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            ex[e].v[i] = expf(l.v[i]);
            T[e].v[i] = 1.0f / (ex[e].v[i] + POE_EPS);
          }
        }
      }
    }
  }
  for (int s = 0; s < S; ++s) {
    const unsigned mem = t.member[s];
    const unsigned act = mem & avail;
    const long long so = ((long long)s * B + b) * F + f;
    if (!shared) {
#pragma unroll
      for (int e = 0; e < MAXE; ++e) {
        if (e < E && (act >> e & 1u)) {
          const long long eo = ((long long)t.rank[s][e] * B + b) * F + f;
          mu[e] = ld<V>(t.mu[e] + eo);
          const Vec<V> l = ld<V>(t.lv[e] + eo);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            ex[e].v[i] = expf(l.v[i]);
            T[e].v[i] = 1.0f / (ex[e].v[i] + POE_EPS);
          }
        }
      }
    }
    Vec<V> P = zero<V>(), N = zero<V>();
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      if (e < E && (act >> e & 1u)) {
#pragma unroll
        for (int i = 0; i < V; ++i) P.v[i] += T[e].v[i], N.v[i] += mu[e].v[i] * T[e].v[i];
      }
    }
    Vec<V> pm = zero<V>(), pl = zero<V>(), ev = zero<V>(), g = zero<V>();
    if (pmu) pm = ld<V>(pmu + so), pl = ld<V>(plv + so);
    if (dz) {
      g = ld<V>(dz + so);
      if (eps) ev = ld<V>(eps + so);
    }
    const float gk = gkl ? gkl[(long long)s * B + b] : 0.f;
    Vec<V> Gmu, GP, jm, ipv, gpm, gpl;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float vp = expf(pl.v[i]);
      const float Tp = 1.0f / (vp + POE_EPS);
      const float Pi = P.v[i] + Tp;
      const float ip = 1.0f / Pi;
      const float jmu = (N.v[i] + pm.v[i] * Tp) * ip;
      const float d = jmu - pm.v[i];
      const float a = gk * d / vp;
      const float r = ip / vp;  // exp(jlv - plv)
      Gmu.v[i] = g.v[i] + a;
      GP.v[i] = -0.5f * g.v[i] * ev.v[i] * ip * sqrtf(ip) + 0.5f * gk * (ip - ip * r);
      jm.v[i] = jmu, ipv.v[i] = ip;
      if (dpmu) {  // the prior as an expert, and its own terms of the KL
        const float dTp = Gmu.v[i] * (pm.v[i] - jmu) * ip + GP.v[i];
        gpm.v[i] = Gmu.v[i] * Tp * ip - a;
        gpl.v[i] = -dTp * vp * Tp * Tp + 0.5f * gk * (1.0f - r - d * d / vp);
      }
    }
    if (dpmu) st<V>(dpmu + so, gpm), st<V>(dplv + so, gpl);
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      if (e < E && (mem >> e & 1u)) {
        Vec<V> gm = zero<V>(), gl = zero<V>();
        if (act >> e & 1u) {
#pragma unroll
          for (int i = 0; i < V; ++i) {
            const float dT = Gmu.v[i] * (mu[e].v[i] - jm.v[i]) * ipv.v[i] + GP.v[i];
            gm.v[i] = Gmu.v[i] * T[e].v[i] * ipv.v[i];
            gl.v[i] = -dT * ex[e].v[i] * T[e].v[i] * T[e].v[i];
          }
        }
        if (shared) {
#pragma unroll
          for (int i = 0; i < V; ++i) amu[e].v[i] += gm.v[i], alv[e].v[i] += gl.v[i];
        } else {
          const long long eo = ((long long)t.rank[s][e] * B + b) * F + f;
          st<V>(gt.dmu[e] + eo, gm), st<V>(gt.dlv[e] + eo, gl);
        }
      }
    }
  }
  if (shared) {
#pragma unroll
    for (int e = 0; e < MAXE; ++e)
      if (e < E) st<V>(gt.dmu[e] + o, amu[e]), st<V>(gt.dlv[e] + o, alv[e]);
  }
}

// The checks both entry points share; fills the table.  *vec: every expert pointer is 16-byte aligned.
int level_table(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int E, const int32_t* member,
                int S, int shared, const float* pmu, const float* plv, int B, int F, LevelTable* t, bool* vec) {
  if (!mu || !lv || !member || E < 1 || E > MAXE || S < 1 || S > MAXS || F < 1 || B < 0) return MVK_EINVAL;
  if (shared != 0 && shared != 1) return MVK_EINVAL;
  if ((pmu == nullptr) != (plv == nullptr) || (shared == 1) != (pmu == nullptr)) return MVK_EINVAL;
  if ((long long)S * B * ((long long)F + 1) > 0x3fffffffffLL) return MVK_EINVAL;
  int count[MAXE] = {0};
  unsigned seen = 0;
  for (int s = 0; s < S; ++s) {
    const int32_t m = member[s];
    if (m <= 0 || m >= (1 << E)) return MVK_EINVAL;  // an empty subset, or an expert the call does not have
    t->member[s] = (uint8_t)m;
    seen |= (unsigned)m;
    for (int e = 0; e < E; ++e) {
      t->rank[s][e] = (uint8_t)count[e];
      if (m >> e & 1) ++count[e];
    }
  }
  if (seen != (1u << E) - 1u) return MVK_EINVAL;  // an expert no subset holds
  *vec = F % 4 == 0 && mvk_aligned16(pmu) && mvk_aligned16(plv);
  for (int e = 0; e < E; ++e) {
    if (!mu[e] || !lv[e]) return MVK_EINVAL;
    t->mu[e] = mu[e], t->lv[e] = lv[e];
    t->mask[e] = masks ? masks[e] : nullptr;
    *vec = *vec && mvk_aligned16(mu[e]) && mvk_aligned16(lv[e]);
  }
  return MVK_OK;
}

}  // namespace

extern "C" {

int mvk_mhvae_level_fwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int E,
                        const int32_t* member, int S, int shared, const float* pmu, const float* plv, const float* eps, int B,
                        int F, float* z, float* kl_rows, void* stream) {
  LevelTable t{};
  bool vec = false;
  const int rc = level_table(mu, lv, masks, E, member, S, shared, pmu, plv, B, F, &t, &vec);
  if (rc != MVK_OK) return rc;
  if (!z || !kl_rows) return MVK_EINVAL;
  if (B == 0) return MVK_OK;
  vec = vec && mvk_aligned16(eps) && mvk_aligned16(z);
  const int Fu = vec ? F / 4 : F;
  const int wpr = Fu <= 64 ? 1 : 4;
  const dim3 grid((unsigned)((B + 4 / wpr - 1) / (4 / wpr)), (unsigned)((S + SG - 1) / SG));
  if (vec)
    hipLaunchKernelGGL(mhvae_level_fwd_kernel<4>, grid, dim3(256), 0, mvk_stream(stream), t, E, S, shared, pmu, plv, eps, B, F,
                       wpr, z, kl_rows);
  else
    hipLaunchKernelGGL(mhvae_level_fwd_kernel<1>, grid, dim3(256), 0, mvk_stream(stream), t, E, S, shared, pmu, plv, eps, B, F,
                       wpr, z, kl_rows);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_mhvae_level_bwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int E,
                        const int32_t* member, int S, int shared, const float* pmu, const float* plv, const float* eps,
                        const float* dz, const float* gkl, int B, int F, float* const* dmu, float* const* dlv, float* dpmu,
                        float* dplv, void* stream) {
  LevelTable t{};
  bool vec = false;
  const int rc = level_table(mu, lv, masks, E, member, S, shared, pmu, plv, B, F, &t, &vec);
  if (rc != MVK_OK) return rc;
  if (!dmu || !dlv || (dpmu == nullptr) != (pmu == nullptr) || (dplv == nullptr) != (pmu == nullptr)) return MVK_EINVAL;
  GradTable gt{};
  vec = vec && mvk_aligned16(eps) && mvk_aligned16(dz) && mvk_aligned16(dpmu) && mvk_aligned16(dplv);
  for (int e = 0; e < E; ++e) {
    if (!dmu[e] || !dlv[e]) return MVK_EINVAL;
    gt.dmu[e] = dmu[e], gt.dlv[e] = dlv[e];
    vec = vec && mvk_aligned16(dmu[e]) && mvk_aligned16(dlv[e]);
  }
  if (B == 0) return MVK_OK;
  const long long units = (long long)B * (vec ? F / 4 : F);
  const long long blocks = (units + 255) / 256;
  if (blocks > 0x7fffffffLL) return MVK_EINVAL;
  if (vec)
    hipLaunchKernelGGL(mhvae_level_bwd_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, mvk_stream(stream), t, gt, E, S, shared,
                       pmu, plv, eps, dz, gkl, B, F, dpmu, dplv);
  else
    hipLaunchKernelGGL(mhvae_level_bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, mvk_stream(stream), t, gt, E, S, shared,
                       pmu, plv, eps, dz, gkl, B, F, dpmu, dplv);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
