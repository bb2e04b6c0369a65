// Full-covariance Gaussian-mixture EM on the device (multivae/samplers/gaussian_mixture/gaussian_mixture_sampler.py:90-112 fits
// scikit-learn's GaussianMixture on the host; :148-164 samples from it).  The arithmetic is scikit-learn's
// (_estimate_log_gaussian_prob, _estimate_gaussian_parameters, _estimate_gaussian_covariances_full,
// _compute_precision_cholesky and the loop of BaseMixture.fit) with this precision split: the per-row arithmetic of the E-step
// is fp32; what is summed over rows (n_c, means, covariances, the lower bound) is fp64 from the first product on (per thread, per
// workgroup and across workgroups: the rows are fp32 data, so x - mu and the products are taken in fp64 and the M-step is a float64
// M-step of the fp32 responsibilities); the per-component finish (regularisation, Cholesky, triangular inverse, log-determinant)
// is fp64; every output is stored as fp32.  Why the products too: a component with no more than L points has a covariance that
// is reg_covar in its null directions, and fp32 rounding of (x - mu)(x - mu)^T is noise of that size there -- it moved the lower
// bound of such a fit by 5e-4 in the CPU emulation of tests/gmm_ref.py, the fp64 products by 2e-6.
//
// Layout of the work
//  * E-step: ONE ROW PER LANE.  A workgroup of 128 lanes stages 128 rows in LDS with coalesced loads (row stride LP + 1 words:
//    lane r reads word r (LP + 1) + i, conflict-free), each lane keeps its row in registers (the kernels are instantiated for
//    LP = 8 / 16 / 32 / 64 >= L so that the row and x - mu are register arrays with compile-time indices), and the components are
//    visited one after the other: the precision factor P_c is staged TRANSPOSED in LDS (Pt[j][i] = P_c[i][j], zero for i > j) and
//    every lane reads the same address, a broadcast, four words at a time (ds_read_b128): one LDS instruction per four FMAs.
//    The triangular product stops at the diagonal.  log p(x, c) goes to resp[n, c], the row's logsumexp is taken online, and
//    the lane rewrites its own resp row as exp(log p - lse).
//  * M-step, pass A (n_c and the weighted row sums): tiles of 64 rows in LDS, every thread owns up to 17 of the C (L + 1)
//    sums in fp64.  Pass B (covariances, centred on the NEW means): grid (row slices, components); a workgroup is a 16 x 16
//    arrangement of threads, each owning an (LP / 16)^2 sub-lattice of the L x L sums in fp64; rows with resp = 0 are skipped
//    (the whole workgroup works on one component, so the branch is uniform): Lloyd's one-hot rows cost C times less.
//  * Every grid is capped and strides over the rows: the partials (caller-owned scratch, mvk_gmm_scratch_bytes) are bounded
//    independently of N and are added in workgroup order by the finish kernels.  No floating-point atomics anywhere.
//  * The finish of a component is one workgroup: the fp64 covariance goes to LDS, a left-looking Cholesky runs one column at a
//    time on the first L threads, thread k then solves column k of the triangular inverse by forward substitution into the
//    UPPER triangle of the same LDS matrix (the inverse transposed is exactly P_c, so the factor and P_c share 32 KB at L = 64).
//  * Convergence lives in a caller-owned block of 8 doubles (MVK_GMM_STATE_*): every kernel of mvk_gmm_em_step reads
//    `converged` and `status` first and returns when either is set, and the last kernel of the step updates the block.
#include <float.h>
#include <math.h>

#include "common.hpp"

namespace {

constexpr int E_TPB = 128;       // E-step: rows per tile = lanes per workgroup
constexpr int E_GRID_CAP = 1024;
constexpr int A_ROWS = 64;       // M-step pass A: rows per LDS tile
constexpr int A_GRID_CAP = 256;
constexpr int A_MAXK = 17;       // ceil(64 * 65 / 256)
constexpr int B_ROWS = 64;       // M-step pass B: rows per LDS tile
constexpr int B_BLOCKS = 512;    // pass B: about this many workgroups (slices x components)
constexpr double LOG_2PI = 1.8378770664093454835606594728112;

__device__ __forceinline__ bool gmm_stopped(const double* state) {
  return state && (state[MVK_GMM_STATE_CONVERGED] != 0.0 || state[MVK_GMM_STATE_STATUS] != 0.0);
}

// 64-bit sum over the workgroup in a fixed order (thread 0 adds the per-wave sums in wave order); valid in thread 0.
template <int TPB>
__device__ __forceinline__ double block_sum_f64(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < TPB / 64; ++w) s += lds[w];
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// E-step.  HARD = false: resp = softmax_c log p(x, c), row_out = logsumexp, lb_part[block] = sum of the block's logsumexps.
// HARD = true (identity precisions, equal weights): resp = one-hot(argmin_c |x - mu_c|^2), row_out = that minimum,
// labels in/out, *changed += rows whose label changed.
template <int LP, bool HARD>
__global__ __launch_bounds__(E_TPB) void gmm_estep_kernel(const float* __restrict__ X, long long N, int L, int C,
                                                          const float* __restrict__ weights, const float* __restrict__ means,
                                                          const float* __restrict__ prec, const float* __restrict__ logdet,
                                                          float* __restrict__ resp, float* __restrict__ row_out,
                                                          int32_t* __restrict__ labels, int32_t* __restrict__ changed,
                                                          double* __restrict__ lb_part, const double* __restrict__ state) {
  if (gmm_stopped(state)) return;
  constexpr int XS = LP + 1;
  __shared__ float xs[E_TPB * XS];
  __shared__ __attribute__((aligned(16))) float Pt[HARD ? 4 : LP * LP];
  __shared__ float mu[LP];
  __shared__ double red[E_TPB / 64];
  const int tid = threadIdx.x;
  const long long ntiles = (N + E_TPB - 1) / E_TPB;
  const float base = -0.5f * (float)L * (float)LOG_2PI;
  double lse_sum = 0.0;
  int nchanged = 0;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long r0 = tile * E_TPB;
    const int rows = (int)((N - r0) < (long long)E_TPB ? (N - r0) : (long long)E_TPB);
    __syncthreads();  // the previous tile's readers of xs are done
    for (int e = tid; e < rows * L; e += E_TPB) xs[(e / L) * XS + (e % L)] = X[r0 * L + e];
    __syncthreads();
    const bool live = tid < rows;
    float x[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) x[i] = (live && i < L) ? xs[tid * XS + i] : 0.f;
    const long long n = r0 + tid;
    float run_max = -INFINITY, run_sum = 0.f;  // online logsumexp (soft) / running minimum (hard)
    float best = INFINITY;
    int best_c = 0;
    for (int c = 0; c < C; ++c) {
      __syncthreads();  // the previous component's readers of Pt / mu are done
      if (!HARD)
        for (int e = tid; e < LP * LP; e += E_TPB) {
          const int j = e / LP, i = e % LP;
          Pt[e] = (i <= j && j < L) ? prec[((long long)c * L + i) * L + j] : 0.f;
        }
      if (tid < LP) mu[tid] = tid < L ? means[(long long)c * L + tid] : 0.f;
      __syncthreads();
      float d[LP];
#pragma unroll
      for (int i = 0; i < LP; ++i) d[i] = x[i] - mu[i];
      float dist = 0.f;
      if (HARD) {
#pragma unroll
        for (int i = 0; i < LP; ++i) dist = fmaf(d[i], d[i], dist);
        if (dist < best) {
          best = dist;
          best_c = c;
        }
      } else {
#pragma unroll
        for (int j = 0; j < LP; ++j) {
          if (j < L) {
            float y = 0.f;
#pragma unroll
            for (int i4 = 0; i4 <= j / 4; ++i4) {
              const float4 p = *reinterpret_cast<const float4*>(&Pt[j * LP + 4 * i4]);
              y = fmaf(d[4 * i4], p.x, y);
              y = fmaf(d[4 * i4 + 1], p.y, y);
              y = fmaf(d[4 * i4 + 2], p.z, y);
              y = fmaf(d[4 * i4 + 3], p.w, y);
            }
            dist = fmaf(y, y, dist);
          }
        }
        const float lp = (base - 0.5f * dist) + logdet[c] + logf(weights[c]);
        if (live) resp[n * C + c] = lp;
        // online logsumexp: (max, sum of exp(lp - max)); a NaN makes the sum NaN and stays
        const float m = fmaxf(run_max, lp);
        if (lp != lp) {
          run_sum = lp;
        } else if (m != -INFINITY) {
          run_sum = run_sum * expf(run_max - m) + expf(lp - m);
          run_max = m;
        }
      }
    }
    if (live) {
      if (HARD) {
        for (int c = 0; c < C; ++c) resp[n * C + c] = c == best_c ? 1.f : 0.f;
        if (row_out) row_out[n] = best;
        if (labels) {
          if (labels[n] != best_c) ++nchanged;
          labels[n] = best_c;
        }
      } else {
        const float lse = run_max + logf(run_sum);
        for (int c = 0; c < C; ++c) resp[n * C + c] = expf(resp[n * C + c] - lse);
        if (row_out) row_out[n] = lse;
        lse_sum += (double)lse;
      }
    }
  }
  if (HARD) {
    if (changed) {
      int v = nchanged;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((tid & 63) == 0 && v) atomicAdd(changed, v);
    }
  } else {
    const double s = block_sum_f64<E_TPB>(lse_sum, red);
    if (tid == 0) lb_part[blockIdx.x] = s;
  }
}

// lower bound of a stand-alone E-step: lb[0] = sum of the partials in workgroup order / N
__global__ void gmm_lb_kernel(const double* __restrict__ lb_part, int G, long long N, double* __restrict__ lb) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += lb_part[g];
  lb[0] = s / (double)N;
}

// ---------------------------------------------------------------------------------------------------------------------------
// M-step pass A: part[block][c (L + 1) + l] = sum over the block's rows of resp[n, c] * (l < L ? x[n, l] : 1).
__global__ __launch_bounds__(256) void gmm_sums_kernel(const float* __restrict__ X, const float* __restrict__ resp, long long N,
                                                       int L, int C, double* __restrict__ part,
                                                       const double* __restrict__ state) {
  if (gmm_stopped(state)) return;
  __shared__ float xs[A_ROWS * 65];
  __shared__ float rs[A_ROWS * 65];
  const int tid = threadIdx.x;
  const int L1 = L + 1, total = C * L1;
  int co[A_MAXK], lo[A_MAXK];
  double acc[A_MAXK];
#pragma unroll
  for (int k = 0; k < A_MAXK; ++k) {
    const int o = tid + 256 * k;
    co[k] = o < total ? o / L1 : -1;
    lo[k] = o < total ? o % L1 : 0;
    acc[k] = 0.0;
  }
  const long long ntiles = (N + A_ROWS - 1) / A_ROWS;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long r0 = tile * A_ROWS;
    const int rows = (int)((N - r0) < (long long)A_ROWS ? (N - r0) : (long long)A_ROWS);
    __syncthreads();
    for (int e = tid; e < rows * L; e += 256) xs[(e / L) * 65 + (e % L)] = X[r0 * L + e];
    for (int e = tid; e < rows * C; e += 256) rs[(e / C) * 65 + (e % C)] = resp[r0 * C + e];
    for (int r = tid; r < rows; r += 256) xs[r * 65 + L] = 1.f;  // L <= 64: column L of the padded row
    __syncthreads();
#pragma unroll
    for (int k = 0; k < A_MAXK; ++k) {
      if (co[k] >= 0) {
        double a = acc[k];
        for (int r = 0; r < rows; ++r) a = fma((double)rs[r * 65 + co[k]], (double)xs[r * 65 + lo[k]], a);
        acc[k] = a;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < A_MAXK; ++k)
    if (co[k] >= 0) part[(long long)blockIdx.x * total + tid + 256 * k] = acc[k];
}

// finish of pass A (one workgroup): n_c = sum + 10 FLT_EPSILON, means = sums / n_c, weights = n_c / sum_c n_c; with lb_part,
// the lower bound of the E-step before it goes to state[PENDING] (a non-finite one sets status 2).
__global__ __launch_bounds__(256) void gmm_sums_finish_kernel(const double* __restrict__ part, int G, int L, int C,
                                                              float* __restrict__ weights, float* __restrict__ means,
                                                              double* __restrict__ nk, double* __restrict__ means64,
                                                              const double* __restrict__ lb_part,
                                                              int GE, long long N, double* __restrict__ state) {
  if (gmm_stopped(state)) return;
  __shared__ double snk[64];
  __shared__ int stop;
  const int tid = threadIdx.x;
  const int L1 = L + 1, total = C * L1;
  if (lb_part) {  // first: a lower bound that is not finite stops the step before any parameter is written
    if (tid == 0) {
      double s = 0.0;
      for (int g = 0; g < GE; ++g) s += lb_part[g];
      s /= (double)N;
      state[MVK_GMM_STATE_PENDING] = s;
      stop = !(fabs(s) <= DBL_MAX);
      if (stop) state[MVK_GMM_STATE_STATUS] = 2.0;
    }
    __syncthreads();
    if (stop) return;
  }
  if (tid < C) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(long long)g * total + tid * L1 + L];
    s += 10.0 * (double)FLT_EPSILON;
    snk[tid] = s;
    nk[tid] = s;
  }
  __syncthreads();
  for (int o = tid; o < C * L; o += 256) {
    const int c = o / L, l = o % L;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(long long)g * total + c * L1 + l];
    means64[o] = s / snk[c];  // pass B centres on the unrounded mean
    means[o] = (float)(s / snk[c]);
  }
  if (weights && tid < C) {
    double tot = 0.0;
    for (int c = 0; c < C; ++c) tot += snk[c];
    weights[tid] = (float)(snk[tid] / tot);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// M-step pass B: part[c][slice][a L + b] = sum over the slice's rows of resp[n, c] (x[n, a] - mu_c[a]) (x[n, b] - mu_c[b]).
template <int LP>
__global__ __launch_bounds__(256) void gmm_cov_kernel(const float* __restrict__ X, const float* __restrict__ resp, long long N,
                                                      int L, int C, const double* __restrict__ means, double* __restrict__ part,
                                                      const double* __restrict__ state) {
  if (gmm_stopped(state)) return;
  constexpr int E = LP >= 16 ? LP / 16 : 1;  // sums per thread and direction
  constexpr int DS = LP + 1;
  __shared__ double ds[B_ROWS * DS];
  __shared__ float ws[B_ROWS];
  __shared__ double mu[LP];
  const int tid = threadIdx.x, ta = tid & 15, tb = tid >> 4;
  const int c = blockIdx.y, S = gridDim.x;
  if (tid < LP) mu[tid] = tid < L ? means[(long long)c * L + tid] : 0.0;
  double acc[E][E];
#pragma unroll
  for (int k = 0; k < E; ++k)
#pragma unroll
    for (int m = 0; m < E; ++m) acc[k][m] = 0.0;
  const long long ntiles = (N + B_ROWS - 1) / B_ROWS;
  for (long long tile = blockIdx.x; tile < ntiles; tile += S) {
    const long long r0 = tile * B_ROWS;
    const int rows = (int)((N - r0) < (long long)B_ROWS ? (N - r0) : (long long)B_ROWS);
    __syncthreads();  // mu is written; the previous tile's readers are done
    for (int e = tid; e < rows * L; e += 256) ds[(e / L) * DS + (e % L)] = (double)X[r0 * L + e] - mu[e % L];
    for (int r = tid; r < rows; r += 256) ws[r] = resp[(r0 + r) * C + c];
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const float w = ws[r];
      if (w == 0.f) continue;  // uniform: one component per workgroup
      double da[E], db[E];
#pragma unroll
      for (int k = 0; k < E; ++k) {
        da[k] = (ta + 16 * k < L) ? (double)w * ds[r * DS + ta + 16 * k] : 0.0;
        db[k] = (tb + 16 * k < L) ? ds[r * DS + tb + 16 * k] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < E; ++k)
#pragma unroll
        for (int m = 0; m < E; ++m) acc[k][m] = fma(da[k], db[m], acc[k][m]);
    }
  }
  double* out = part + ((long long)c * S + blockIdx.x) * L * L;
#pragma unroll
  for (int k = 0; k < E; ++k)
#pragma unroll
    for (int m = 0; m < E; ++m) {
      const int a = ta + 16 * k, b = tb + 16 * m;
      if (a < L && b < L) out[a * L + b] = acc[k][m];
    }
}

// finish of pass B, one workgroup per component: covariance, its Cholesky factor, P_c = (factor^-1)^T and sum ln diag P_c.
__global__ __launch_bounds__(256) void gmm_cov_finish_kernel(const double* __restrict__ part, int S, int L,
                                                             const double* __restrict__ nk, double reg_covar,
                                                             float* __restrict__ covs, float* __restrict__ chol,
                                                             float* __restrict__ prec, float* __restrict__ logdet,
                                                             double* __restrict__ state) {
  if (gmm_stopped(state)) return;
  __shared__ double A[64 * 64];   // lower triangle + diagonal: the factor; strict upper triangle: P_c
  __shared__ double zdiag[64];    // diagonal of P_c
  __shared__ double sv[64];
  __shared__ int bad;
  const int tid = threadIdx.x, c = blockIdx.x;
  const double n = nk[c];
  if (tid == 0) bad = 0;
  for (int e = tid; e < L * L; e += 256) {
    double s = 0.0;
    for (int g = 0; g < S; ++g) s += part[((long long)c * S + g) * L * L + e];
    s /= n;
    const int a = e / L, b = e % L;
    if (a == b) s += reg_covar;
    covs[(long long)c * L * L + e] = (float)s;
    A[a * 64 + b] = s;
  }
  __syncthreads();
  // left-looking Cholesky, column j on threads i = j .. L-1
  for (int j = 0; j < L; ++j) {
    if (tid >= j && tid < L) {
      double s = A[tid * 64 + j];
      for (int m = 0; m < j; ++m) s -= A[tid * 64 + m] * A[j * 64 + m];
      sv[tid] = s;
    }
    __syncthreads();
    const double p = sv[j];
    if (!(p > 0.0) || !(p <= DBL_MAX)) {  // uniform: every thread reads the same pivot
      if (tid == 0 && state) state[MVK_GMM_STATE_STATUS] = 1.0;
      bad = 1;
      break;
    }
    const double dj = sqrt(p);
    if (tid >= j && tid < L) A[tid * 64 + j] = tid == j ? dj : sv[tid] / dj;
    __syncthreads();
  }
  __syncthreads();
  if (bad) {  // no state block to report to: the outputs say so
    for (int e = tid; e < L * L; e += 256) {
      chol[(long long)c * L * L + e] = NAN;
      prec[(long long)c * L * L + e] = NAN;
    }
    if (tid == 0) logdet[c] = NAN;
    return;
  }
  // column k of Z = factor^-1 by forward substitution; Z[i][k] is P_c[k][i]: row k of the upper triangle
  if (tid < L) {
    const int k = tid;
    const double zk = 1.0 / A[k * 64 + k];
    zdiag[k] = zk;
    for (int i = k + 1; i < L; ++i) {
      double s = A[i * 64 + k] * zk;
      for (int m = k + 1; m < i; ++m) s += A[i * 64 + m] * A[k * 64 + m];
      A[k * 64 + i] = -s / A[i * 64 + i];
    }
  }
  __syncthreads();
  for (int e = tid; e < L * L; e += 256) {
    const int a = e / L, b = e % L;
    chol[(long long)c * L * L + e] = a >= b ? (float)A[a * 64 + b] : 0.f;
    prec[(long long)c * L * L + e] = a < b ? (float)A[a * 64 + b] : (a == b ? (float)zdiag[a] : 0.f);
  }
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < L; ++i) s += log(zdiag[i]);
    logdet[c] = (float)s;
  }
}

// last kernel of an EM step: the order of BaseMixture.fit (prev = lb; lb = new; change = lb - prev; converged = |change| < tol)
__global__ void gmm_state_kernel(double* __restrict__ state, double tol) {
  if (threadIdx.x || blockIdx.x) return;
  if (gmm_stopped(state)) return;
  const double prev = state[MVK_GMM_STATE_LB], lb = state[MVK_GMM_STATE_PENDING];
  state[MVK_GMM_STATE_PREV] = prev;
  state[MVK_GMM_STATE_LB] = lb;
  state[MVK_GMM_STATE_ITER] += 1.0;
  if (fabs(lb - prev) < tol) state[MVK_GMM_STATE_CONVERGED] = 1.0;
}

// z[i, a] = mu_c[a] + sum_{b <= a} chol_c[a, b] eps[i, b], c = comp[i]
__global__ __launch_bounds__(256) void gmm_sample_kernel(const float* __restrict__ means, const float* __restrict__ chol,
                                                         const int32_t* __restrict__ comp, const float* __restrict__ eps,
                                                         long long n, int L, int C, float* __restrict__ z) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= n * L) return;
  const long long i = o / L;
  const int a = (int)(o % L);
  const int c = comp[i];
  if (c < 0 || c >= C) {
    z[o] = NAN;
    return;
  }
  const float* row = chol + ((long long)c * L + a) * L;
  float s = means[(long long)c * L + a];
  for (int b = 0; b <= a; ++b) s = fmaf(row[b], eps[i * L + b], s);
  z[o] = s;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
struct GmmScratch {
  double* lb_part;   // E_GRID_CAP
  double* nk;        // 64
  double* means64;   // 64 * 64
  double* sums;      // A_GRID_CAP * C * (L + 1)
  double* cov;       // C * S * L * L
  long long doubles;
};

int gmm_slices(int C) {
  const int s = B_BLOCKS / C;
  return s < 1 ? 1 : s;
}

GmmScratch gmm_carve(void* scratch, int L, int C) {
  GmmScratch s;
  double* p = static_cast<double*>(scratch);
  s.lb_part = p;
  s.nk = p + E_GRID_CAP;
  s.means64 = s.nk + 64;
  s.sums = s.means64 + 64 * 64;
  s.cov = s.sums + (long long)A_GRID_CAP * C * (L + 1);
  s.doubles = (s.cov - p) + (long long)C * gmm_slices(C) * L * L;
  return s;
}

bool gmm_shape_ok(long long N, int L, int C) { return N >= 0 && L >= 1 && L <= 64 && C >= 1 && C <= 64; }

int gmm_grid(long long N, int rows, int cap) {
  const long long t = (N + rows - 1) / rows;
  return (int)(t < cap ? t : cap);
}

template <bool HARD>
int gmm_launch_estep(const float* X, long long N, int L, int C, const float* weights, const float* means, const float* prec,
                     const float* logdet, float* resp, float* row_out, int32_t* labels, int32_t* changed, double* lb_part,
                     const double* state, int G, hipStream_t s) {
#define MVK_GMM_E(LP)                                                                                                        \
  hipLaunchKernelGGL((gmm_estep_kernel<LP, HARD>), dim3(G), dim3(E_TPB), 0, s, X, N, L, C, weights, means, prec, logdet, resp, \
                     row_out, labels, changed, lb_part, state)
  if (L <= 8)
    MVK_GMM_E(8);
  else if (L <= 16)
    MVK_GMM_E(16);
  else if (L <= 32)
    MVK_GMM_E(32);
  else
    MVK_GMM_E(64);
#undef MVK_GMM_E
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int gmm_launch_mstep(const float* X, const float* resp, long long N, int L, int C, double reg_covar, int means_only,
                     float* weights, float* means, float* covs, float* chol, float* prec, float* logdet, const GmmScratch& sc,
                     const double* lb_part, int GE, double* state, hipStream_t s) {
  const int GA = gmm_grid(N, A_ROWS, A_GRID_CAP);
  hipLaunchKernelGGL(gmm_sums_kernel, dim3(GA), dim3(256), 0, s, X, resp, N, L, C, sc.sums, state);
  MVK_CHECK_LAUNCH();
  hipLaunchKernelGGL(gmm_sums_finish_kernel, dim3(1), dim3(256), 0, s, sc.sums, GA, L, C, weights, means, sc.nk, sc.means64, lb_part, GE, N,
                     state);
  MVK_CHECK_LAUNCH();
  if (means_only) return MVK_OK;
  const int S = gmm_grid(N, B_ROWS, gmm_slices(C));
#define MVK_GMM_B(LP) \
  hipLaunchKernelGGL((gmm_cov_kernel<LP>), dim3(S, C), dim3(256), 0, s, X, resp, N, L, C, sc.means64, sc.cov, state)
  if (L <= 16)
    MVK_GMM_B(16);
  else if (L <= 32)
    MVK_GMM_B(32);
  else
    MVK_GMM_B(64);
#undef MVK_GMM_B
  MVK_CHECK_LAUNCH();
  hipLaunchKernelGGL(gmm_cov_finish_kernel, dim3(C), dim3(256), 0, s, sc.cov, S, L, sc.nk, reg_covar, covs, chol, prec, logdet,
                     state);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // namespace

extern "C" {

int mvk_gmm_scratch_bytes(int L, int C, int64_t* bytes) {
  if (!bytes || !gmm_shape_ok(0, L, C)) return MVK_EINVAL;
  *bytes = gmm_carve(nullptr, L, C).doubles * (int64_t)sizeof(double);
  return MVK_OK;
}

int mvk_gmm_estep(const float* X, int64_t N, int L, int C, const float* weights, const float* means, const float* prec_chol,
                  const float* logdet, int hard, float* resp, float* row_out, int32_t* labels, int32_t* changed, double* lb,
                  void* scratch, void* stream) {
  if (!gmm_shape_ok(N, L, C)) return MVK_EINVAL;
  if (N == 0) return MVK_OK;
  if (!X || !means || !resp || !scratch) return MVK_EINVAL;
  if (!hard && (!weights || !prec_chol || !logdet)) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  const GmmScratch sc = gmm_carve(scratch, L, C);
  const int G = gmm_grid(N, E_TPB, E_GRID_CAP);
  if (hard) {
    if (changed && hipMemsetAsync(changed, 0, sizeof(int32_t), s) != hipSuccess) return MVK_ELAUNCH;
    return gmm_launch_estep<true>(X, N, L, C, nullptr, means, nullptr, nullptr, resp, row_out, labels, changed, nullptr, nullptr,
                                  G, s);
  }
  int rc = gmm_launch_estep<false>(X, N, L, C, weights, means, prec_chol, logdet, resp, row_out, nullptr, nullptr, sc.lb_part,
                                   nullptr, G, s);
  if (rc != MVK_OK) return rc;
  if (lb) {
    hipLaunchKernelGGL(gmm_lb_kernel, dim3(1), dim3(64), 0, s, sc.lb_part, G, (long long)N, lb);
    MVK_CHECK_LAUNCH();
  }
  return MVK_OK;
}

int mvk_gmm_mstep(const float* X, const float* resp, int64_t N, int L, int C, double reg_covar, int means_only, float* weights,
                  float* means, float* covs, float* cov_chol, float* prec_chol, float* logdet, void* scratch, void* stream) {
  if (!gmm_shape_ok(N, L, C)) return MVK_EINVAL;
  if (N == 0) return MVK_OK;
  if (!X || !resp || !means || !scratch) return MVK_EINVAL;
  if (!means_only && (!weights || !covs || !cov_chol || !prec_chol || !logdet)) return MVK_EINVAL;
  const GmmScratch sc = gmm_carve(scratch, L, C);
  return gmm_launch_mstep(X, resp, N, L, C, reg_covar, means_only, weights, means, covs, cov_chol, prec_chol, logdet, sc, nullptr,
                          0, nullptr, mvk_stream(stream));
}

int mvk_gmm_em_step(const float* X, int64_t N, int L, int C, double reg_covar, double tol, float* weights, float* means,
                    float* covs, float* cov_chol, float* prec_chol, float* logdet, float* resp, double* state, void* scratch,
                    void* stream) {
  if (!gmm_shape_ok(N, L, C)) return MVK_EINVAL;
  if (N == 0) return MVK_OK;
  if (!X || !weights || !means || !covs || !cov_chol || !prec_chol || !logdet || !resp || !state || !scratch) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  const GmmScratch sc = gmm_carve(scratch, L, C);
  const int G = gmm_grid(N, E_TPB, E_GRID_CAP);
  int rc = gmm_launch_estep<false>(X, N, L, C, weights, means, prec_chol, logdet, resp, nullptr, nullptr, nullptr, sc.lb_part,
                                   state, G, s);
  if (rc != MVK_OK) return rc;
  rc = gmm_launch_mstep(X, resp, N, L, C, reg_covar, 0, weights, means, covs, cov_chol, prec_chol, logdet, sc, sc.lb_part, G,
                        state, s);
  if (rc != MVK_OK) return rc;
  hipLaunchKernelGGL(gmm_state_kernel, dim3(1), dim3(64), 0, s, state, tol);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_gmm_sample(const float* means, const float* cov_chol, const int32_t* comp, const float* eps, int64_t n, int L, int C,
                   float* z, void* stream) {
  if (!gmm_shape_ok(n, L, C)) return MVK_EINVAL;
  if (n == 0) return MVK_OK;
  if (!means || !cov_chol || !comp || !eps || !z) return MVK_EINVAL;
  const long long total = (long long)n * L;
  hipLaunchKernelGGL(gmm_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, mvk_stream(stream), means, cov_chol,
                     comp, eps, (long long)n, L, C, z);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
