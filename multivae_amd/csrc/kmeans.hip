// Batched k-means (Lloyd) on the device: R independent fits of K centres on the same rows X [N,L] advance in one launch sequence
// (multivae/metrics/latent_clustering/clustering_class.py fits scikit-learn's KMeans on a host copy of the embeddings, once per
// run).  The iteration is scikit-learn's _kmeans_single_lloyd: labels from the current centres, new centres from those labels,
// replace, then stop on equal labels (strict) or on a centre shift <= tol.  One deviation: a cluster without rows keeps its
// centre (scikit-learn moves it to the row farthest from its own centre); it is counted in the run's state block.
//
// Precision split (that of gmm.hip): the per-row squared distance is fp32 and direct (d = x - c, fmaf(d, d, .) in index order,
// not |x|^2 - 2 x.c + |c|^2); every sum over rows (cluster sums, counts, inertia, centre shift) is fp64 from the first addend
// on; centres and distances are stored as fp32.  Counts that are integers (changed labels, contingency table, correct rows)
// are integers.  No floating-point atomics: every fp64 sum is added in a fixed order, so two launches give the same bits, and
// the bits of run r do not depend on R (the row -> workgroup map depends on N alone).
//
// Layout of the work
//  * ONE ROW PER LANE, grid (row slices, R): a workgroup of 128 lanes holds ONE run's K x L centres in LDS (row stride LP words,
//    staged once per workgroup) and strides over tiles of 128 rows.  A tile is staged in LDS with coalesced loads (row stride
//    LP + 1 words: lane r reads word r (LP + 1) + i, conflict-free), each lane keeps its row in registers (instantiated for
//    LP = 8 / 16 / 32 / 64 >= L), and the centres are visited one after the other: every lane reads the same address, a
//    broadcast, four words at a time (ds_read_b128): one LDS instruction per four subtract-FMA pairs.
//  * Step: the K (L + 1) fp64 sums of the workgroup (row sums and counts, at most 33 KB) live in LDS.  After the labels of a
//    tile are known, each wave publishes one 64-bit ballot per cluster (the lanes whose row went there); the thread that owns
//    sum (k, l) walks the set bits of cluster k's ballots in row order and adds x[row][l] from the staged tile: the work per
//    tile is 128 (L + 1) additions whatever K is, X is read once per step and run, and no [N, K] array exists.
//  * The grid is capped (KM_GRID_CAP slices) and strides over the tiles: the partials (caller-owned scratch,
//    mvk_kmeans_scratch_bytes) are bounded independently of N and are added in workgroup order by the finish kernel, one
//    workgroup per run, which also replaces the centres and updates the run's state block.
//  * Convergence lives in a caller-owned block of 8 doubles per run (MVK_KMEANS_STATE_*): both kernels of mvk_kmeans_step
//    read the run's CONVERGED first and return when it is set, so a stopped run keeps every bit while the others go on.
//  * Assign: the same row kernel without the sums; the contingency table is counted in an LDS histogram per workgroup when
//    K (n_classes + 1) <= KM_HIST words and flushed with one 64-bit integer atomic per non-zero entry, else with one global
//    integer atomic per row.
#include <float.h>
#include <math.h>

#include "common.hpp"

namespace {

constexpr int KM_TPB = 128;      // rows per tile = lanes per workgroup
constexpr int KM_WAVES = KM_TPB / 64;
constexpr int KM_GRID_CAP = 32;  // row slices per run; a function of nothing but N, so that run r's bits do not depend on R
constexpr int KM_HIST = 2048;    // assign: LDS histogram words
constexpr int KM_MAX_R = 32;

__device__ __forceinline__ double km_block_sum_f64(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += lds[w];
  __syncthreads();
  return s;
}

__device__ __forceinline__ long long km_block_sum_i64(long long v, long long* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += lds[w];
  __syncthreads();
  return s;
}

struct KmAssignArgs {   // STEP = false
  int32_t* labels;      // [R,N] out, nullable
  float* d2;            // [R,N] out, nullable
  const int32_t* y;     // [N], nullable
  int n_classes;
  unsigned long long* table;    // [R,K,n_classes + 1], accumulated, nullable
  const int32_t* majority;      // [R,K], nullable
  unsigned long long* correct;  // [R], accumulated, nullable
};

// The row kernel.  STEP: labels in / out, part_sums[run][slice][K (L + 1)], part_in[run][slice] (inertia), part_ch[run][slice]
// (changed labels), nothing for a run whose CONVERGED is set.  Otherwise: the outputs of KmAssignArgs and part_in.
template <int LP, bool STEP>
__global__ __launch_bounds__(KM_TPB) void kmeans_rows_kernel(const float* __restrict__ X, long long N, int L, int K,
                                                             const float* __restrict__ centers, int32_t* __restrict__ step_labels,
                                                             const double* __restrict__ state, double* __restrict__ part_sums,
                                                             double* __restrict__ part_in, long long* __restrict__ part_ch,
                                                             KmAssignArgs a) {
  const int run = blockIdx.y, G = gridDim.x;
  if (STEP && state[(long long)run * MVK_KMEANS_STATE_DOUBLES + MVK_KMEANS_STATE_CONVERGED] != 0.0) return;
  constexpr int XS = LP + 1;
  __shared__ float xs[KM_TPB * XS];
  __shared__ __attribute__((aligned(16))) float cs[64 * LP];
  __shared__ double sums[STEP ? 64 * (LP + 1) : 1];
  __shared__ unsigned long long masks[STEP ? KM_WAVES * 64 : 1];
  __shared__ unsigned int hist[STEP ? 1 : KM_HIST];
  __shared__ double red[KM_WAVES];
  __shared__ long long redi[KM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L1 = L + 1, total = K * L1;
  const float* crun = centers + (long long)run * K * L;
  for (int e = tid; e < K * LP; e += KM_TPB) {
    const int k = e / LP, i = e % LP;
    cs[e] = i < L ? crun[k * L + i] : 0.f;
  }
  const int cells = STEP ? 0 : K * (a.n_classes + 1);
  const bool use_hist = !STEP && a.table && cells <= KM_HIST;
  if (STEP)
    for (int o = tid; o < total; o += KM_TPB) sums[o] = 0.0;
  else if (use_hist)
    for (int o = tid; o < cells; o += KM_TPB) hist[o] = 0u;
  int32_t* lab_out = STEP ? step_labels + (long long)run * N : (a.labels ? a.labels + (long long)run * N : nullptr);
  const long long ntiles = (N + KM_TPB - 1) / KM_TPB;
  double inertia = 0.0;
  long long count = 0;  // STEP: rows whose label changed; else: rows with majority[label] == y
  for (long long tile = blockIdx.x; tile < ntiles; tile += G) {
    const long long r0 = tile * KM_TPB;
    const int rows = (int)((N - r0) < (long long)KM_TPB ? (N - r0) : (long long)KM_TPB);
    __syncthreads();  // the previous tile's readers of xs and masks are done; cs, sums and hist are written
    for (int e = tid; e < rows * L; e += KM_TPB) xs[(e / L) * XS + (e % L)] = X[r0 * L + e];
    __syncthreads();
    const bool live = tid < rows;
    float x[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) x[i] = (live && i < L) ? xs[tid * XS + i] : 0.f;
    float best = INFINITY;
    int best_k = 0;
    for (int k = 0; k < K; ++k) {
      float dist = 0.f;
#pragma unroll
      for (int i4 = 0; i4 < LP / 4; ++i4) {
        const float4 c = *reinterpret_cast<const float4*>(&cs[k * LP + 4 * i4]);
        const float d0 = x[4 * i4] - c.x, d1 = x[4 * i4 + 1] - c.y, d2 = x[4 * i4 + 2] - c.z, d3 = x[4 * i4 + 3] - c.w;
        dist = fmaf(d0, d0, dist);
        dist = fmaf(d1, d1, dist);
        dist = fmaf(d2, d2, dist);
        dist = fmaf(d3, d3, dist);
      }
      if (dist < best || k == 0) {  // the first minimum; a NaN distance never wins after k = 0
        best = dist;
        best_k = k;
      }
    }
    const long long n = r0 + tid;
    if (live) {
      inertia += (double)best;
      if (STEP) {
        if (lab_out[n] != best_k) ++count;
        lab_out[n] = best_k;
      } else {
        if (lab_out) lab_out[n] = best_k;
        if (a.d2) a.d2[(long long)run * N + n] = best;
        if (a.y) {
          const int yy = a.y[n];
          if (a.table) {
            const int col = (yy >= 0 && yy < a.n_classes) ? yy : a.n_classes;
            if (use_hist)
              atomicAdd(&hist[best_k * (a.n_classes + 1) + col], 1u);
            else
              atomicAdd(&a.table[((long long)run * K + best_k) * (a.n_classes + 1) + col], 1ull);
          }
          if (a.correct && a.majority[(long long)run * K + best_k] == yy) ++count;
        }
      }
    }
    if (STEP) {
      // one ballot per cluster and wave, then the owner of sum (k, l) adds the rows of cluster k in row order
      for (int k = 0; k < K; ++k) {
        const unsigned long long m = __ballot(live && best_k == k);
        if (lane == 0) masks[wave * 64 + k] = m;
      }
      __syncthreads();
      for (int o = tid; o < total; o += KM_TPB) {
        const int k = o / L1, l = o % L1;
        double s = sums[o];
#pragma unroll
        for (int w = 0; w < KM_WAVES; ++w) {
          unsigned long long m = masks[w * 64 + k];
          if (l == L) {
            s += (double)__popcll(m);
          } else {
            while (m) {
              const int r = w * 64 + __ffsll((long long)m) - 1;
              m &= m - 1;
              s += (double)xs[r * XS + l];
            }
          }
        }
        sums[o] = s;
      }
    }
  }
  __syncthreads();
  const long long slot = (long long)run * G + blockIdx.x;
  if (STEP) {
    double* out = part_sums + slot * total;
    for (int o = tid; o < total; o += KM_TPB) out[o] = sums[o];
    const long long ch = km_block_sum_i64(count, redi);
    if (tid == 0) part_ch[slot] = ch;
  } else {
    if (use_hist)
      for (int o = tid; o < cells; o += KM_TPB)
        if (hist[o]) atomicAdd(&a.table[(long long)run * cells + o], (unsigned long long)hist[o]);
    if (a.correct) {
      const long long ok = km_block_sum_i64(count, redi);
      if (tid == 0 && ok) atomicAdd(&a.correct[run], (unsigned long long)ok);
    }
  }
  if (part_in) {
    const double s = km_block_sum_f64(inertia, red);
    if (tid == 0) part_in[slot] = s;
  }
}

// inertia[run] = the slices' partials in slice order
__global__ void kmeans_inertia_kernel(const double* __restrict__ part_in, int G, double* __restrict__ inertia) {
  if (threadIdx.x) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += part_in[(long long)blockIdx.x * G + g];
  inertia[blockIdx.x] = s;
}

// finish of a step, one workgroup per run: counts and row sums in slice order, new centre = sum / count (fp64) stored as fp32, a
// cluster without rows keeps its centre; SHIFT = sum (new - old)^2 over the stored fp32 centres; then the state block.
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double* __restrict__ part_sums, const double* __restrict__ part_in,
                                                            const long long* __restrict__ part_ch, int G, int L, int K,
                                                            const double* __restrict__ tol, float* __restrict__ centers,
                                                            double* __restrict__ state) {
  const int run = blockIdx.x, tid = threadIdx.x;
  double* st = state + (long long)run * MVK_KMEANS_STATE_DOUBLES;
  if (st[MVK_KMEANS_STATE_CONVERGED] != 0.0) return;
  __shared__ double cnt[64];
  __shared__ double red[4];
  const int L1 = L + 1, total = K * L1;
  const double* part = part_sums + (long long)run * G * total;
  if (tid < K) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(long long)g * total + tid * L1 + L];
    cnt[tid] = s;
  }
  __syncthreads();
  float* crun = centers + (long long)run * K * L;
  double shift = 0.0;
  for (int o = tid; o < K * L; o += 256) {
    const int k = o / L, l = o % L;
    if (cnt[k] > 0.0) {
      double s = 0.0;
      for (int g = 0; g < G; ++g) s += part[(long long)g * total + k * L1 + l];
      const float cnew = (float)(s / cnt[k]);
      const double d = (double)cnew - (double)crun[o];
      shift = fma(d, d, shift);
      crun[o] = cnew;
    }
  }
  const double shift_tot = km_block_sum_f64(shift, red);
  if (tid == 0) {
    double inertia = 0.0;
    long long changed = 0;
    for (int g = 0; g < G; ++g) {
      inertia += part_in[(long long)run * G + g];
      changed += part_ch[(long long)run * G + g];
    }
    int empty = 0;
    for (int k = 0; k < K; ++k) empty += cnt[k] > 0.0 ? 0 : 1;
    st[MVK_KMEANS_STATE_ITER] += 1.0;
    st[MVK_KMEANS_STATE_SHIFT] = shift_tot;
    st[MVK_KMEANS_STATE_CHANGED] = (double)changed;
    st[MVK_KMEANS_STATE_INERTIA] = inertia;
    st[MVK_KMEANS_STATE_EMPTY] += (double)empty;
    if (changed == 0)
      st[MVK_KMEANS_STATE_CONVERGED] = 1.0;
    else if (shift_tot <= tol[0])
      st[MVK_KMEANS_STATE_CONVERGED] = 2.0;
  }
}

// majority[r, k] = first maximum of table[r, k, 0 .. n_classes); a cluster without a row in a real class maps to itself
__global__ void kmeans_vote_kernel(const long long* __restrict__ table, int cells, int K, int n_classes,
                                   int32_t* __restrict__ majority) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= cells) return;
  const long long* row = table + (long long)o * (n_classes + 1);
  long long best = 0;
  int arg = o % K;
  for (int c = 0; c < n_classes; ++c)
    if (row[c] > best) {
      best = row[c];
      arg = c;
    }
  majority[o] = arg;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
struct KmScratch {
  double* part_in;      // R * KM_GRID_CAP
  long long* part_ch;   // R * KM_GRID_CAP
  double* part_sums;    // R * KM_GRID_CAP * K * (L + 1)
  long long words;      // of 8 bytes
};

KmScratch km_carve(void* scratch, int L, int K, int R) {
  KmScratch s;
  double* p = static_cast<double*>(scratch);
  s.part_in = p;
  s.part_ch = reinterpret_cast<long long*>(p + (long long)R * KM_GRID_CAP);
  s.part_sums = p + 2LL * R * KM_GRID_CAP;
  s.words = 2LL * R * KM_GRID_CAP + (long long)R * KM_GRID_CAP * K * (L + 1);
  return s;
}

bool km_shape_ok(long long N, int L, int K, int R) {
  return N >= 0 && L >= 1 && L <= 64 && K >= 1 && K <= 64 && R >= 1 && R <= KM_MAX_R;
}

int km_grid(long long N) {
  const long long t = (N + KM_TPB - 1) / KM_TPB;
  return (int)(t < KM_GRID_CAP ? t : KM_GRID_CAP);
}

template <bool STEP>
int km_launch_rows(const float* X, long long N, int L, int K, int R, const float* centers, int32_t* step_labels,
                   const double* state, double* part_sums, double* part_in, long long* part_ch, const KmAssignArgs& a, int G,
                   hipStream_t s) {
#define MVK_KM_ROWS(LP)                                                                                                     \
  hipLaunchKernelGGL((kmeans_rows_kernel<LP, STEP>), dim3(G, R), dim3(KM_TPB), 0, s, X, N, L, K, centers, step_labels, state, \
                     part_sums, part_in, part_ch, a)
  if (L <= 8)
    MVK_KM_ROWS(8);
  else if (L <= 16)
    MVK_KM_ROWS(16);
  else if (L <= 32)
    MVK_KM_ROWS(32);
  else
    MVK_KM_ROWS(64);
#undef MVK_KM_ROWS
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // namespace

extern "C" {

int mvk_kmeans_scratch_bytes(int L, int K, int R, int64_t* bytes) {
  if (!bytes || !km_shape_ok(0, L, K, R)) return MVK_EINVAL;
  *bytes = km_carve(nullptr, L, K, R).words * (int64_t)sizeof(double);
  return MVK_OK;
}

int mvk_kmeans_assign(const float* X, int64_t N, int L, int K, int R, const float* centers, int32_t* labels, float* d2,
                      const int32_t* y, int n_classes, int64_t* table, const int32_t* majority, int64_t* correct, double* inertia,
                      void* scratch, void* stream) {
  if (!km_shape_ok(N, L, K, R)) return MVK_EINVAL;
  if (table && (!y || n_classes < 1 || n_classes > (1 << 24))) return MVK_EINVAL;
  if (correct && (!y || !majority)) return MVK_EINVAL;
  if (N == 0) return MVK_OK;
  if (!X || !centers) return MVK_EINVAL;
  if (inertia && !scratch) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  const int G = km_grid(N);
  KmAssignArgs a;
  a.labels = labels;
  a.d2 = d2;
  a.y = y;
  a.n_classes = table ? n_classes : 0;
  a.table = reinterpret_cast<unsigned long long*>(table);
  a.majority = majority;
  a.correct = reinterpret_cast<unsigned long long*>(correct);
  double* part_in = inertia ? km_carve(scratch, L, K, R).part_in : nullptr;
  int rc = km_launch_rows<false>(X, N, L, K, R, centers, nullptr, nullptr, nullptr, part_in, nullptr, a, G, s);
  if (rc != MVK_OK) return rc;
  if (inertia) {
    hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(R), dim3(64), 0, s, part_in, G, inertia);
    MVK_CHECK_LAUNCH();
  }
  return MVK_OK;
}

int mvk_kmeans_step(const float* X, int64_t N, int L, int K, int R, const double* tol, float* centers, int32_t* labels,
                    double* state, void* scratch, void* stream) {
  if (!km_shape_ok(N, L, K, R)) return MVK_EINVAL;
  if (N == 0) return MVK_OK;
  if (!X || !tol || !centers || !labels || !state || !scratch) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  const KmScratch sc = km_carve(scratch, L, K, R);
  const int G = km_grid(N);
  KmAssignArgs none = {};
  int rc = km_launch_rows<true>(X, N, L, K, R, centers, labels, state, sc.part_sums, sc.part_in, sc.part_ch, none, G, s);
  if (rc != MVK_OK) return rc;
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3(R), dim3(256), 0, s, sc.part_sums, sc.part_in, sc.part_ch, G, L, K, tol, centers,
                     state);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_kmeans_vote(const int64_t* table, int R, int K, int n_classes, int32_t* majority, void* stream) {
  if (R < 1 || R > KM_MAX_R || K < 1 || K > 64 || n_classes < 1 || n_classes > (1 << 24) || !table || !majority) return MVK_EINVAL;
  const int cells = R * K;
  hipLaunchKernelGGL(kmeans_vote_kernel, dim3((cells + 255) / 256), dim3(256), 0, mvk_stream(stream),
                     reinterpret_cast<const long long*>(table), cells, K, n_classes, majority);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
