// Streaming first and second moments of two feature streams for the Frechet distance (multivae/metrics/fids/fids.py appends every
// batch's activations to a Python list, concatenates, copies all of them to the host and runs np.mean / np.cov there).  Stream 0 is
// the real data, stream 1 the generated data, both [n, D] fp32 rows per call, any D >= 1 and n >= 1.
//
// Scheme (include/mvk.h, "Frechet statistics").  Per stream the caller-owned state holds a shift c[D] (fp32, the column mean of
// the stream's FIRST batch, fixed afterwards), the row count (int64), S1[D] = sum (x - c) and S2 = sum (x - c)(x - c)^T, both fp64.
// The shift is what keeps fp32 products usable: features that sit far from zero (Inception's pool features are non-negative)
// lose their covariance to cancellation in un-shifted fp32 raw moments, while x - c is of the size of the spread.
//
// Layout of the work
//  * Update: one workgroup of four waves per FD_T x FD_T tile on or above the diagonal and per stream (grid x = the packed tile
//    index, grid z = the stream: both streams in one launch).  The rows of the call are walked in chunks of FD_CHUNK: the two
//    column blocks of the chunk (one on a diagonal tile) are staged in LDS as x - c, zero-padded to an even number of rows and to
//    the tile's width, never read out of bounds; every wave reads its 32 x 32 quarter of the state tile into fp64 registers first,
//    forms the chunk's quarter of (X - c)^T (X - c) with v_mfma_f32_32x32x2_f32 (bit for bit a row-ordered fmaf chain), adds it to
//    those registers after every chunk, and writes them back after the last chunk.  A thread loads its rows of the NEXT chunk into
//    registers before the products of the current one (every load of a chunk in flight at once, their latency behind the MFMAs).
//    The workgroup of a diagonal tile also sums its 64 columns (S1, fp64, row order), workgroup 0 adds n to the count.
//  * State: S2 is stored as packed tiles (tile (ti, tj), ti <= tj, at index ti nt - ti (ti - 1) / 2 + tj - ti; FD_T x FD_T doubles,
//    row-major, the part of an edge tile beyond D stays zero): nothing below the diagonal is computed or stored, and the
//    read-modify-write of a tile is contiguous.
//  * Determinism: a state element is written by exactly one workgroup per launch and no sum depends on a launch parameter other
//    than the call's own n and D, so a repeat of the same sequence of calls is bit-identical.  No floating-point atomics.
//  * Finish: cov[i][j] is computed from (a, b) = (min, max) of (i, j) by one expression, so the lower triangle mirrors the upper
//    bit for bit; the terms (one workgroup, fixed order, fp64) are taken from the written mean and cov.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int FD_T = 64;       // tile edge of S2 (four waves, a 32 x 32 MFMA accumulator each)
constexpr int FD_CHUNK = 64;   // rows per chunk: 2 column blocks x 64 rows x 64 columns x 4 B = 32 KiB of LDS
constexpr int FD_TPB = 256;
constexpr long long FD_MAX_D = 65535LL * FD_T;  // nt (nt + 1) / 2 tiles must fit grid x

typedef float fd_f32x16 __attribute__((ext_vector_type(16)));

struct FdLayout {
  long long nt, Dp, ntile;         // tiles per edge, padded width nt FD_T, tiles on or above the diagonal
  long long off_s1, off_s2, off_c; // bytes; the two int64 counts are at 0
  long long bytes;
};

__host__ __device__ inline FdLayout fd_layout(long long D) {
  FdLayout L;
  L.nt = (D + FD_T - 1) / FD_T;
  L.Dp = L.nt * FD_T;
  L.ntile = L.nt * (L.nt + 1) / 2;
  L.off_s1 = 16;
  L.off_s2 = L.off_s1 + 2 * L.Dp * (long long)sizeof(double);
  L.off_c = L.off_s2 + 2 * L.ntile * FD_T * FD_T * (long long)sizeof(double);
  L.bytes = L.off_c + 2 * L.Dp * (long long)sizeof(float);
  return L;
}

__device__ __forceinline__ long long* fd_count(char* st) { return reinterpret_cast<long long*>(st); }
__device__ __forceinline__ double* fd_s1(char* st, const FdLayout& L, int stream) {
  return reinterpret_cast<double*>(st + L.off_s1) + stream * L.Dp;
}
__device__ __forceinline__ double* fd_s2(char* st, const FdLayout& L, int stream) {
  return reinterpret_cast<double*>(st + L.off_s2) + stream * L.ntile * FD_T * FD_T;
}
__device__ __forceinline__ float* fd_c(char* st, const FdLayout& L, int stream) {
  return reinterpret_cast<float*>(st + L.off_c) + stream * L.Dp;
}

// c[stream][col] = the column mean of the n rows: one thread per column, rows added in row order in fp64, stored as fp32
__global__ __launch_bounds__(FD_TPB) void fd_shift_kernel(const float* __restrict__ X0, const float* __restrict__ X1, long long n,
                                                          int D, char* __restrict__ state) {
  const int stream = blockIdx.y;
  const float* X = stream ? X1 : X0;
  const long long col = (long long)blockIdx.x * FD_TPB + threadIdx.x;
  if (col >= D) return;
  const FdLayout L = fd_layout(D);
  double s = 0.0;
  for (long long r = 0; r < n; ++r) s += (double)X[r * D + col];
  fd_c(state, L, stream)[col] = (float)(s / (double)n);
}

__global__ __launch_bounds__(FD_TPB) void fd_update_kernel(const float* __restrict__ X0, const float* __restrict__ X1, long long n,
                                                           int D, char* __restrict__ state) {
  __shared__ float A[FD_CHUNK * FD_T], B[FD_CHUNK * FD_T];
  constexpr int PER = FD_CHUNK * FD_T / FD_TPB;  // elements of a column block per thread and chunk
  constexpr int RSTEP = FD_TPB / FD_T;           // a thread keeps its column and walks the rows in steps of RSTEP
  const int stream = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* X = stream ? X1 : X0;
  const FdLayout L = fd_layout(D);
  const int nt = (int)L.nt;
  int p = blockIdx.x, ti = 0;
  while (p >= nt - ti) {  // the packed index back to (ti, tj), ti <= tj
    p -= nt - ti;
    ++ti;
  }
  const int tj = ti + p;
  const bool diag = ti == tj;
  const int cc = tid % FD_T, rb = tid / FD_T;
  const long long ca = (long long)ti * FD_T + cc, cb = (long long)tj * FD_T + cc;
  const bool in_a = ca < D, in_b = !diag && cb < D;
  const float* c = fd_c(state, L, stream);  // padded to nt FD_T entries
  const float sa = c[ca], sb = c[cb];
  const int wi = wave >> 1, wj = wave & 1;
  const bool work = !(diag && wi > wj);  // the quarter below the diagonal of a diagonal tile is never read
  const float* Bs = diag ? A : B;
  const int ao = wi * 32 + (lane & 31), bo = wj * 32 + (lane & 31), kh = lane >> 5;
  double* tile = fd_s2(state, L, stream) + (long long)blockIdx.x * FD_T * FD_T;
  double acc64[16];  // this wave's part of the state tile: read first, every chunk added in row order, written last
#pragma unroll
  for (int i = 0; i < 16; ++i) acc64[i] = work ? tile[(wi * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh) * FD_T + bo] : 0.0;
  double s1 = 0.0;
  // a chunk's rows are loaded into registers (all loads in flight together) one chunk ahead of the products
  float va[PER], vb[PER];
  auto load = [&](long long r0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const long long row = r0 + rb + RSTEP * i;
      va[i] = (in_a && row < n) ? X[row * D + ca] : sa;  // padding: x - c = 0
      vb[i] = (in_b && row < n) ? X[row * D + cb] : sb;
    }
  };
  load(0);
  for (long long r0 = 0; r0 < n; r0 += FD_CHUNK) {
    const int rows = (int)((n - r0) < (long long)FD_CHUNK ? (n - r0) : (long long)FD_CHUNK);
    const int rows_pad = (rows + 1) & ~1;  // the MFMA's K is 2
    __syncthreads();  // the previous chunk's readers are done
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      A[(rb + RSTEP * i) * FD_T + cc] = va[i] - sa;
      if (!diag) B[(rb + RSTEP * i) * FD_T + cc] = vb[i] - sb;
    }
    __syncthreads();
    if (r0 + FD_CHUNK < n) load(r0 + FD_CHUNK);
    if (work) {
      fd_f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      int k = 0;
      for (; k + 8 <= rows_pad; k += 8) {  // four steps at a time: their eight LDS reads are issued together
        float a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a[u] = A[(k + 2 * u + kh) * FD_T + ao];
          b[u] = Bs[(k + 2 * u + kh) * FD_T + bo];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
      }
      for (; k < rows_pad; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(k + kh) * FD_T + ao], Bs[(k + kh) * FD_T + bo], acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc64[i] += (double)acc[i];
    }
    if (diag && tid < FD_T)
      for (int r = 0; r < rows; ++r) s1 += (double)A[r * FD_T + tid];
  }
  if (work) {
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[(wi * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh) * FD_T + bo] = acc64[i];
  }
  if (diag && tid < FD_T) fd_s1(state, L, stream)[ti * FD_T + tid] += s1;
  if (blockIdx.x == 0 && tid == 0) fd_count(state)[stream] += n;
}

// mean[stream][j] and cov[stream][i][j], i strided over grid y; one expression for (i, j) and (j, i)
__global__ __launch_bounds__(FD_TPB) void fd_finish_kernel(char* __restrict__ state, int D, double* __restrict__ mean,
                                                           double* __restrict__ cov) {
  const int stream = blockIdx.z;
  const long long j = (long long)blockIdx.x * FD_TPB + threadIdx.x;
  if (j >= D) return;
  const FdLayout L = fd_layout(D);
  const double n = (double)fd_count(state)[stream];
  const double* s1 = fd_s1(state, L, stream);
  const double* s2 = fd_s2(state, L, stream);
  if (blockIdx.y == 0) mean[(long long)stream * D + j] = (double)fd_c(state, L, stream)[j] + s1[j] / n;
  for (long long i = blockIdx.y; i < D; i += gridDim.y) {
    const long long a = i < j ? i : j, b = i < j ? j : i;
    const long long ta = a / FD_T, tb = b / FD_T;
    const long long tile = ta * L.nt - ta * (ta - 1) / 2 + (tb - ta);
    const double q = s2[(tile * FD_T + a % FD_T) * FD_T + b % FD_T];
    cov[((long long)stream * D + i) * D + j] = (q - s1[a] * s1[b] / n) / (n - 1.0);
  }
}

__device__ __forceinline__ double fd_block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < FD_TPB / 64; ++w) s += lds[w];
  __syncthreads();
  return s;
}

// terms = {|mean0 - mean1|^2, tr cov0, tr cov1, n0, n1} from the written mean and cov (one workgroup, fixed order)
__global__ __launch_bounds__(FD_TPB) void fd_terms_kernel(char* __restrict__ state, int D, const double* __restrict__ mean,
                                                          const double* __restrict__ cov, double* __restrict__ terms) {
  __shared__ double red[FD_TPB / 64];
  double d2 = 0.0, t0 = 0.0, t1 = 0.0;
  for (long long j = threadIdx.x; j < D; j += FD_TPB) {
    const double d = mean[j] - mean[D + j];
    d2 = fma(d, d, d2);
    t0 += cov[j * D + j];
    t1 += cov[((long long)D + j) * D + j];
  }
  d2 = fd_block_sum(d2, red);
  t0 = fd_block_sum(t0, red);
  t1 = fd_block_sum(t1, red);
  if (threadIdx.x == 0) {
    terms[MVK_FD_TERM_DMEAN2] = d2;
    terms[MVK_FD_TERM_TRACE0] = t0;
    terms[MVK_FD_TERM_TRACE1] = t1;
    terms[MVK_FD_TERM_N0] = (double)fd_count(state)[0];
    terms[MVK_FD_TERM_N1] = (double)fd_count(state)[1];
  }
}

bool fd_shape_ok(int D) { return D >= 1 && (long long)D <= FD_MAX_D; }

}  // namespace

extern "C" {

int mvk_fd_tile(void) { return FD_T; }

int mvk_fd_chunk(void) { return FD_CHUNK; }

int mvk_fd_state_bytes(int D, int64_t* bytes) {
  if (!bytes || !fd_shape_ok(D)) return MVK_EINVAL;
  *bytes = fd_layout(D).bytes;
  return MVK_OK;
}

int mvk_fd_begin(const float* X0, const float* X1, int64_t n, int D, void* state, void* stream) {
  if (!X0 || !state || n < 1 || !fd_shape_ok(D)) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  if (hipMemsetAsync(state, 0, (size_t)fd_layout(D).bytes, s) != hipSuccess) return MVK_ELAUNCH;
  hipLaunchKernelGGL(fd_shift_kernel, dim3((D + FD_TPB - 1) / FD_TPB, X1 ? 2 : 1), dim3(FD_TPB), 0, s, X0, X1, (long long)n, D,
                     static_cast<char*>(state));
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_fd_update(const float* X0, const float* X1, int64_t n, int D, void* state, void* stream) {
  if (!X0 || !state || n < 1 || !fd_shape_ok(D)) return MVK_EINVAL;
  const FdLayout L = fd_layout(D);
  hipLaunchKernelGGL(fd_update_kernel, dim3((unsigned)L.ntile, 1, X1 ? 2 : 1), dim3(FD_TPB), 0, mvk_stream(stream), X0, X1,
                     (long long)n, D, static_cast<char*>(state));
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_fd_finish(void* state, int D, double* mean, double* cov, double* terms, void* stream) {
  if (!state || !mean || !cov || !terms || !fd_shape_ok(D)) return MVK_EINVAL;
  hipStream_t s = mvk_stream(stream);
  hipLaunchKernelGGL(fd_finish_kernel, dim3((D + FD_TPB - 1) / FD_TPB, D < 65535 ? D : 65535, 2), dim3(FD_TPB), 0, s,
                     static_cast<char*>(state), D, mean, cov);
  MVK_CHECK_LAUNCH();
  hipLaunchKernelGGL(fd_terms_kernel, dim3(1), dim3(FD_TPB), 0, s, static_cast<char*>(state), D, mean, cov, terms);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
