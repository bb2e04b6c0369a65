// The stages of the CUB text encoder (models/nn/cub.py CubTextEncoder: a post-norm transformer encoder over sentences of at most
// 64 tokens) that are not GEMMs: the embedding gather and its scatter gradient, the masked self-attention of one (sentence, head)
// and its backward, residual + dropout + LayerNorm and its backward, and the feed-forward dropout (include/mvk.h, "CUB text
// encoder").  The projections and the feed-forward products are the tiled engine's (mvk_linear_*).
//
// Layout of the work
//  * Attention: one workgroup of four waves per (sentence, head).  q (scaled by 1 / sqrt(hd) on the way in, as torch scales it), k
//    and v of the head are staged in LDS with rows hd + 1 apart (a wave reads 64 rows at one column: consecutive banks), the scores
//    in an [S][S + 1] tile.  S <= 64 and hd <= 128: the three products of the forward are 2 S^2 hd FLOP each, 1 MFLOP at the largest
//    shape; they are plain FMAs, every sum over its index in order.  (The f32-input MFMA runs at the rate of the f32 VALU on
//    gfx950 and a 16-row tile is not filled by S = 1 or 5.)  The softmax of a row is one wave's: lane j holds column j.
//    LDS: forward 3 S (hd + 1) + S (S + 1) floats (116 KB at S = 64, hd = 128; 53 KB at the default S = 32), backward
//    2 S (hd + 1) + 2 S (S + 1) (99 KB / 41 KB): the backward stages V and dctx first, then K and Q in the same two tiles.
//  * Residual + LayerNorm: one wave per row, four rows per workgroup; mean, then the centred second moment, then the output
//    (three passes over the wave's own elements of z = x + drop(t), which it parks in the z output, or in y when none is wanted).
//    The backward's column sums (dgamma, dbeta) are two launches: one thread per column over a slab of 64 rows, then over the slabs.
//  * Embedding gradient: one workgroup per (vocabulary row, 256 columns).  It walks the token list in chunks of 4096, every thread
//    over 16 consecutive tokens, and compacts the positions that name its row into an LDS list in index order (counts, exclusive
//    prefix); then every thread adds its column of those rows in list order.  No atomics.
//  * Determinism: every output element is one fixed sequence of fp32 operations (wave sums are the xor butterfly of common.hpp).
#include "common.hpp"

namespace {

constexpr int TX_TPB = 256;
constexpr int TX_WAVES = TX_TPB / MVK_WAVE;
constexpr int TX_CHUNK = 4096;              // tokens per pass of the embedding gradient
constexpr int TX_PER = TX_CHUNK / TX_TPB;   // consecutive tokens per thread
constexpr int TX_SLAB = 64;                 // rows per column-sum slab

// the dropout factor of element i of a site: scale when kept, 0 when dropped (noise == nullptr: always scale, which is 1 then)
__device__ __forceinline__ bool tx_kept(const float* __restrict__ noise, long long i, float p) { return !noise || noise[i] >= p; }

__global__ __launch_bounds__(TX_TPB) void tx_embed_fwd_kernel(const long long* __restrict__ tok, const float* __restrict__ emb,
                                                                const float* __restrict__ pe, const float* __restrict__ noise, float p,
                                                                float scale, float sqrt_e, float* __restrict__ out, int S, int E, int V) {
  const long long row = blockIdx.x;
  const int s = (int)(row % S);
  const long long t = tok[row];
  const bool ok = t >= 0 && t < V;
  for (int e = threadIdx.x; e < E; e += TX_TPB) {
    const long long i = row * E + e;
    const float v = fmaf(ok ? emb[t * E + e] : 0.f, sqrt_e, pe[(long long)s * E + e]);
    out[i] = tx_kept(noise, i, p) ? v * scale : 0.f;
  }
}

__global__ __launch_bounds__(TX_TPB) void tx_embed_bwd_kernel(const long long* __restrict__ tok, const float* __restrict__ g,
                                                                const float* __restrict__ g2, const float* __restrict__ noise, float p,
                                                                float scale, float sqrt_e, float* __restrict__ dE, long long n, int E,
                                                                int accumulate) {
  __shared__ int list[TX_CHUNK];
  __shared__ int cnt[TX_TPB];
  const int tid = threadIdx.x, e = blockIdx.y * TX_TPB + tid;
  const long long v = blockIdx.x;
  float acc = 0.f;
  for (long long c0 = 0; c0 < n; c0 += TX_CHUNK) {
    const long long lo = c0 + (long long)tid * TX_PER;
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < TX_PER; ++k)
      if (lo + k < n && tok[lo + k] == v) bits |= 1u << k;
    cnt[tid] = __popc(bits);
    __syncthreads();
    int off = 0, total = 0;
    for (int t = 0; t < TX_TPB; ++t) {
      const int c = cnt[t];
      off += t < tid ? c : 0;
      total += c;
    }
#pragma unroll
    for (int k = 0; k < TX_PER; ++k)
      if (bits >> k & 1u) list[off++] = tid * TX_PER + k;  // off stays below total <= TX_CHUNK
    __syncthreads();
    if (e < E) {
      for (int j = 0; j < total; ++j) {
        const long long i = (c0 + list[j]) * E + e;
        float gv = g[i];
        if (g2) gv += g2[i];
        acc += tx_kept(noise, i, p) ? gv * scale : 0.f;
      }
    }
    __syncthreads();  // the list and the counts are rewritten by the next chunk
  }
  if (e < E) {
    const float r = sqrt_e * acc;
    dE[v * E + e] = accumulate ? dE[v * E + e] + r : r;
  }
}

__global__ __launch_bounds__(TX_TPB) void tx_attn_fwd_kernel(const float* __restrict__ qkv, const int* __restrict__ keymask,
                                                               const float* __restrict__ noise, float p, float scale,
                                                               float* __restrict__ P, float* __restrict__ ctx, int S, int E, int nh) {
  extern __shared__ __attribute__((aligned(16))) float tx_lds[];
  const int hd = E / nh, HP = hd + 1, SP = S + 1;
  float* q = tx_lds;          // [S][HP]
  float* k = q + S * HP;      // [S][HP]
  float* v = k + S * HP;      // [S][HP]
  float* sc = v + S * HP;     // [S][SP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / nh, h = blockIdx.x % nh;
  const float qs = 1.f / sqrtf((float)hd);
  for (int idx = tid; idx < S * hd; idx += TX_TPB) {
    const int i = idx / hd, d = idx % hd;
    const float* src = qkv + ((long long)b * S + i) * 3 * E + h * hd + d;
    q[i * HP + d] = src[0] * qs;
    k[i * HP + d] = src[E];
    v[i * HP + d] = src[2 * E];
  }
  __syncthreads();
  for (int idx = tid; idx < S * S; idx += TX_TPB) {
    const int i = idx / S, j = idx % S;
    const float *qi = q + i * HP, *kj = k + j * HP;
    float acc = 0.f;
    for (int d = 0; d < hd; ++d) acc = fmaf(qi[d], kj[d], acc);
    sc[i * SP + j] = (keymask && keymask[(long long)b * S + j] == 0) ? -INFINITY : acc;
  }
  __syncthreads();
  for (int i = wave; i < S; i += TX_WAVES) {  // lane j: column j of row i
    const float x = lane < S ? sc[i * SP + lane] : -INFINITY;
    const float m = wave_max(x);
    const float ex = lane < S ? expf(x - m) : 0.f;  // a row of -inf: -inf - -inf = NaN, as torch
    const float pr = ex / wave_sum(ex);
    if (lane < S) {
      const long long gi = (((long long)b * nh + h) * S + i) * S + lane;
      if (P) P[gi] = pr;
      sc[i * SP + lane] = tx_kept(noise, gi, p) ? pr * scale : 0.f;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < S * hd; idx += TX_TPB) {
    const int i = idx / hd, d = idx % hd;
    const float* pi = sc + i * SP;
    float acc = 0.f;
    for (int j = 0; j < S; ++j) acc = fmaf(pi[j], v[j * HP + d], acc);
    ctx[((long long)b * S + i) * E + h * hd + d] = acc;
  }
}

__global__ __launch_bounds__(TX_TPB) void tx_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                               const float* __restrict__ dctx, const float* __restrict__ noise, float p,
                                                               float scale, float* __restrict__ dqkv, int S, int E, int nh) {
  extern __shared__ __attribute__((aligned(16))) float tx_lds[];
  const int hd = E / nh, HP = hd + 1, SP = S + 1;
  float* ta = tx_lds;          // [S][HP]: V, then K
  float* tb = ta + S * HP;     // [S][HP]: dctx, then Q
  float* pm = tb + S * HP;     // [S][SP]: P
  float* gm = pm + S * SP;     // [S][SP]: P o D, then dP, then dS
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / nh, h = blockIdx.x % nh;
  const float qs = 1.f / sqrtf((float)hd);
  const long long pbase = ((long long)b * nh + h) * S * S;
  for (int idx = tid; idx < S * hd; idx += TX_TPB) {
    const int i = idx / hd, d = idx % hd;
    ta[i * HP + d] = qkv[((long long)b * S + i) * 3 * E + 2 * E + h * hd + d];
    tb[i * HP + d] = dctx[((long long)b * S + i) * E + h * hd + d];
  }
  for (int idx = tid; idx < S * S; idx += TX_TPB) {
    const int i = idx / S, j = idx % S;
    const float pr = P[pbase + idx];
    pm[i * SP + j] = pr;
    gm[i * SP + j] = tx_kept(noise, pbase + idx, p) ? pr * scale : 0.f;
  }
  __syncthreads();
  // dV[j][d] = sum_i (P o D)[i][j] dctx[i][d]
  for (int idx = tid; idx < S * hd; idx += TX_TPB) {
    const int j = idx / hd, d = idx % hd;
    float acc = 0.f;
    for (int i = 0; i < S; ++i) acc = fmaf(gm[i * SP + j], tb[i * HP + d], acc);
    dqkv[((long long)b * S + j) * 3 * E + 2 * E + h * hd + d] = acc;
  }
  __syncthreads();
  // dP[i][j] = (sum_d dctx[i][d] V[j][d]) D[i][j]
  for (int idx = tid; idx < S * S; idx += TX_TPB) {
    const int i = idx / S, j = idx % S;
    const float *di = tb + i * HP, *vj = ta + j * HP;
    float acc = 0.f;
    for (int d = 0; d < hd; ++d) acc = fmaf(di[d], vj[d], acc);
    gm[i * SP + j] = tx_kept(noise, pbase + idx, p) ? acc * scale : 0.f;
  }
  __syncthreads();  // the last readers of V and dctx
  for (int idx = tid; idx < S * hd; idx += TX_TPB) {
    const int i = idx / hd, d = idx % hd;
    const float* src = qkv + ((long long)b * S + i) * 3 * E + h * hd + d;
    ta[i * HP + d] = src[E];
    tb[i * HP + d] = src[0];
  }
  // dS = P o (dP - rowsum(dP o P)): a wave per row
  for (int i = wave; i < S; i += TX_WAVES) {
    const float pr = lane < S ? pm[i * SP + lane] : 0.f, dp = lane < S ? gm[i * SP + lane] : 0.f;
    const float r = wave_sum(dp * pr);
    if (lane < S) gm[i * SP + lane] = pr * (dp - r);
  }
  __syncthreads();
  // dQ[i][d] = sum_j dS[i][j] K[j][d] / sqrt(hd), dK[j][d] = sum_i dS[i][j] Q[i][d] / sqrt(hd)
  for (int idx = tid; idx < S * hd; idx += TX_TPB) {
    const int r = idx / hd, d = idx % hd;
    float aq = 0.f, ak = 0.f;
    for (int j = 0; j < S; ++j) {
      aq = fmaf(gm[r * SP + j], ta[j * HP + d], aq);
      ak = fmaf(gm[j * SP + r], tb[j * HP + d], ak);
    }
    float* dst = dqkv + ((long long)b * S + r) * 3 * E + h * hd + d;
    dst[0] = aq * qs;
    dst[E] = ak * qs;
  }
}

__global__ __launch_bounds__(TX_TPB) void tx_add_ln_fwd_kernel(const float* __restrict__ x, const float* t, const float* __restrict__ noise,
                                                                 float p, float scale, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, const int* __restrict__ rowmask,
                                                                 int zero_pads, float* __restrict__ y, float* z, float* __restrict__ mean,
                                                                 float* __restrict__ rstd, long long rows, int E) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * TX_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;  // whole waves leave; no barrier below
  const long long r0 = row * E;
  float* zb = z ? z : y;  // a lane re-reads only what it wrote itself
  float s = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float tv = t[r0 + e];
    const float zv = x[r0 + e] + (tx_kept(noise, r0 + e, p) ? tv * scale : 0.f);
    zb[r0 + e] = zv;
    s += zv;
  }
  const float mu = wave_sum(s) / (float)E;
  float q = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float c = zb[r0 + e] - mu;
    q = fmaf(c, c, q);
  }
  const float rs = 1.f / sqrtf(wave_sum(q) / (float)E + eps);
  const bool zero = zero_pads && rowmask && rowmask[row] == 0;
  for (int e = lane; e < E; e += 64) {
    const float xh = (zb[r0 + e] - mu) * rs;
    const float o = fmaf(xh, gamma ? gamma[e] : 1.f, beta ? beta[e] : 0.f);
    y[r0 + e] = zero ? 0.f : o;
  }
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
}

__global__ __launch_bounds__(TX_TPB) void tx_add_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dy2,
                                                                 const float* __restrict__ z, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ noise, float p, float scale,
                                                                 float* __restrict__ dx, float* __restrict__ dt, long long rows, int E) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * TX_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long r0 = row * E;
  const float mu = mean[row], rs = rstd[row];
  float s1 = 0.f, s2 = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float gv = (dy[r0 + e] + (dy2 ? dy2[r0 + e] : 0.f)) * (gamma ? gamma[e] : 1.f);
    s1 += gv;
    s2 = fmaf(gv, (z[r0 + e] - mu) * rs, s2);
  }
  const float m1 = wave_sum(s1) / (float)E, m2 = wave_sum(s2) / (float)E;
  for (int e = lane; e < E; e += 64) {
    const float gv = (dy[r0 + e] + (dy2 ? dy2[r0 + e] : 0.f)) * (gamma ? gamma[e] : 1.f);
    const float d = rs * ((gv - m1) - (z[r0 + e] - mu) * rs * m2);
    dx[r0 + e] = d;
    if (dt) dt[r0 + e] = tx_kept(noise, r0 + e, p) ? d * scale : 0.f;
  }
}

// ws[slab][0][e] = sum over the slab's rows of (dy + dy2) xh, ws[slab][1][e] = of (dy + dy2), rows in order
__global__ __launch_bounds__(TX_TPB) void tx_ln_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ dy2,
                                                                const float* __restrict__ z, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, float* __restrict__ ws, long long rows, int E) {
  const int e = blockIdx.x * TX_TPB + threadIdx.x;
  if (e >= E) return;
  const long long ra = (long long)blockIdx.y * TX_SLAB, rb = ra + TX_SLAB < rows ? ra + TX_SLAB : rows;
  float a = 0.f, c = 0.f;
  for (long long r = ra; r < rb; ++r) {
    const float gv = dy[r * E + e] + (dy2 ? dy2[r * E + e] : 0.f);
    a = fmaf(gv, (z[r * E + e] - mean[r]) * rstd[r], a);
    c += gv;
  }
  ws[((long long)blockIdx.y * 2) * E + e] = a;
  ws[((long long)blockIdx.y * 2 + 1) * E + e] = c;
}

__global__ __launch_bounds__(TX_TPB) void tx_ln_colsum_finish_kernel(const float* __restrict__ ws, float* __restrict__ dgamma,
                                                                       float* __restrict__ dbeta, int nslab, int E) {
  const int e = blockIdx.x * TX_TPB + threadIdx.x;
  if (e >= E) return;
  float a = 0.f, c = 0.f;
  for (int s = 0; s < nslab; ++s) {
    a += ws[((long long)s * 2) * E + e];
    c += ws[((long long)s * 2 + 1) * E + e];
  }
  if (dgamma) dgamma[e] += a;
  if (dbeta) dbeta[e] += c;
}

__global__ __launch_bounds__(TX_TPB) void tx_drop_kernel(float* __restrict__ x, const float* __restrict__ noise, float p, float scale,
                                                           long long n) {
  for (long long i = (long long)blockIdx.x * TX_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TX_TPB)
    x[i] = noise[i] >= p ? x[i] * scale : 0.f;
}

// p == 0 or no noise: no dropout (the kernels see a null noise pointer and scale 1)
inline bool tx_p_ok(float p) { return p >= 0.f && p < 1.f; }
inline const float* tx_noise(const float* noise, float p) { return p > 0.f ? noise : nullptr; }
inline float tx_scale(const float* noise, float p) { return (noise && p > 0.f) ? 1.f / (1.f - p) : 1.f; }

inline bool tx_attn_ok(int B, int S, int E, int nh) {
  return B >= 1 && S >= 1 && S <= MVK_TXT_MAX_SEQ && nh >= 1 && E >= nh && E % nh == 0 && E / nh <= MVK_TXT_MAX_HEAD_DIM &&
         (long long)B * nh <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int mvk_txt_embed_fwd(const int64_t* tokens, const float* emb, const float* pe, const float* noise, float p, float* out, int B, int S,
                      int E, int V, void* stream) {
  if (!tokens || !emb || !pe || !out || B < 1 || S < 1 || E < 1 || V < 1 || !tx_p_ok(p)) return MVK_EINVAL;
  const long long rows = (long long)B * S;
  if (rows > 0x7fffffffLL) return MVK_EINVAL;
  const float* nz = tx_noise(noise, p);
  hipLaunchKernelGGL(tx_embed_fwd_kernel, dim3((unsigned)rows), dim3(TX_TPB), 0, mvk_stream(stream),
                     reinterpret_cast<const long long*>(tokens), emb, pe, nz, p, tx_scale(nz, p), sqrtf((float)E), out, S, E, V);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_txt_embed_bwd(const int64_t* tokens, const float* g, const float* g2, const float* noise, float p, float* dE, int accumulate,
                      int B, int S, int E, int V, void* stream) {
  if (!tokens || !g || !dE || B < 1 || S < 1 || E < 1 || V < 1 || !tx_p_ok(p)) return MVK_EINVAL;
  const int eb = (E + TX_TPB - 1) / TX_TPB;
  if (eb > 65535) return MVK_EINVAL;
  const float* nz = tx_noise(noise, p);
  hipLaunchKernelGGL(tx_embed_bwd_kernel, dim3((unsigned)V, (unsigned)eb), dim3(TX_TPB), 0, mvk_stream(stream),
                     reinterpret_cast<const long long*>(tokens), g, g2, nz, p, tx_scale(nz, p), sqrtf((float)E), dE, (long long)B * S, E,
                     accumulate);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_txt_attn_fwd(const float* qkv, const int32_t* keymask, const float* noise, float p, float* P, float* ctx, int B, int S, int E,
                     int nhead, void* stream) {
  if (!qkv || !ctx || !tx_attn_ok(B, S, E, nhead) || !tx_p_ok(p)) return MVK_EINVAL;
  const int hd = E / nhead;
  const int lds = (3 * S * (hd + 1) + S * (S + 1)) * (int)sizeof(float);
  static_assert((3 * MVK_TXT_MAX_SEQ * (MVK_TXT_MAX_HEAD_DIM + 1) + MVK_TXT_MAX_SEQ * (MVK_TXT_MAX_SEQ + 1)) * 4 <= 160 * 1024,
                "one workgroup's LDS");
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(tx_attn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  const float* nz = tx_noise(noise, p);
  hipLaunchKernelGGL(tx_attn_fwd_kernel, dim3((unsigned)(B * nhead)), dim3(TX_TPB), lds, mvk_stream(stream), qkv, keymask, nz, p,
                     tx_scale(nz, p), P, ctx, S, E, nhead);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_txt_attn_bwd(const float* qkv, const float* P, const float* dctx, const float* noise, float p, float* dqkv, int B, int S, int E,
                     int nhead, void* stream) {
  if (!qkv || !P || !dctx || !dqkv || !tx_attn_ok(B, S, E, nhead) || !tx_p_ok(p)) return MVK_EINVAL;
  const int hd = E / nhead;
  const int lds = (2 * S * (hd + 1) + 2 * S * (S + 1)) * (int)sizeof(float);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(tx_attn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  const float* nz = tx_noise(noise, p);
  hipLaunchKernelGGL(tx_attn_bwd_kernel, dim3((unsigned)(B * nhead)), dim3(TX_TPB), lds, mvk_stream(stream), qkv, P, dctx, nz, p,
                     tx_scale(nz, p), dqkv, S, E, nhead);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_txt_add_ln_fwd(const float* x, const float* t, const float* noise, float p, const float* gamma, const float* beta, float eps,
                       const int32_t* rowmask, int zero_pads, float* y, float* z, float* mean, float* rstd, int64_t rows, int E,
                       void* stream) {
  if (!x || !t || !y || y == x || y == t || rows < 1 || E < 1 || !tx_p_ok(p) || !(eps >= 0.f)) return MVK_EINVAL;
  const long long blocks = ((long long)rows + TX_WAVES - 1) / TX_WAVES;
  if (blocks > 0x7fffffffLL) return MVK_EINVAL;
  const float* nz = tx_noise(noise, p);
  hipLaunchKernelGGL(tx_add_ln_fwd_kernel, dim3((unsigned)blocks), dim3(TX_TPB), 0, mvk_stream(stream), x, t, nz, p, tx_scale(nz, p), gamma,
                     beta, eps, rowmask, zero_pads, y, z, mean, rstd, (long long)rows, E);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_txt_add_ln_bwd(const float* dy, const float* dy2, const float* z, const float* mean, const float* rstd, const float* gamma,
                       const float* noise, float p, float* dx, float* dt, float* dgamma, float* dbeta, float* ws, int64_t ws_floats,
                       int64_t rows, int E, void* stream) {
  if (!dy || !z || !mean || !rstd || !dx || rows < 1 || E < 1 || !tx_p_ok(p)) return MVK_EINVAL;
  const long long blocks = ((long long)rows + TX_WAVES - 1) / TX_WAVES, nslab = ((long long)rows + TX_SLAB - 1) / TX_SLAB;
  const int eb = (E + TX_TPB - 1) / TX_TPB;
  if (blocks > 0x7fffffffLL || nslab > 65535 || eb > 65535) return MVK_EINVAL;
  const bool sums = dgamma || dbeta;
  if (sums && (!ws || ws_floats < 2LL * E * nslab)) return MVK_EINVAL;
  const float* nz = tx_noise(noise, p);
  hipLaunchKernelGGL(tx_add_ln_bwd_kernel, dim3((unsigned)blocks), dim3(TX_TPB), 0, mvk_stream(stream), dy, dy2, z, mean, rstd, gamma, nz,
                     p, tx_scale(nz, p), dx, dt, (long long)rows, E);
  MVK_CHECK_LAUNCH();
  if (sums) {
    hipLaunchKernelGGL(tx_ln_colsum_kernel, dim3((unsigned)eb, (unsigned)nslab), dim3(TX_TPB), 0, mvk_stream(stream), dy, dy2, z, mean, rstd,
                       ws, (long long)rows, E);
    MVK_CHECK_LAUNCH();
    hipLaunchKernelGGL(tx_ln_colsum_finish_kernel, dim3((unsigned)eb), dim3(TX_TPB), 0, mvk_stream(stream), ws, dgamma, dbeta, (int)nslab, E);
    MVK_CHECK_LAUNCH();
  }
  return MVK_OK;
}

int mvk_txt_drop(float* x, const float* noise, float p, int64_t n, void* stream) {
  if (!x || n < 1 || !tx_p_ok(p)) return MVK_EINVAL;
  const float* nz = tx_noise(noise, p);
  if (!nz) return MVK_OK;  // nothing is dropped and the scale is 1
  long long blocks = ((long long)n + TX_TPB - 1) / TX_TPB;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(tx_drop_kernel, dim3((unsigned)blocks), dim3(TX_TPB), 0, mvk_stream(stream), x, nz, p, tx_scale(nz, p), (long long)n);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
