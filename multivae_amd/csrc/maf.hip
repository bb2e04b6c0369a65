// Masked autoregressive flows (MAF: a stack of MADE blocks, models/nn/flows.py) for JNF (models/jnf/jnf_model.py): the flows of ALL
// modalities forward in one launch, their backward in two, and the sequential inverse of one flow in one.  Further down, the same
// MADEs run the other way round: the inverse autoregressive flow (IAF) of the flow samplers (samplers/iaf_sampler), ONE flow, its
// sequential forward in one launch, its backward in two and its one-pass inverse in one.
//
// One MADE is n_hidden + 1 masked linear layers: [H,D], (n_hidden - 1) x [H,H], [2D,H], ReLU between them.  With deg(k) = k % (D - 1)
// for a hidden unit k the masks are index arithmetic (degrees_ordering = "sequential"):
//   layer 0:       W[o,k] counts when deg(o) >= k            (k an input coordinate)
//   hidden layers: W[o,k] counts when deg(o) >= deg(k)
//   output layer:  W[d,k] and W[D+d,k] count when deg(k) < d (rows d: mu, rows D+d: the log-scale "log_var")
// The kernels never read a mask buffer, and a masked weight's value does not reach a result (not even a NaN there: where such a
// weight is loaded at all, it is replaced by 0 before it is used).
// One block of the flow: u = (x - mu(x)) exp(-lv(x)); ladj -= sum_d lv; x' = flip(u).
//
// Everything is fp32 FMA with fp32 sums in a fixed order (no atomics): a result is bit-reproducible run to run.
//   forward:  a workgroup of four waves owns RT = 4 rows of one flow, activations in LDS; one wave per output unit (four units per
//             round), its lanes stride over the input index (coalesced weight rows), the row sums folded by wave_sum_dpp.
//   backward: the same tile; one THREAD per input index k (weight columns are coalesced across lanes), the deltas of the tile's four
//             rows sit side by side in LDS ([unit][RT]: one broadcast b128 read per weight).  A second launch sums
//             delta^T activation over the batch, one thread per weight entry, four interleaved partial sums in a fixed order.
//   inverse:  x_i depends on x_0..x_{i-1} only, and a hidden unit of degree g on x_0..x_g only: step i computes the hidden units of
//             degree i - 1 of every layer (final from then on) and the two outputs mu_i, lv_i — ONE pass over the weights per
//             block, in D steps.
#include "common.hpp"

namespace {

constexpr int MAXM = MVK_MAX_MODALITIES;
constexpr int RT = 4;  // rows of a workgroup's tile
constexpr int MAXL = MVK_MAF_MAX_BLOCKS * (MVK_MAF_MAX_HIDDEN + 1);  // linear layers of one flow
constexpr float LOG_2PI = 1.8378770664093453f;

struct MafW {
  const float* w[MAXM * MAXL];
};
struct MafWB {
  const float* w[MAXM * MAXL];
  const float* b[MAXM * MAXL];
};
struct MafGW {
  float* w[MAXM * MAXL];
  float* b[MAXM * MAXL];
};
struct MafPost {
  const float* mu[MAXM];
  const float* lv[MAXM];
};
struct MafGPost {
  float* mu[MAXM];
  float* lv[MAXM];
};
struct MafWB1 {
  const float* w[MAXL];
  const float* b[MAXL];
};
struct MafW1 {
  const float* w[MAXL];
};

// floats one (flow, block) takes in the forward's workspace and in the deltas: [B,D] + [B,D] + n_hidden x [B,H]
__host__ __device__ inline long long chunk_floats(int B, int D, int H, int nh) { return (long long)B * (2 * D + (long long)nh * H); }

// (sum over the wave's k of pred(k) ? w[k] * act[r * lda + k] : 0) for the tile's four rows r, the same totals in every lane
template <class Pred>
__device__ __forceinline__ float4 wave_dot(const float* __restrict__ w, const float* act, int lda, int K, int lane, Pred pred) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = lane; k < K; k += 64) {
    if (pred(k)) {
      const float wv = w[k];
      a0 = fmaf(wv, act[k], a0);
      a1 = fmaf(wv, act[lda + k], a1);
      a2 = fmaf(wv, act[2 * lda + k], a2);
      a3 = fmaf(wv, act[3 * lda + k], a3);
    }
  }
  return make_float4(wave_sum_dpp(a0), wave_sum_dpp(a1), wave_sum_dpp(a2), wave_sum_dpp(a3));
}

__device__ __forceinline__ float pick(const float4 a, int r) { return r == 0 ? a.x : r == 1 ? a.y : r == 2 ? a.z : a.w; }

// kind 0: layer 0 (in = x), 1: hidden layer, 2: output layer.  out[r * ldo + o] for o < N; the caller synchronises.
// A wave takes FOUR output units per round (o, o + 4, o + 8, o + 12): their weight loads are in flight together, where one unit
// per round waits out one memory latency per unit.  W[o,k] counts when lhs(k) <= thr(o): lhs = k (layer 0) or deg(k), thr = deg(o)
// or d - 1 (output layer); a weight that does not count is loaded (every address is inside the matrix) and replaced by 0.
__device__ __forceinline__ void made_layer(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int ldi,
                                           int K, float* out, int ldo, int N, int kind, int D, const int* deg) {
  static_assert(RT == 4, "wave_dot and the b128 delta reads are written for four rows");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = wave; o < N; o += 16) {
    int oj[4], thr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      oj[j] = o + 4 * j < N ? o + 4 * j : N - 1;  // a unit past the end repeats the last one and is not written
      thr[j] = kind == 2 ? (oj[j] < D ? oj[j] : oj[j] - D) - 1 : deg[oj[j]];
    }
    float a[4][RT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < RT; ++r) a[j][r] = 0.f;
    for (int k = lane; k < K; k += 64) {
      const int lhs = kind == 0 ? k : deg[k];
      float w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = W[(long long)oj[j] * K + k];
      const float x0 = in[k], x1 = in[ldi + k], x2 = in[2 * ldi + k], x3 = in[3 * ldi + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float wv = lhs <= thr[j] ? w[j] : 0.f;
        a[j][0] = fmaf(wv, x0, a[j][0]);
        a[j][1] = fmaf(wv, x1, a[j][1]);
        a[j][2] = fmaf(wv, x2, a[j][2]);
        a[j][3] = fmaf(wv, x3, a[j][3]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 acc = make_float4(wave_sum_dpp(a[j][0]), wave_sum_dpp(a[j][1]), wave_sum_dpp(a[j][2]), wave_sum_dpp(a[j][3]));
      if (lane < RT && o + 4 * j < N) {
        const float v = pick(acc, lane) + bias[oj[j]];
        out[lane * ldo + oj[j]] = kind == 2 ? v : fmaxf(v, 0.f);
      }
    }
  }
}

// LDS: xs [RT,D] | bufA [RT,S] | bufB [RT,S] | lad [RT] | deg [H]   (S = max(H, 2D))
__global__ __launch_bounds__(256) void maf_fwd_kernel(const MafWB net, const MafPost post, int has_post,
                                                      const float* __restrict__ z, int nb, int nh, int D, int H, int B,
                                                      float* __restrict__ z0, float* __restrict__ ladj,
                                                      float* __restrict__ rows, float* __restrict__ ws) {
  extern __shared__ float lds[];
  const int S = H > 2 * D ? H : 2 * D;
  float* xs = lds;
  float* bufA = xs + RT * D;
  float* bufB = bufA + RT * S;
  float* lad = bufB + RT * S;
  int* deg = reinterpret_cast<int*>(lad + RT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.y, b0 = blockIdx.x * RT;
  const int nl = nh + 1;
  const long long CH = chunk_floats(B, D, H, nh);

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    xs[i] = b < B ? z[(long long)b * D + c] : 0.f;
  }
  for (int k = tid; k < H; k += 256) deg[k] = k % (D - 1);
  if (tid < RT) lad[tid] = 0.f;
  __syncthreads();

  for (int blk = 0; blk < nb; ++blk) {
    const int l0 = (m * nb + blk) * nl;
    float* wsx = ws ? ws + (long long)(m * nb + blk) * CH : nullptr;
    if (wsx)
      for (int i = tid; i < RT * D; i += 256) {
        const int r = i / D, c = i - r * D, b = b0 + r;
        if (b < B) wsx[(long long)b * D + c] = xs[i];
      }
    const float* in = xs;
    int ldi = D, K = D;
    float* out = bufA;
    for (int l = 0; l < nh; ++l) {
      made_layer(net.w[l0 + l], net.b[l0 + l], in, ldi, K, out, H, H, l == 0 ? 0 : 1, D, deg);
      __syncthreads();
      if (wsx) {
        float* wh = wsx + 2LL * B * D + (long long)l * B * H;
        for (int i = tid; i < RT * H; i += 256) {
          const int r = i / H, c = i - r * H, b = b0 + r;
          if (b < B) wh[(long long)b * H + c] = out[i];
        }
      }
      in = out;
      ldi = H;
      K = H;
      out = out == bufA ? bufB : bufA;
    }
    made_layer(net.w[l0 + nh], net.b[l0 + nh], in, ldi, K, out, 2 * D, 2 * D, 2, D, deg);
    __syncthreads();
    // u = (x - mu) exp(-lv), flipped, into the buffer the last hidden layer no longer needs
    float* tmp = out == bufA ? bufB : bufA;
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, c = i - r * D, b = b0 + r;
      const float mu = out[r * 2 * D + c], lv = out[r * 2 * D + D + c];
      tmp[r * D + (D - 1 - c)] = (xs[i] - mu) * expf(-lv);
      if (wsx && b < B) wsx[(long long)B * D + (long long)b * D + c] = lv;
    }
    {  // wave r: ladj[r] -= sum_d lv[r,d]
      float s = 0.f;
      for (int c = lane; c < D; c += 64) s += out[wave * 2 * D + D + c];
      s = wave_sum_dpp(s);
      if (lane == 0) lad[wave] -= s;
    }
    __syncthreads();
    for (int i = tid; i < RT * D; i += 256) xs[i] = tmp[i];
    __syncthreads();
  }

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    if (b < B) z0[((long long)m * B + b) * D + c] = xs[i];
  }
  const int b = b0 + wave;  // wave r finishes row r
  if (b < B) {
    if (lane == 0) ladj[(long long)m * B + b] = lad[wave];
    if (has_post) {
      const float* __restrict__ mu0 = post.mu[m] + (long long)b * D;
      const float* __restrict__ lv0 = post.lv[m] + (long long)b * D;
      float s = 0.f;
      for (int c = lane; c < D; c += 64) {
        const float dlt = xs[wave * D + c] - mu0[c], v = lv0[c];
        s += -0.5f * (v + LOG_2PI + dlt * dlt * expf(-v));
      }
      s = wave_sum_dpp(s);
      if (lane == 0) rows[(long long)m * B + b] = -(s + lad[wave]);
    }
  }
}

// LDS: gx [RT,D] | gxn [RT,D] | dzs [RT,D] | dA [S,RT] | dB [S,RT] | gl [RT] | deg [H]
__global__ __launch_bounds__(256) void maf_bwd_data_kernel(const MafW net, const MafPost post, const MafGPost gpost, int has_post,
                                                           int M, int nb, int nh, int D, int H, int B,
                                                           const float* __restrict__ z0, const float* __restrict__ ws,
                                                           const float* __restrict__ grows, const float* __restrict__ dz0,
                                                           const float* __restrict__ dladj, float* __restrict__ dz,
                                                           float* __restrict__ deltas) {
  extern __shared__ float lds[];
  const int S = H > 2 * D ? H : 2 * D;
  float* gx = lds;
  float* gxn = gx + RT * D;
  float* dzs = gxn + RT * D;
  float* dA = dzs + RT * D;  // 16-byte aligned: 3 RT D floats in front, RT = 4
  float* dB = dA + S * RT;
  float* gl = dB + S * RT;
  int* deg = reinterpret_cast<int*>(gl + RT);
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * RT;
  const int nl = nh + 1;
  const long long CH = chunk_floats(B, D, H, nh);
  // with dz wanted (the sum over the flows in increasing m) one workgroup walks all flows of its rows
  const int m_first = dz ? 0 : blockIdx.y, m_last = dz ? M : m_first + 1;

  for (int k = tid; k < H; k += 256) deg[k] = k % (D - 1);

  for (int m = m_first; m < m_last; ++m) {
    __syncthreads();
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, c = i - r * D, b = b0 + r;
      float g = 0.f;
      if (b < B) {
        const long long at = ((long long)m * B + b) * D + c;
        if (has_post) {
          const float gr = grows ? grows[(long long)m * B + b] : 0.f;
          const long long pb = (long long)b * D + c;
          const float dlt = z0[at] - post.mu[m][pb], e = expf(-post.lv[m][pb]), t = dlt * e;
          g = gr * t;
          gpost.mu[m][pb] = -g;
          gpost.lv[m][pb] = gr * 0.5f * (1.f - dlt * t);
        }
        if (dz0) g += dz0[at];
      }
      gx[i] = g;
    }
    if (tid < RT) {
      const int b = b0 + tid;
      float g = 0.f;
      if (b < B) {
        if (has_post && grows) g = -grows[(long long)m * B + b];
        if (dladj) g += dladj[(long long)m * B + b];
      }
      gl[tid] = g;
    }
    __syncthreads();

    for (int blk = nb - 1; blk >= 0; --blk) {
      const int l0 = (m * nb + blk) * nl;
      const float* wsx = ws + (long long)(m * nb + blk) * CH;
      const float* wlv = wsx + (long long)B * D;
      // this block's output u, unflipped: the next block's saved input, or z0 behind the last block
      const float* unext = blk == nb - 1 ? z0 + (long long)m * B * D : wsx + CH;
      float* dl = deltas ? deltas + (long long)(m * nb + blk) * CH : nullptr;
      float* cur = dA;
      float* nxt = dB;
      for (int i = tid; i < RT * D; i += 256) {
        const int r = i / D, c = i - r * D, b = b0 + r;
        float dmu = 0.f, dlv = 0.f, dx = 0.f;
        if (b < B) {
          const float gu = gx[r * D + (D - 1 - c)];
          const float lv = wlv[(long long)b * D + c], u = unext[(long long)b * D + (D - 1 - c)], e = expf(-lv);
          dx = gu * e;
          dmu = -dx;
          dlv = -gu * u - gl[r];
          if (dl) {
            dl[(long long)b * 2 * D + c] = dmu;
            dl[(long long)b * 2 * D + D + c] = dlv;
          }
        }
        cur[c * RT + r] = dmu;
        cur[(D + c) * RT + r] = dlv;
        gxn[i] = dx;
      }
      __syncthreads();
      for (int l = nh; l >= 0; --l) {
        const float* __restrict__ W = net.w[l0 + l];
        const int N = l == nh ? 2 * D : H, K = l == 0 ? D : H;
        for (int k = tid; k < K; k += 256) {
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
          const int dk = l == 0 ? k : deg[k];
          // a weight that does not count is loaded (the address is inside the matrix) and replaced by 0: the loads of an unrolled
          // group are in flight together instead of one memory latency per output unit
#pragma unroll 8
          for (int o = 0; o < N; ++o) {
            const bool on = l == nh ? dk < (o < D ? o : o - D) : deg[o] >= dk;
            const float wl = W[(long long)o * K + k];
            const float wv = on ? wl : 0.f;
            const float4 d4 = *reinterpret_cast<const float4*>(cur + o * RT);
            a0 = fmaf(wv, d4.x, a0);
            a1 = fmaf(wv, d4.y, a1);
            a2 = fmaf(wv, d4.z, a2);
            a3 = fmaf(wv, d4.w, a3);
          }
          const float a[RT] = {a0, a1, a2, a3};
          if (l == 0) {
#pragma unroll
            for (int r = 0; r < RT; ++r) gxn[r * D + k] += a[r];
          } else {
            const float* hprev = wsx + 2LL * B * D + (long long)(l - 1) * B * H;
            float* dh = dl ? dl + 2LL * B * D + (long long)(l - 1) * B * H : nullptr;
#pragma unroll
            for (int r = 0; r < RT; ++r) {
              const int b = b0 + r;
              float v = 0.f;
              if (b < B) {
                v = hprev[(long long)b * H + k] > 0.f ? a[r] : 0.f;
                if (dh) dh[(long long)b * H + k] = v;
              }
              nxt[k * RT + r] = v;
            }
          }
        }
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
      }
      float* t = gx;
      gx = gxn;
      gxn = t;
    }
    if (dz)
      for (int i = tid; i < RT * D; i += 256) dzs[i] = m == 0 ? gx[i] : dzs[i] + gx[i];
  }
  if (dz) {
    __syncthreads();
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, c = i - r * D, b = b0 + r;
      if (b < B) dz[(long long)b * D + c] = dzs[i];
    }
  }
}

// dW[o,k] += sum_b delta[b,o] in[b,k] (unmasked entries only), db[o] += sum_b delta[b,o]; blockIdx.y = (flow, block, layer)
__global__ __launch_bounds__(256) void maf_bwd_weight_kernel(const MafGW g, int nh, int D, int H, int B,
                                                             const float* __restrict__ ws, const float* __restrict__ deltas) {
  const int nl = nh + 1;
  const int fl = blockIdx.y, l = fl % nl, fb = fl / nl;
  const int N = l == nh ? 2 * D : H, K = l == 0 ? D : H;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * K) return;
  const int o = (int)(idx / K), k = (int)(idx - (long long)o * K);
  const long long CH = chunk_floats(B, D, H, nh);
  const float* in = ws + fb * CH + (l == 0 ? 0 : 2LL * B * D + (long long)(l - 1) * B * H);
  const float* dl = deltas + fb * CH + (l == nh ? 0 : 2LL * B * D + (long long)l * B * H);
  const int dk = l == 0 ? k : k % (D - 1);
  const bool on = l == nh ? dk < (o < D ? o : o - D) : (o % (D - 1)) >= dk;
  if (on && g.w[fl]) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};  // rows b = j mod 4 each in increasing order, then (s0 + s1) + (s2 + s3)
    int b = 0;
    for (; b + 4 <= B; b += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = fmaf(dl[(long long)(b + j) * N + o], in[(long long)(b + j) * K + k], s[j]);
    }
    for (int j = 0; b < B; ++b, ++j) s[j] = fmaf(dl[(long long)b * N + o], in[(long long)b * K + k], s[j]);
    g.w[fl][idx] += (s[0] + s[1]) + (s[2] + s[3]);
  }
  if (k == 0 && g.b[fl]) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 4 <= B; b += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += dl[(long long)(b + j) * N + o];
    }
    for (int j = 0; b < B; ++b, ++j) s[j] += dl[(long long)b * N + o];
    g.b[fl][o] += (s[0] + s[1]) + (s[2] + s[3]);
  }
}

// LDS: cur [RT,D] | ys [RT,D] | hs [nh][RT,H] | lad [RT] | deg [H]
__global__ __launch_bounds__(256) void maf_inverse_kernel(const MafWB1 net, const float* __restrict__ y, int nb, int nh, int D,
                                                          int H, int R, float* __restrict__ x, float* __restrict__ ladj) {
  extern __shared__ float lds[];
  float* cur = lds;
  float* ys = cur + RT * D;
  float* hs = ys + RT * D;
  float* lad = hs + nh * RT * H;
  int* deg = reinterpret_cast<int*>(lad + RT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * RT;
  const int nl = nh + 1;

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    cur[i] = b < R ? y[(long long)b * D + c] : 0.f;
  }
  for (int k = tid; k < H; k += 256) deg[k] = k % (D - 1);
  if (tid < RT) lad[tid] = 0.f;
  __syncthreads();

  float4 acc, acc2;
  for (int blk = nb - 1; blk >= 0; --blk) {
    const int l0 = blk * nl;
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, c = i - r * D;
      ys[r * D + (D - 1 - c)] = cur[i];
    }
    __syncthreads();
    // cur becomes x, coordinate by coordinate; what is read of it at step i (x_0 .. x_{i-1}) has been written by then
    for (int i = 0; i < D; ++i) {
      if (i > 0) {
        const int g = i - 1;  // the hidden units of degree g are final now
        for (int l = 0; l < nh; ++l) {
          const float* __restrict__ W = net.w[l0 + l];
          const float* __restrict__ bias = net.b[l0 + l];
          float* out = hs + l * RT * H;
          for (int o = g + wave * (D - 1); o < H; o += 4 * (D - 1)) {
            if (l == 0)
              acc = wave_dot(W + (long long)o * D, cur, D, D, lane, [=](int k) { return k <= g; });
            else
              acc = wave_dot(W + (long long)o * H, out - RT * H, H, H, lane, [=](int k) { return deg[k] <= g; });
            if (lane < RT) out[lane * H + o] = fmaxf(pick(acc, lane) + bias[o], 0.f);
          }
          __syncthreads();
        }
      }
      if (wave == 0) {
        const float* __restrict__ W = net.w[l0 + nh];
        const float* __restrict__ bias = net.b[l0 + nh];
        const float* hl = hs + (nh - 1) * RT * H;
        acc = wave_dot(W + (long long)i * H, hl, H, H, lane, [=](int k) { return deg[k] < i; });
        acc2 = wave_dot(W + (long long)(D + i) * H, hl, H, H, lane, [=](int k) { return deg[k] < i; });
        if (lane < RT) {
          const float mu = pick(acc, lane) + bias[i], lv = pick(acc2, lane) + bias[D + i];
          cur[lane * D + i] = ys[lane * D + i] * expf(lv) + mu;
          lad[lane] += lv;
        }
      }
      __syncthreads();
    }
  }

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    if (b < R) x[(long long)b * D + c] = cur[i];
  }
  if (ladj && tid < RT && b0 + tid < R) ladj[b0 + tid] = lad[tid];
}

// ---- inverse autoregressive flow (IAF, models/nn/flows.py): ONE flow, the same MADEs run the other way round ------------------------
// One block: y_i = (x_i - m_i(y)) exp(-s_i(y)) for i = 0..D-1 from y = 0, ladj -= s_i; x' = flip(y)   ((m, s) = MADE(y)).
// Its inverse is one MADE pass: y = flip(y), x = y exp(s(y)) + m(y), ladj += sum_d s_d.

// wave_dot down a COLUMN of a row-major matrix: (sum over k of pred(k) ? w[k * stride] * act[r * lda + k] : 0)
template <class Pred>
__device__ __forceinline__ float4 wave_dot_col(const float* __restrict__ w, int stride, const float* act, int lda, int K, int lane,
                                               Pred pred) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = lane; k < K; k += 64) {
    if (pred(k)) {
      const float wv = w[(long long)k * stride];
      a0 = fmaf(wv, act[k], a0);
      a1 = fmaf(wv, act[lda + k], a1);
      a2 = fmaf(wv, act[2 * lda + k], a2);
      a3 = fmaf(wv, act[3 * lda + k], a3);
    }
  }
  return make_float4(wave_sum_dpp(a0), wave_sum_dpp(a1), wave_sum_dpp(a2), wave_sum_dpp(a3));
}

// The schedule of maf_inverse_kernel: step i makes the hidden units of degree i - 1 of every layer final, then m_i, s_i and y_i.
// LDS: xs [RT,D] | ys [RT,D] | ss [RT,D] | hs [nh][RT,H] | lad [RT] | deg [H]
__global__ __launch_bounds__(256) void iaf_fwd_kernel(const MafWB1 net, const float* __restrict__ x, int nb, int nh, int D, int H,
                                                      int B, float* __restrict__ z0, float* __restrict__ ladj,
                                                      float* __restrict__ rows, float* __restrict__ ws) {
  extern __shared__ float lds[];
  float* xs = lds;
  float* ys = xs + RT * D;
  float* ss = ys + RT * D;
  float* hs = ss + RT * D;
  float* lad = hs + nh * RT * H;
  int* deg = reinterpret_cast<int*>(lad + RT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * RT;
  const int nl = nh + 1;
  const long long CH = chunk_floats(B, D, H, nh);

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    xs[i] = b < B ? x[(long long)b * D + c] : 0.f;
  }
  for (int k = tid; k < H; k += 256) deg[k] = k % (D - 1);
  if (tid < RT) lad[tid] = 0.f;
  __syncthreads();

  float4 acc, acc2;
  for (int blk = 0; blk < nb; ++blk) {
    const int l0 = blk * nl;
    // ys becomes y, coordinate by coordinate; what is read of it at step i (y_0 .. y_{i-1}) has been written by then
    for (int i = 0; i < D; ++i) {
      if (i > 0) {
        const int g = i - 1;
        for (int l = 0; l < nh; ++l) {
          const float* __restrict__ W = net.w[l0 + l];
          const float* __restrict__ bias = net.b[l0 + l];
          float* out = hs + l * RT * H;
          for (int o = g + wave * (D - 1); o < H; o += 4 * (D - 1)) {
            if (l == 0)
              acc = wave_dot(W + (long long)o * D, ys, D, D, lane, [=](int k) { return k <= g; });
            else
              acc = wave_dot(W + (long long)o * H, out - RT * H, H, H, lane, [=](int k) { return deg[k] <= g; });
            if (lane < RT) out[lane * H + o] = fmaxf(pick(acc, lane) + bias[o], 0.f);
          }
          __syncthreads();
        }
      }
      if (wave == 0) {
        const float* __restrict__ W = net.w[l0 + nh];
        const float* __restrict__ bias = net.b[l0 + nh];
        const float* hl = hs + (nh - 1) * RT * H;
        acc = wave_dot(W + (long long)i * H, hl, H, H, lane, [=](int k) { return deg[k] < i; });
        acc2 = wave_dot(W + (long long)(D + i) * H, hl, H, H, lane, [=](int k) { return deg[k] < i; });
        if (lane < RT) {
          const float m = pick(acc, lane) + bias[i], s = pick(acc2, lane) + bias[D + i];
          ys[lane * D + i] = (xs[lane * D + i] - m) * expf(-s);
          ss[lane * D + i] = s;
          lad[lane] -= s;
        }
      }
      __syncthreads();
    }
    // every hidden unit (degrees 0 .. D - 2) is final: hs is MADE(y)'s hidden activations
    if (ws) {
      float* wsx = ws + (long long)blk * CH;
      for (int i = tid; i < RT * D; i += 256) {
        const int r = i / D, c = i - r * D, b = b0 + r;
        if (b < B) {
          wsx[(long long)b * D + c] = ys[i];
          wsx[(long long)B * D + (long long)b * D + c] = ss[i];
        }
      }
      for (int l = 0; l < nh; ++l) {
        float* wh = wsx + 2LL * B * D + (long long)l * B * H;
        for (int i = tid; i < RT * H; i += 256) {
          const int r = i / H, c = i - r * H, b = b0 + r;
          if (b < B) wh[(long long)b * H + c] = hs[l * RT * H + i];
        }
      }
    }
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, c = i - r * D;
      xs[r * D + (D - 1 - c)] = ys[i];
    }
    __syncthreads();
  }

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    if (b < B) z0[(long long)b * D + c] = xs[i];
  }
  const int b = b0 + wave;  // wave r finishes row r
  if (b < B) {
    if (lane == 0) ladj[b] = lad[wave];
    if (rows) {
      float s = 0.f;
      for (int c = lane; c < D; c += 64) {
        const float v = xs[wave * D + c];
        s += -0.5f * (LOG_2PI + v * v);
      }
      s = wave_sum_dpp(s);
      if (lane == 0) rows[b] = -(s + lad[wave]);
    }
  }
}

// The block's Jacobian in y is lower triangular (x_j = y_j exp(s_j(y)) + m_j(y)): the backward is a transposed triangular solve that
// interleaves with ONE backward pass of the MADE.  i = D-1 .. 0: the deltas of the hidden units of degree i (they need the output
// cotangents cm_j, cs_j of j > i only), last hidden layer first; v_i = the MADE's input gradient at coordinate i;
// lam_i = exp(-s_i) (gy_i + v_i); cm_i = -lam_i; cs_i = -gl - lam_i y_i exp(s_i).  dx = lam.
// LDS: g [RT,D] | c [RT,2D] | dl [nh][RT,H] | gl [RT] | deg [H]
__global__ __launch_bounds__(256) void iaf_bwd_data_kernel(const MafW1 net, int nb, int nh, int D, int H, int B,
                                                           const float* __restrict__ z0, const float* __restrict__ ws,
                                                           const float* __restrict__ grows, const float* __restrict__ dz0,
                                                           const float* __restrict__ dladj, float* __restrict__ dx,
                                                           float* __restrict__ deltas) {
  extern __shared__ float lds[];
  float* g = lds;
  float* c = g + RT * D;
  float* dl = c + RT * 2 * D;
  float* gl = dl + nh * RT * H;
  int* deg = reinterpret_cast<int*>(gl + RT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * RT;
  const int nl = nh + 1;
  const long long CH = chunk_floats(B, D, H, nh);

  for (int k = tid; k < H; k += 256) deg[k] = k % (D - 1);
  // the gradient at the last block's y: z0 is that y flipped
  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, cc = i - r * D, b = b0 + r;
    float v = 0.f;
    if (b < B) {
      const long long at = (long long)b * D + (D - 1 - cc);
      if (grows) v = grows[b] * z0[at];
      if (dz0) v += dz0[at];
    }
    g[i] = v;
  }
  if (tid < RT) {
    const int b = b0 + tid;
    float v = 0.f;
    if (b < B) {
      if (grows) v = -grows[b];
      if (dladj) v += dladj[b];
    }
    gl[tid] = v;
  }
  __syncthreads();

  float4 acc;
  for (int blk = nb - 1; blk >= 0; --blk) {
    const int l0 = blk * nl;
    const float* wsx = ws + (long long)blk * CH;
    const float* wss = wsx + (long long)B * D;
    const float* whs = wsx + 2LL * B * D;
    for (int i = D - 1; i >= 0; --i) {
      if (i < D - 1) {  // no hidden unit has degree D - 1
        for (int l = nh - 1; l >= 0; --l) {
          const float* __restrict__ W = net.w[l0 + l + 1];
          const float* hl = whs + (long long)l * B * H;
          float* out = dl + l * RT * H;
          for (int o = i + wave * (D - 1); o < H; o += 4 * (D - 1)) {
            if (l == nh - 1)
              acc = wave_dot_col(W + o, H, c, 2 * D, 2 * D, lane, [=](int k) { return (k < D ? k : k - D) > i; });
            else
              acc = wave_dot_col(W + o, H, out + RT * H, H, H, lane, [=](int k) { return deg[k] >= i; });
            if (lane < RT) {
              const int b = b0 + lane;
              out[lane * H + o] = b < B && hl[(long long)b * H + o] > 0.f ? pick(acc, lane) : 0.f;
            }
          }
          __syncthreads();
        }
      }
      if (wave == 0) {
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < D - 1) acc = wave_dot_col(net.w[l0] + i, D, dl, H, H, lane, [=](int k) { return deg[k] >= i; });
        if (lane < RT) {
          const int b = b0 + lane;
          float s = 0.f, y = 0.f;
          if (b < B) {
            s = wss[(long long)b * D + i];
            y = wsx[(long long)b * D + i];
          }
          const float lam = expf(-s) * (g[lane * D + i] + pick(acc, lane));
          g[lane * D + i] = lam;
          c[lane * 2 * D + i] = -lam;
          c[lane * 2 * D + D + i] = -gl[lane] - lam * (y * expf(s));
        }
      }
      __syncthreads();
    }
    if (deltas) {
      float* dlx = deltas + (long long)blk * CH;
      for (int i = tid; i < RT * 2 * D; i += 256) {
        const int r = i / (2 * D), b = b0 + r;
        if (b < B) dlx[(long long)b * 2 * D + (i - r * 2 * D)] = c[i];
      }
      for (int l = 0; l < nh; ++l) {
        float* dh = dlx + 2LL * B * D + (long long)l * B * H;
        for (int i = tid; i < RT * H; i += 256) {
          const int r = i / H, b = b0 + r;
          if (b < B) dh[(long long)b * H + (i - r * H)] = dl[l * RT * H + i];
        }
      }
    }
    if (blk > 0) {  // the block's input is the previous block's y flipped; c is free once the deltas are out
      __syncthreads();
      for (int i = tid; i < RT * D; i += 256) {
        const int r = i / D, cc = i - r * D;
        c[r * D + (D - 1 - cc)] = g[i];
      }
      __syncthreads();
      for (int i = tid; i < RT * D; i += 256) g[i] = c[i];
      __syncthreads();
    }
  }
  if (dx)
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, cc = i - r * D, b = b0 + r;
      if (b < B) dx[(long long)b * D + cc] = g[i];
    }
}

// LDS: xs [RT,D] | bufA [RT,S] | bufB [RT,S] | lad [RT] | deg [H]   (S = max(H, 2D))
__global__ __launch_bounds__(256) void iaf_inverse_kernel(const MafWB1 net, const float* __restrict__ y, int nb, int nh, int D,
                                                          int H, int R, float* __restrict__ x, float* __restrict__ ladj) {
  extern __shared__ float lds[];
  const int S = H > 2 * D ? H : 2 * D;
  float* xs = lds;
  float* bufA = xs + RT * D;
  float* bufB = bufA + RT * S;
  float* lad = bufB + RT * S;
  int* deg = reinterpret_cast<int*>(lad + RT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * RT;
  const int nl = nh + 1;

  for (int i = tid; i < RT * D; i += 256) {  // flipped: the last block's input
    const int r = i / D, c = i - r * D, b = b0 + r;
    xs[r * D + (D - 1 - c)] = b < R ? y[(long long)b * D + c] : 0.f;
  }
  for (int k = tid; k < H; k += 256) deg[k] = k % (D - 1);
  if (tid < RT) lad[tid] = 0.f;
  __syncthreads();

  for (int blk = nb - 1; blk >= 0; --blk) {
    const int l0 = blk * nl;
    const float* in = xs;
    int ldi = D, K = D;
    float* out = bufA;
    for (int l = 0; l < nh; ++l) {
      made_layer(net.w[l0 + l], net.b[l0 + l], in, ldi, K, out, H, H, l == 0 ? 0 : 1, D, deg);
      __syncthreads();
      in = out;
      ldi = H;
      K = H;
      out = out == bufA ? bufB : bufA;
    }
    made_layer(net.w[l0 + nh], net.b[l0 + nh], in, ldi, K, out, 2 * D, 2 * D, 2, D, deg);
    __syncthreads();
    // y exp(s) + m into the buffer the last hidden layer no longer needs, flipped for the block that follows
    float* tmp = out == bufA ? bufB : bufA;
    for (int i = tid; i < RT * D; i += 256) {
      const int r = i / D, c = i - r * D;
      const float m = out[r * 2 * D + c], s = out[r * 2 * D + D + c];
      tmp[r * D + (blk > 0 ? D - 1 - c : c)] = xs[i] * expf(s) + m;
    }
    {  // wave r: ladj[r] += sum_d s[r,d]
      float s = 0.f;
      for (int c = lane; c < D; c += 64) s += out[wave * 2 * D + D + c];
      s = wave_sum_dpp(s);
      if (lane == 0) lad[wave] += s;
    }
    __syncthreads();
    for (int i = tid; i < RT * D; i += 256) xs[i] = tmp[i];
    __syncthreads();
  }

  for (int i = tid; i < RT * D; i += 256) {
    const int r = i / D, c = i - r * D, b = b0 + r;
    if (b < R) x[(long long)b * D + c] = xs[i];
  }
  if (ladj && tid < RT && b0 + tid < R) ladj[b0 + tid] = lad[tid];
}

bool shape_ok(int M, int nb, int nh, int D, int H) {
  return M >= 1 && M <= MAXM && nb >= 1 && nb <= MVK_MAF_MAX_BLOCKS && nh >= 1 && nh <= MVK_MAF_MAX_HIDDEN && D >= 2 &&
         D <= MVK_MAF_MAX_DIM && H >= 1 && H <= MVK_MAF_MAX_DIM;
}

}  // namespace

int mvk_maf_fwd(const float* z, const float* const* W, const float* const* b, int M, int n_blocks, int n_hidden, int D, int H,
                const float* const* mu0, const float* const* lv0, int B, float* z0, float* ladj, float* rows, float* ws,
                void* stream) {
  if (!z || !W || !b || !shape_ok(M, n_blocks, n_hidden, D, H) || B < 0 || !z0 || !ladj) return MVK_EINVAL;
  if ((mu0 == nullptr) != (lv0 == nullptr) || (mu0 != nullptr) != (rows != nullptr)) return MVK_EINVAL;
  const int nl = n_blocks * (n_hidden + 1);
  MafWB net{};
  MafPost post{};
  for (int m = 0; m < M; ++m) {
    for (int l = 0; l < nl; ++l) {
      if (!W[m * nl + l] || !b[m * nl + l]) return MVK_EINVAL;
      net.w[m * nl + l] = W[m * nl + l];
      net.b[m * nl + l] = b[m * nl + l];
    }
    if (mu0) {
      if (!mu0[m] || !lv0[m]) return MVK_EINVAL;
      post.mu[m] = mu0[m];
      post.lv[m] = lv0[m];
    }
  }
  if (B == 0) return MVK_OK;
  const int S = H > 2 * D ? H : 2 * D;
  const size_t lds = sizeof(float) * ((size_t)RT * D + 2 * (size_t)RT * S + RT + H);
  hipLaunchKernelGGL(maf_fwd_kernel, dim3((B + RT - 1) / RT, M), dim3(256), lds, mvk_stream(stream), net, post, mu0 ? 1 : 0, z,
                     n_blocks, n_hidden, D, H, B, z0, ladj, rows, ws);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_maf_bwd(const float* const* W, int M, int n_blocks, int n_hidden, int D, int H, const float* const* mu0,
                const float* const* lv0, const float* z0, const float* ws, const float* grows, const float* dz0,
                const float* dladj, int B, float* const* dmu0, float* const* dlv0, float* dz, float* deltas, float* const* dW,
                float* const* db, void* stream) {
  if (!W || !shape_ok(M, n_blocks, n_hidden, D, H) || B < 0 || !z0 || !ws) return MVK_EINVAL;
  if ((mu0 == nullptr) != (lv0 == nullptr) || (mu0 != nullptr) != (dmu0 != nullptr) || (mu0 != nullptr) != (dlv0 != nullptr))
    return MVK_EINVAL;
  if (grows && !mu0) return MVK_EINVAL;         // the row term is defined through the posteriors
  if (!grows && !dz0 && !dladj) return MVK_EINVAL;  // nothing to propagate
  if ((dW || db) && !deltas) return MVK_EINVAL;
  const int nl = n_blocks * (n_hidden + 1);
  MafW net{};
  MafPost post{};
  MafGPost gpost{};
  MafGW gw{};
  for (int m = 0; m < M; ++m) {
    for (int l = 0; l < nl; ++l) {
      if (!W[m * nl + l]) return MVK_EINVAL;
      net.w[m * nl + l] = W[m * nl + l];
      gw.w[m * nl + l] = dW ? dW[m * nl + l] : nullptr;  // a null entry: that layer's gradient is not wanted
      gw.b[m * nl + l] = db ? db[m * nl + l] : nullptr;
    }
    if (mu0) {
      if (!mu0[m] || !lv0[m] || !dmu0[m] || !dlv0[m]) return MVK_EINVAL;
      post.mu[m] = mu0[m];
      post.lv[m] = lv0[m];
      gpost.mu[m] = dmu0[m];
      gpost.lv[m] = dlv0[m];
    }
  }
  if (B == 0) return MVK_OK;
  const int S = H > 2 * D ? H : 2 * D;
  const size_t lds = sizeof(float) * (3 * (size_t)RT * D + 2 * (size_t)RT * S + RT + H);
  hipLaunchKernelGGL(maf_bwd_data_kernel, dim3((B + RT - 1) / RT, dz ? 1 : M), dim3(256), lds, mvk_stream(stream), net, post,
                     gpost, mu0 ? 1 : 0, M, n_blocks, n_hidden, D, H, B, z0, ws, grows, dz0, dladj, dz, deltas);
  MVK_CHECK_LAUNCH();
  if (dW || db) {
    const long long big = (long long)H * (H > 2 * D ? H : 2 * D);  // the largest layer: [H,D] <= [2D,H], [H,H]
    hipLaunchKernelGGL(maf_bwd_weight_kernel, dim3((unsigned)((big + 255) / 256), M * nl), dim3(256), 0, mvk_stream(stream), gw,
                       n_hidden, D, H, B, ws, deltas);
    MVK_CHECK_LAUNCH();
  }
  return MVK_OK;
}

int mvk_maf_inverse(const float* y, const float* const* W, const float* const* b, int n_blocks, int n_hidden, int D, int H, int R,
                    float* x, float* ladj, void* stream) {
  if (!y || !W || !b || !shape_ok(1, n_blocks, n_hidden, D, H) || R < 0 || !x) return MVK_EINVAL;
  const int nl = n_blocks * (n_hidden + 1);
  MafWB1 net{};
  for (int l = 0; l < nl; ++l) {
    if (!W[l] || !b[l]) return MVK_EINVAL;
    net.w[l] = W[l];
    net.b[l] = b[l];
  }
  if (R == 0) return MVK_OK;
  const size_t lds = sizeof(float) * (2 * (size_t)RT * D + (size_t)n_hidden * RT * H + RT + H);
  hipLaunchKernelGGL(maf_inverse_kernel, dim3((R + RT - 1) / RT), dim3(256), lds, mvk_stream(stream), net, y, n_blocks, n_hidden,
                     D, H, R, x, ladj);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_iaf_fwd(const float* x, const float* const* W, const float* const* b, int n_blocks, int n_hidden, int D, int H, int B,
                float* z0, float* ladj, float* rows, float* ws, void* stream) {
  if (!x || !W || !b || !shape_ok(1, n_blocks, n_hidden, D, H) || B < 0 || !z0 || !ladj) return MVK_EINVAL;
  const int nl = n_blocks * (n_hidden + 1);
  MafWB1 net{};
  for (int l = 0; l < nl; ++l) {
    if (!W[l] || !b[l]) return MVK_EINVAL;
    net.w[l] = W[l];
    net.b[l] = b[l];
  }
  if (B == 0) return MVK_OK;
  const size_t lds = sizeof(float) * (3 * (size_t)RT * D + (size_t)n_hidden * RT * H + RT + H);
  hipLaunchKernelGGL(iaf_fwd_kernel, dim3((B + RT - 1) / RT), dim3(256), lds, mvk_stream(stream), net, x, n_blocks, n_hidden, D, H,
                     B, z0, ladj, rows, ws);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_iaf_bwd(const float* const* W, int n_blocks, int n_hidden, int D, int H, const float* z0, const float* ws,
                const float* grows, const float* dz0, const float* dladj, int B, float* dx, float* deltas, float* const* dW,
                float* const* db, void* stream) {
  if (!W || !shape_ok(1, n_blocks, n_hidden, D, H) || B < 0 || !z0 || !ws) return MVK_EINVAL;
  if (!grows && !dz0 && !dladj) return MVK_EINVAL;  // nothing to propagate
  if ((dW || db) && !deltas) return MVK_EINVAL;
  const int nl = n_blocks * (n_hidden + 1);
  MafW1 net{};
  MafGW gw{};
  for (int l = 0; l < nl; ++l) {
    if (!W[l]) return MVK_EINVAL;
    net.w[l] = W[l];
    gw.w[l] = dW ? dW[l] : nullptr;  // a null entry: that layer's gradient is not wanted
    gw.b[l] = db ? db[l] : nullptr;
  }
  if (B == 0) return MVK_OK;
  const size_t lds = sizeof(float) * (3 * (size_t)RT * D + (size_t)n_hidden * RT * H + RT + H);
  hipLaunchKernelGGL(iaf_bwd_data_kernel, dim3((B + RT - 1) / RT), dim3(256), lds, mvk_stream(stream), net, n_blocks, n_hidden, D, H,
                     B, z0, ws, grows, dz0, dladj, dx, deltas);
  MVK_CHECK_LAUNCH();
  if (dW || db) {
    const long long big = (long long)H * (H > 2 * D ? H : 2 * D);
    hipLaunchKernelGGL(maf_bwd_weight_kernel, dim3((unsigned)((big + 255) / 256), nl), dim3(256), 0, mvk_stream(stream), gw,
                       n_hidden, D, H, B, ws, deltas);
    MVK_CHECK_LAUNCH();
  }
  return MVK_OK;
}

int mvk_iaf_inverse(const float* y, const float* const* W, const float* const* b, int n_blocks, int n_hidden, int D, int H, int R,
                    float* x, float* ladj, void* stream) {
  if (!y || !W || !b || !shape_ok(1, n_blocks, n_hidden, D, H) || R < 0 || !x) return MVK_EINVAL;
  const int nl = n_blocks * (n_hidden + 1);
  MafWB1 net{};
  for (int l = 0; l < nl; ++l) {
    if (!W[l] || !b[l]) return MVK_EINVAL;
    net.w[l] = W[l];
    net.b[l] = b[l];
  }
  if (R == 0) return MVK_OK;
  const int S = H > 2 * D ? H : 2 * D;
  const size_t lds = sizeof(float) * ((size_t)RT * D + 2 * (size_t)RT * S + RT + H);
  hipLaunchKernelGGL(iaf_inverse_kernel, dim3((R + RT - 1) / RT), dim3(256), lds, mvk_stream(stream), net, y, n_blocks, n_hidden,
                     D, H, R, x, ladj);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}
