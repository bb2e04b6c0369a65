// The PolyMNIST digit classifier (multivae/metrics/classifiers/mmnist.py) in eval mode, whole, in one launch, with what the
// coherence evaluator does with its logits: [n,3,28,28] -> conv 4x4/s2/p1 (10) + ReLU -> conv 4x4/s2/p1 (20) + ReLU -> flatten
// (c, h, w) -> 980 -> 128 + ReLU -> 10, then argmax and the per-class (correct, count) pairs of ClassCounts.update.
//
// Layout of the work (include/mvk.h, "PolyMNIST classifier")
//  * One workgroup of sixteen waves owns CL_T = 16 images and walks them in groups of CL_G = 4.  A group's images are staged in LDS
//    with a zero border (30 x 30 per channel: the padding costs no branch); the next group's pixels are loaded into registers
//    before the current group's arithmetic.  conv1: one thread per (image, output position), all 10 channels in registers.  conv2:
//    one thread per (image, output position, five of the 20 channels), the channel block being the same for a whole wave.  The
//    weights are wave-uniform reads of the parameters' own storage through the constant address space, i.e. scalar loads into
//    scalar registers, 40 at a time: every vector instruction of the two loops is an FMA or an LDS read of two pixels, and the
//    four waves of a SIMD cover one another's scalar-load latency.
//  * Only conv2's output outlives its stage: [16][980] floats in LDS (rows CL_HS apart).  fc1 is [16, 980] x [980, 128] on
//    v_mfma_f32_16x16x4_f32 (exact fp32): a wave owns one 16-column block and one half of K, a lane reads four consecutive k of
//    its image from LDS and of its weight row from global memory (the rows of the [128, 980] parameter: L2-resident, shared by
//    all workgroups; a chunk of steps is loaded one chunk ahead) and feeds them to four MFMAs, two accumulators taking the even
//    and the odd 16-k steps; the two K halves meet in LDS in a fixed order.  fc2, the argmax and the counts are a few threads'
//    work on LDS.
//  * Determinism: every logit is one fixed sequence of fp32 operations on its own image's row and the weights; an MFMA row
//    depends on its own A row only, a padded row (image >= n) is computed on zeros and never stored.  So the logits of an image
//    are the same bits in every run, for every n and every place in a tile.  The counts are integer atomics.
#include "common.hpp"

namespace {

constexpr int CL_T = 16;    // images per workgroup = the rows of the MFMA tile
constexpr int CL_G = 4;     // images per staged group
constexpr int CL_TPB = 1024;
constexpr int CL_XS = 3 * 30 * 30;   // a staged image with its border
constexpr int CL_H1 = 10 * 16 * 16;  // conv1's output [10][14][14] with its border
constexpr int CL_K = 980, CL_HS = 988;  // fc1's K; the row pitch of conv2's output (16-byte rows, banks 4 (7 i + q) mod 32)
constexpr int CL_H3S = 132;          // row pitch of fc1's output [16][128]
constexpr int CL_IMG = 3 * 28 * 28;
constexpr int CL_PRE = (CL_G * CL_IMG + CL_TPB - 1) / CL_TPB;  // pixels of a group per thread
constexpr int CL_LDS_FLOATS = CL_G * CL_XS + CL_G * CL_H1 + CL_T * CL_HS;
// after the last group the staging area holds fc1's two K halves, its output, the logits and the counts
static_assert(3 * CL_T * CL_H3S + CL_T * 10 + 22 <= CL_G * CL_XS, "the tail reuses the staging area");

typedef float cl_f32x4 __attribute__((ext_vector_type(4)));
typedef float cl_f32x2 __attribute__((ext_vector_type(2)));
// The convolution weights are read at wave-uniform addresses and nothing writes them during the launch: through the constant
// address space they are scalar loads into scalar registers, not one vector load per lane.
typedef const float __attribute__((address_space(4))) * cl_cptr;
__device__ __forceinline__ cl_cptr cl_const(const float* p) { return reinterpret_cast<cl_cptr>(reinterpret_cast<uintptr_t>(p)); }
// The same pointer, opaque to the optimiser: the loads behind it stay in the loop they are written in (hoisted out of the group
// loop, the 480 + 3200 weights do not fit the scalar registers and are spilled to vector lanes).
__device__ __forceinline__ cl_cptr cl_here(cl_cptr p) {
  asm volatile("" : "+s"(p));
  return p;
}

struct ClfArgs {
  const float *x, *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
  long long n;
  float* logits;
  int* pred;
  const long long* labels;
  long long label_rows;
  unsigned long long* counts;
  int w3vec;  // w3 is 16-byte aligned: its rows are read four k at a time
};

__global__ __launch_bounds__(CL_TPB) void polyclf_kernel(const ClfArgs g) {
  extern __shared__ __attribute__((aligned(16))) float cl_lds[];
  float* xs = cl_lds;                 // [CL_G][3][30][30]
  float* h1 = xs + CL_G * CL_XS;      // [CL_G][10][16][16]
  float* h2 = h1 + CL_G * CL_H1;      // [CL_T][CL_HS]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long i0 = (long long)blockIdx.x * CL_T;
  const cl_cptr w1 = cl_const(g.w1), b1 = cl_const(g.b1), w2 = cl_const(g.w2), b2 = cl_const(g.b2);

  // the borders of both staged maps are zero for the whole launch: only interiors are written below
  for (int e = tid; e < CL_G * CL_XS + CL_G * CL_H1; e += CL_TPB) cl_lds[e] = 0.f;

  float pre[CL_PRE];
  auto load_group = [&](int grp) {  // pixels of images i0 + 4 grp .. + 3, zeros for an image >= n
    const long long base = i0 + (long long)grp * CL_G;
#pragma unroll
    for (int u = 0; u < CL_PRE; ++u) {
      const int e = tid + u * CL_TPB;
      const bool ok = e < CL_G * CL_IMG && base + e / CL_IMG < g.n;
      pre[u] = ok ? g.x[base * CL_IMG + e] : 0.f;
    }
  };
  load_group(0);
#pragma unroll 1
  for (int grp = 0; grp < CL_T / CL_G; ++grp) {
    __syncthreads();  // the zero fill; the previous group's readers of xs and h1
#pragma unroll
    for (int u = 0; u < CL_PRE; ++u) {
      const int e = tid + u * CL_TPB;
      if (e < CL_G * CL_IMG) {
        const int gi = e / CL_IMG, r = e % CL_IMG, c = r / 784, y = (r % 784) / 28, xx = r % 28;
        xs[gi * CL_XS + c * 900 + (y + 1) * 30 + xx + 1] = pre[u];
      }
    }
    __syncthreads();
    if (grp + 1 < CL_T / CL_G) load_group(grp + 1);

    // conv1 + bias + ReLU: input row 2 oy - 1 + ky is staged row 2 oy + ky.  k runs (c, ky, kx) for every channel.
    if (tid < CL_G * 196) {
      const int gi = tid / 196, p = tid % 196, oy = p / 14, ox = p % 14;
      const float* src = xs + gi * CL_XS + (2 * oy) * 30 + 2 * ox;
      float acc[10];
#pragma unroll
      for (int co = 0; co < 10; ++co) acc[co] = b1[co];
#pragma unroll 1
      for (int cky = 0; cky < 12; ++cky) {  // (c, ky)
        const int c = cky >> 2, ky = cky & 3;
        const cl_f32x2 lo = *reinterpret_cast<const cl_f32x2*>(src + c * 900 + ky * 30);
        const cl_f32x2 hi = *reinterpret_cast<const cl_f32x2*>(src + c * 900 + ky * 30 + 2);
        const float v[4] = {lo[0], lo[1], hi[0], hi[1]};
        const cl_cptr w = cl_here(w1 + cky * 4);
#pragma unroll
        for (int co = 0; co < 10; ++co) {
#pragma unroll
          for (int kx = 0; kx < 4; ++kx) acc[co] = fmaf(v[kx], w[co * 48 + kx], acc[co]);
        }
      }
      float* dst = h1 + gi * CL_H1 + (oy + 1) * 16 + ox + 1;
#pragma unroll
      for (int co = 0; co < 10; ++co) dst[co * 256] = fmaxf(acc[co], 0.f);
    }
    __syncthreads();

    // conv2 + bias + ReLU, written flattened in (c, h, w) order; waves 4 q .. 4 q + 3 compute channels 5 q .. 5 q + 4
    {
      const int q = wave >> 2, it = tid & 255;
      if (it < CL_G * 49) {
        const int gi = it / 49, p = it % 49, oy = p / 7, ox = p % 7;
        const float* src = h1 + gi * CL_H1 + (2 * oy) * 16 + 2 * ox;
        const cl_cptr wq = w2 + q * 5 * 160;
        float acc[5];
#pragma unroll
        for (int co = 0; co < 5; ++co) acc[co] = b2[q * 5 + co];
#pragma unroll 1
        for (int ch = 0; ch < 20; ++ch) {  // (c, two ky)
          const int c = ch >> 1, ky0 = (ch & 1) * 2;
          const cl_cptr w = cl_here(wq + ch * 8);
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const cl_f32x2 lo = *reinterpret_cast<const cl_f32x2*>(src + c * 256 + (ky0 + kk) * 16);
            const cl_f32x2 hi = *reinterpret_cast<const cl_f32x2*>(src + c * 256 + (ky0 + kk) * 16 + 2);
            const float v[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int co = 0; co < 5; ++co) {
#pragma unroll
              for (int kx = 0; kx < 4; ++kx) acc[co] = fmaf(v[kx], w[co * 160 + kk * 4 + kx], acc[co]);
            }
          }
        }
        float* dst = h2 + (grp * CL_G + gi) * CL_HS + q * 5 * 49 + p;
#pragma unroll
        for (int co = 0; co < 5; ++co) dst[co * 49] = fmaxf(acc[co], 0.f);
      }
    }
  }
  __syncthreads();

  // fc1.  A[i = image l15][k], B[k][j = output l15]; slot lq of MFMA u of step s is k = 16 s + 4 lq + u.  Wave w: the 16 outputs
  // of block w & 7; waves 0-7 take steps 0-30, waves 8-15 steps 31-60 and the last four k.
  float* part = xs;                              // [2][CL_T][CL_H3S]
  float* h3 = part + 2 * CL_T * CL_H3S;          // [CL_T][CL_H3S]
  float* lg = h3 + CL_T * CL_H3S;                // [CL_T][10]
  int* cnt = reinterpret_cast<int*>(lg + CL_T * 10);  // [11][2]
  {
    const int l15 = lane & 15, lq = lane >> 4, blk = wave & 7, kh = wave >> 3;
    constexpr int STEPS = CL_K / 16;  // 61 whole steps, then 4 k
    constexpr int CH = 8;             // steps per chunk: a chunk's weights are loaded one chunk ahead
    const int s0 = kh ? 31 : 0, s1 = kh ? STEPS : 31;
    const float* arow = h2 + l15 * CL_HS + 4 * lq;
    const float* __restrict__ wrow = g.w3 + (long long)(blk * 16 + l15) * CL_K + 4 * lq;
    cl_f32x4 acc[2] = {cl_f32x4{0.f, 0.f, 0.f, 0.f}, cl_f32x4{0.f, 0.f, 0.f, 0.f}};
    cl_f32x4 cur[CH], nxt[CH];
    auto load_chunk = [&](cl_f32x4 (&dst)[CH], int sb) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const float* p = wrow + 16 * (sb + i);
        if (sb + i >= s1)
          dst[i] = cl_f32x4{0.f, 0.f, 0.f, 0.f};
        else if (g.w3vec)
          dst[i] = *reinterpret_cast<const cl_f32x4*>(p);
        else
          dst[i] = cl_f32x4{p[0], p[1], p[2], p[3]};
      }
    };
    load_chunk(cur, s0);
#pragma unroll 1
    for (int sb = s0; sb < s1; sb += CH) {
      if (sb + CH < s1) load_chunk(nxt, sb + CH);
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        if (sb + i < s1) {  // wave-uniform
          const cl_f32x4 a = *reinterpret_cast<const cl_f32x4*>(arow + 16 * (sb + i));
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[i & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], cur[i][u], acc[i & 1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < CH; ++i) cur[i] = nxt[i];
    }
    if (kh) {  // k = 976 + lq
      const int kt = 16 * STEPS + lq;
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(h2[l15 * CL_HS + kt], g.w3[(long long)(blk * 16 + l15) * CL_K + kt], acc[0], 0, 0, 0);
    }
    // D[i = 4 lq + r][j = l15]; the staging area is free since the last group's conv1
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(kh * CL_T + 4 * lq + r) * CL_H3S + blk * 16 + l15] = acc[0][r] + acc[1][r];
    if (tid < 22) cnt[tid] = 0;
  }
  __syncthreads();
  for (int e = tid; e < CL_T * 128; e += CL_TPB) {  // + bias + ReLU
    const int img = e >> 7, o = e & 127;
    h3[img * CL_H3S + o] = fmaxf((part[img * CL_H3S + o] + part[(CL_T + img) * CL_H3S + o]) + g.b3[o], 0.f);
  }
  __syncthreads();

  // fc2 + bias: one thread per (image, class), k in order
  if (tid < CL_T * 10) {
    const int img = tid / 10, o = tid % 10;
    const float* __restrict__ w4 = g.w4 + o * 128;
    const float* a = h3 + img * CL_H3S;
    float acc = g.b4[o];
#pragma unroll 8
    for (int k = 0; k < 128; ++k) acc = fmaf(a[k], w4[k], acc);
    lg[tid] = acc;
    if (g.logits && i0 + img < g.n) g.logits[(i0 + img) * 10 + o] = acc;
  }
  if (!g.pred && !g.counts) return;
  __syncthreads();
  if (tid < CL_T && i0 + tid < g.n) {
    // torch.argmax: the first maximum, a NaN counting as the maximum
    float best = lg[tid * 10];
    int bi = 0;
#pragma unroll
    for (int j = 1; j < 10; ++j) {
      const float v = lg[tid * 10 + j];
      if (best == best && (v != v || v > best)) {
        best = v;
        bi = j;
      }
    }
    if (g.pred) g.pred[i0 + tid] = bi;
    if (g.counts) {
      const long long lab = g.labels[(i0 + tid) % g.label_rows];
      const int r = (lab >= 0 && lab < 10) ? (int)lab : 10;
      if (lab == bi) atomicAdd(&cnt[2 * r], 1);
      atomicAdd(&cnt[2 * r + 1], 1);
    }
  }
  if (!g.counts) return;
  __syncthreads();
  if (tid < 22 && cnt[tid] != 0) atomicAdd(&g.counts[tid], (unsigned long long)cnt[tid]);
}

}  // namespace

extern "C" {

int mvk_polyclf_tile(void) { return CL_T; }

int mvk_polyclf_fwd(const float* x, int64_t n, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                    const float* b3, const float* w4, const float* b4, float* logits, int32_t* pred, const int64_t* labels,
                    int64_t label_rows, int64_t* counts, void* stream) {
  if (n < 0 || (!logits && !pred && !counts)) return MVK_EINVAL;
  if (counts && (!labels || label_rows <= 0 || n % label_rows != 0)) return MVK_EINVAL;
  if (n == 0) return MVK_OK;
  if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) return MVK_EINVAL;
  const long long tiles = ((long long)n + CL_T - 1) / CL_T;
  if (tiles > 0x7fffffffLL) return MVK_EINVAL;
  constexpr int lds = CL_LDS_FLOATS * (int)sizeof(float);
  static_assert(lds <= 160 * 1024, "one workgroup's LDS");
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(polyclf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  ClfArgs g;
  g.x = x, g.w1 = w1, g.b1 = b1, g.w2 = w2, g.b2 = b2, g.w3 = w3, g.b3 = b3, g.w4 = w4, g.b4 = b4;
  g.n = n, g.logits = logits, g.pred = pred;
  g.labels = reinterpret_cast<const long long*>(labels), g.label_rows = label_rows;
  g.counts = reinterpret_cast<unsigned long long*>(counts);
  g.w3vec = mvk_aligned16(w3) ? 1 : 0;
  hipLaunchKernelGGL(polyclf_kernel, dim3((unsigned)tiles), dim3(CL_TPB), lds, mvk_stream(stream), g);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
