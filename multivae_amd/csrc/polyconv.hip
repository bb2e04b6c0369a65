// 3x3 / stride 2 / pad 1 convolution and its transpose on the odd map chain of the PolyMNIST convolutional networks
// (multivae/models/nn/mmnist.py:36-206: 28 -> 14 -> 7 -> 4 and back with output_padding 0 or 1), exact fp32 on
// v_mfma_f32_16x16x4_f32, reading the reference weight layout W[Cv][Cu][3][3] of Conv2d(Cu, Cv) == ConvTranspose2d(Cv, Cu).
//
// Layout of the work (include/mvk.h, "PolyMNIST convolutional networks")
//  * pc_layer is the layer arithmetic, written once: it walks wave tasks (PC_MT tiles of 16 output positions x one block of 16
//    output channels) over a range of images whose source and destination are plain pointers, global memory or LDS alike.  The
//    layer kernels call it on the whole batch; the fused trunks (polyenc_kernel / polydec_kernel) call it three times on a tile
//    of PC_T images whose two intermediate maps live in LDS.
//  * down (Conv2d forward, ConvTranspose2d backward-data): rows are output positions (img, oy, ox), k runs (16 channels, tap,
//    4 channels); a lane reads the 36 consecutive weights W[cv][16 s + 4 lq .. + 3][3][3] of its output channel per 16-channel
//    step and four consecutive channels of its position's source pixel per tap.
//  * up (ConvTranspose2d forward, Conv2d backward-data): output positions are walked one parity class (Y mod 2, X mod 2) at a
//    time; a class has 1, 2, 2 or 4 taps, the same for all of its positions, so no MFMA is spent on a tap that cannot reach an
//    output.  A window that overhangs the small map (output_padding) reads zeros.
//  * wgrad: dW[cv][cu][tap] = sum over small positions of U(gathered)[cu] V[cv]: a wave owns a 16 x 16 (cu, cv) block for all
//    nine taps and one slice of the positions; the slices' slabs are added by a finish kernel in a fixed order.  The bias
//    gradient (the sums of V's channels, or of U's) rides along in the same slabs.
//  * Determinism: every output entry is one fixed sequence of fp32 operations on its own image's pixels; an MFMA row depends on
//    its own A row only, a tap outside the map contributes products with zero, a padded row is computed on zeros and never
//    stored.  So an image's result is the same bits for every n and every place in a tile, in the layer kernels and in the
//    fused trunks alike.  No floating-point atomics.
#include "common.hpp"

namespace {

typedef float pc_f4 __attribute__((ext_vector_type(4)));

constexpr int PC_MT = 2;      // 16-row position tiles per wave task
constexpr int PC_T = 4;       // images per workgroup of a fused trunk
constexpr int PC_TPB = 1024;  // threads of a fused trunk's workgroup
constexpr int PC_H1 = 14 * 14 * 32, PC_H2 = 7 * 7 * 64, PC_H3 = 4 * 4 * 128, PC_IMG = 3 * 28 * 28;
constexpr int PC_LDS_FLOATS = PC_T * (PC_H1 + PC_H2);

__device__ __forceinline__ pc_f4 pc_mfma(float a, float b, pc_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// One layer over images [0, nimg) of src / dst.  U is the big map [img][H][W][CU] (u_nchw: [img][CU][H][W]), V the small one
// [img][h][wd][CV].  UP = false: V = act(conv(U) + bias); UP = true: U = act(convT(V) + bias).  Then * mact'(msrc) with msrc
// laid out like the destination.  Source images >= nsrc read as zeros, destination images >= ndst are not stored.  Tasks
// task0, task0 + tstride, ... are this wave's.  wvec: w is 16-byte aligned.
template <int CU, int CV, bool UP>
__device__ __forceinline__ void pc_layer(const float* src, float* dst, const float* __restrict__ w, const float* __restrict__ bias,
                                         const float* msrc, int act, int mact, int H, int W, int h, int wd, int nimg, int nsrc,
                                         int ndst, int u_nchw, int wvec, int task0, int tstride, int lane) {
  const int l15 = lane & 15, lq = lane >> 4;
  if constexpr (!UP) {
    constexpr int NB = CV / 16;
    const int hw = h * wd, rows = nimg * hw;
    const int groups = (rows + 16 * PC_MT - 1) / (16 * PC_MT);
#pragma unroll 1
    for (int task = task0; task < groups * NB; task += tstride) {
      const int jb = task % NB, grp = task / NB, cv = jb * 16 + l15;
      int aimg[PC_MT], ay[PC_MT], ax[PC_MT];
      bool aok[PC_MT];
      pc_f4 acc[PC_MT];
#pragma unroll
      for (int m = 0; m < PC_MT; ++m) {
        const int r = (grp * PC_MT + m) * 16 + l15;
        aimg[m] = r / hw;
        const int p = r - aimg[m] * hw;
        ay[m] = p / wd, ax[m] = p - ay[m] * wd;
        aok[m] = r < rows && aimg[m] < nsrc;
        acc[m] = pc_f4{0.f, 0.f, 0.f, 0.f};
      }
      if constexpr (CU % 16 == 0) {
        const float* __restrict__ wl = w + (long long)cv * 9 * CU + 36 * lq;
#pragma unroll 1
        for (int s = 0; s < CU / 16; ++s) {
          float wr[36];  // [u][tap] of channels 16 s + 4 lq + u
          if (wvec) {
#pragma unroll
            for (int q = 0; q < 9; ++q) {
              const pc_f4 v = *reinterpret_cast<const pc_f4*>(wl + s * 144 + 4 * q);
              wr[4 * q] = v[0], wr[4 * q + 1] = v[1], wr[4 * q + 2] = v[2], wr[4 * q + 3] = v[3];
            }
          } else {
#pragma unroll
            for (int q = 0; q < 36; ++q) wr[q] = wl[s * 144 + q];
          }
#pragma unroll
          for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int m = 0; m < PC_MT; ++m) {
              const int Y = 2 * ay[m] - 1 + t / 3, X = 2 * ax[m] - 1 + t % 3;
              const bool ok = aok[m] && Y >= 0 && Y < H && X >= 0 && X < W;
              pc_f4 a = pc_f4{0.f, 0.f, 0.f, 0.f};
              if (ok) a = *reinterpret_cast<const pc_f4*>(src + (long long)aimg[m] * (H * W * CU) + ((Y * W + X) * CU + 16 * s + 4 * lq));
#pragma unroll
              for (int u = 0; u < 4; ++u) acc[m] = pc_mfma(a[u], wr[u * 9 + t], acc[m]);
            }
          }
        }
      } else {  // CU == 3: k = cu * 9 + tap, 27 of 28 slots
        static_assert(CU == 3, "the image layer");
#pragma unroll 1
        for (int s = 0; s < 7; ++s) {
          const int kk = 4 * s + lq, cu = kk / 9, t = kk - cu * 9;
          const bool kok = kk < 27;
          const float b = kok ? w[cv * 27 + kk] : 0.f;
#pragma unroll
          for (int m = 0; m < PC_MT; ++m) {
            const int Y = 2 * ay[m] - 1 + t / 3, X = 2 * ax[m] - 1 + t % 3;
            const bool ok = kok && aok[m] && Y >= 0 && Y < H && X >= 0 && X < W;
            float a = 0.f;
            if (ok) a = src[(long long)aimg[m] * (H * W * 3) + (u_nchw ? (cu * H + Y) * W + X : (Y * W + X) * 3 + cu)];
            acc[m] = pc_mfma(a, b, acc[m]);
          }
        }
      }
      // D[row 4 lq + rr][cv]; rows are (img, oy, ox) in order: V's own row index
      const float bv = bias ? bias[cv] : 0.f;
#pragma unroll
      for (int m = 0; m < PC_MT; ++m) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int r = (grp * PC_MT + m) * 16 + 4 * lq + rr;
          if (r < rows && r / hw < ndst) {
            const long long o = (long long)r * CV + cv;
            float v = mvk_act(acc[m][rr] + bv, act);
            if (msrc) v *= mvk_act_grad_from_out(msrc[o], mact);
            dst[o] = v;
          }
        }
      }
    }
  } else {
    constexpr int NB = (CU + 15) / 16;
    int task = task0, base = 0;
#pragma unroll 1
    for (int cls = 0; cls < 4; ++cls) {
      const int py = cls >> 1, px = cls & 1;
      const int ha = (H + 1 - py) / 2, wb = (W + 1 - px) / 2, cw = ha * wb;
      const int rows = nimg * cw;
      const int groups = (rows + 16 * PC_MT - 1) / (16 * PC_MT);
      const int nky = py ? 2 : 1, nkx = px ? 2 : 1;
#pragma unroll 1
      for (; task < base + groups * NB; task += tstride) {
        const int local = task - base, jb = local % NB, grp = local / NB, cu = jb * 16 + l15;
        const bool cok = cu < CU;
        int aimg[PC_MT], aa[PC_MT], ab[PC_MT];
        bool aok[PC_MT];
        pc_f4 acc[PC_MT];
#pragma unroll
        for (int m = 0; m < PC_MT; ++m) {
          const int r = (grp * PC_MT + m) * 16 + l15;
          aimg[m] = r / cw;
          const int p = r - aimg[m] * cw;
          aa[m] = p / wb, ab[m] = p - aa[m] * wb;
          aok[m] = r < rows && aimg[m] < nsrc;
          acc[m] = pc_f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll 1
        for (int s = 0; s < CV / 16; ++s) {
          const float* __restrict__ wl = w + ((long long)(16 * s + 4 * lq) * CU + cu) * 9;
#pragma unroll 1
          for (int iy = 0; iy < nky; ++iy) {
            // Y = 2 a + py = 2 sy - 1 + ky: an even Y takes ky = 1 from sy = a, an odd one ky = 0 from a + 1 and ky = 2 from a
            const int ky = py ? 2 * iy : 1, dy = (py && iy == 0) ? 1 : 0;
#pragma unroll 1
            for (int ix = 0; ix < nkx; ++ix) {
              const int kx = px ? 2 * ix : 1, dx = (px && ix == 0) ? 1 : 0, t = ky * 3 + kx;
              float b[4];
#pragma unroll
              for (int u = 0; u < 4; ++u) b[u] = cok ? wl[u * CU * 9 + t] : 0.f;
#pragma unroll
              for (int m = 0; m < PC_MT; ++m) {
                const int sy = aa[m] + dy, sx = ab[m] + dx;
                const bool ok = aok[m] && sy < h && sx < wd;
                pc_f4 a = pc_f4{0.f, 0.f, 0.f, 0.f};
                if (ok) a = *reinterpret_cast<const pc_f4*>(src + (long long)aimg[m] * (h * wd * CV) + ((sy * wd + sx) * CV + 16 * s + 4 * lq));
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m] = pc_mfma(a[u], b[u], acc[m]);
              }
            }
          }
        }
        const float bv = (bias && cok) ? bias[cu] : 0.f;
#pragma unroll
        for (int m = 0; m < PC_MT; ++m) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int r = (grp * PC_MT + m) * 16 + 4 * lq + rr;
            const int img = r / cw, p = r - img * cw, a = p / wb, bq = p - a * wb;
            if (cok && r < rows && img < ndst) {
              const int Y = 2 * a + py, X = 2 * bq + px;
              const long long o = (long long)img * (H * W * CU) + (u_nchw ? (cu * H + Y) * W + X : (Y * W + X) * CU + cu);
              float v = mvk_act(acc[m][rr] + bv, act);
              if (msrc) v *= mvk_act_grad_from_out(msrc[o], mact);
              dst[o] = v;
            }
          }
        }
      }
      base += groups * NB;
    }
  }
}

struct PcArgs {
  const float *src, *w, *bias, *msrc;
  float* dst;
  int act, mact, H, W, h, wd, n, u_nchw, wvec;
};

template <int CU, int CV, bool UP>
__global__ __launch_bounds__(256) void pc_layer_kernel(const PcArgs g) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  pc_layer<CU, CV, UP>(g.src, g.dst, g.w, g.bias, g.msrc, g.act, g.mact, g.H, g.W, g.h, g.wd, g.n, g.n, g.n, g.u_nchw, g.wvec,
                       blockIdx.x * 4 + wave, gridDim.x * 4, lane);
}

struct PcNetArgs {
  const float *x, *w0, *b0, *w1, *b1, *w2, *b2;
  float* out;
  long long n;
  int wvec0, wvec1, wvec2;
};

// image [n, 3, 28, 28] -> h3 [n, 4, 4, 128]; h1 and h2 of the workgroup's PC_T images stay in LDS
__global__ __launch_bounds__(PC_TPB) void polyenc_kernel(const PcNetArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pc_lds[];
  float* h1 = pc_lds;
  float* h2 = h1 + PC_T * PC_H1;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long i0 = (long long)blockIdx.x * PC_T;
  const int nv = g.n - i0 < PC_T ? (int)(g.n - i0) : PC_T;
  pc_layer<3, 32, false>(g.x + i0 * PC_IMG, h1, g.w0, g.b0, nullptr, MVK_ACT_RELU, MVK_ACT_NONE, 28, 28, 14, 14, PC_T, nv, PC_T, 1,
                         g.wvec0, wave, PC_TPB / 64, lane);
  __syncthreads();
  pc_layer<32, 64, false>(h1, h2, g.w1, g.b1, nullptr, MVK_ACT_RELU, MVK_ACT_NONE, 14, 14, 7, 7, PC_T, PC_T, PC_T, 0, g.wvec1, wave,
                          PC_TPB / 64, lane);
  __syncthreads();
  pc_layer<64, 128, false>(h2, g.out + i0 * PC_H3, g.w2, g.b2, nullptr, MVK_ACT_RELU, MVK_ACT_NONE, 7, 7, 4, 4, PC_T, PC_T, nv, 0,
                           g.wvec2, wave, PC_TPB / 64, lane);
}

// h0 [n, 4, 4, 128] -> image [n, 3, 28, 28]; the 7x7x64 and 14x14x32 maps stay in LDS
__global__ __launch_bounds__(PC_TPB) void polydec_kernel(const PcNetArgs g) {
  extern __shared__ __attribute__((aligned(16))) float pc_lds[];
  float* d2 = pc_lds;
  float* d1 = d2 + PC_T * PC_H1;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long i0 = (long long)blockIdx.x * PC_T;
  const int nv = g.n - i0 < PC_T ? (int)(g.n - i0) : PC_T;
  pc_layer<64, 128, true>(g.x + i0 * PC_H3, d1, g.w0, g.b0, nullptr, MVK_ACT_RELU, MVK_ACT_NONE, 7, 7, 4, 4, PC_T, nv, PC_T, 0, 0, wave,
                          PC_TPB / 64, lane);
  __syncthreads();
  pc_layer<32, 64, true>(d1, d2, g.w1, g.b1, nullptr, MVK_ACT_RELU, MVK_ACT_NONE, 14, 14, 7, 7, PC_T, PC_T, PC_T, 0, 0, wave, PC_TPB / 64,
                         lane);
  __syncthreads();
  pc_layer<3, 32, true>(d2, g.out + i0 * PC_IMG, g.w2, g.b2, nullptr, MVK_ACT_NONE, MVK_ACT_NONE, 28, 28, 14, 14, PC_T, PC_T, nv, 1, 0,
                        wave, PC_TPB / 64, lane);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------
struct PcWgArgs {
  const float *U, *V;
  float* slabs;  // [Z][9 CU CV + 128]
  int n, H, W, h, wd, u_nchw, Z, chunk, db_side;  // db_side 0: none, 1: sums of V's channels, 2: sums of U's channels
};

// A[i = cu][k = position] per tap, B[k = position][j = cv].  A wave: block (cub, cvb), slice z of the positions.
template <int CU, int CV>
__global__ __launch_bounds__(256) void pc_wgrad_kernel(const PcWgArgs g) {
  constexpr int NBU = (CU + 15) / 16, NBV = CV / 16, SLAB = 9 * CU * CV + 128;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int task = blockIdx.x * 4 + wave;
  if (task >= NBU * NBV * g.Z) return;
  const int cvb = task % NBV, cub = (task / NBV) % NBU, z = task / (NBV * NBU);
  const int cu = cub * 16 + l15, cv = cvb * 16 + l15;
  const bool cuok = cu < CU;
  const int hw = g.h * g.wd, rows = g.n * hw, H = g.H, W = g.W;
  const int p0 = z * g.chunk, p1 = min(rows, p0 + g.chunk);
  const float* __restrict__ U = g.U;
  const float* __restrict__ V = g.V;
  pc_f4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = pc_f4{0.f, 0.f, 0.f, 0.f};
  float dbs = 0.f;
#pragma unroll 1
  for (int pb = p0; pb < p1; pb += 4) {
    const int p = pb + lq;
    const bool ok = p < p1;
    const int img = p / hw, q = p - img * hw, oy = q / g.wd, ox = q - oy * g.wd;
    const float b = ok ? V[(long long)p * CV + cv] : 0.f;
    const long long ub = (long long)img * (H * W * CU);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int Y = 2 * oy - 1 + t / 3, X = 2 * ox - 1 + t % 3;
      float a = 0.f;
      if (ok && cuok && Y >= 0 && Y < H && X >= 0 && X < W) a = U[ub + (g.u_nchw ? (cu * H + Y) * W + X : (Y * W + X) * CU + cu)];
      acc[t] = pc_mfma(a, b, acc[t]);
    }
    if (g.db_side == 1) {
      dbs += b;
    } else if (g.db_side == 2 && cvb == 0 && ok && cuok) {  // every big pixel belongs to the small position (Y / 2, X / 2)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int Y = 2 * oy + (d >> 1), X = 2 * ox + (d & 1);
        if (Y < H && X < W) dbs += U[ub + (g.u_nchw ? (cu * H + Y) * W + X : (Y * W + X) * CU + cu)];
      }
    }
  }
  float* slab = g.slabs + (long long)z * SLAB;
  // D[cu = cub 16 + 4 lq + rr][cv]
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int c = cub * 16 + 4 * lq + rr;
      if (c < CU) slab[(cv * CU + c) * 9 + t] = acc[t][rr];
    }
  }
  if (g.db_side) {  // the four position streams of a channel, in order
    const float s0 = __shfl(dbs, l15, 64), s1 = __shfl(dbs, l15 + 16, 64), s2 = __shfl(dbs, l15 + 32, 64), s3 = __shfl(dbs, l15 + 48, 64);
    const float s = (s0 + s1) + (s2 + s3);
    if (g.db_side == 1 && cub == 0 && lq == 0) slab[9 * CU * CV + cv] = s;
    if (g.db_side == 2 && cvb == 0 && lq == 0 && cuok) slab[9 * CU * CV + cu] = s;
  }
}

// out[e] (+)= sum over slices; e < count: the weights, then the ndb bias entries behind them in a slab.  A workgroup owns 32
// entries; eight threads per entry add one contiguous eighth of the slices each, in slice order, and the eight partial sums are
// added in order: the order depends on Z alone.
constexpr int PC_FIN_E = 32, PC_FIN_G = 8;
__global__ __launch_bounds__(PC_FIN_E * PC_FIN_G) void pc_wgrad_finish_kernel(const float* __restrict__ slabs, int Z, int slab, int count,
                                                                          int ndb, float* dW, float* db, int accumulate) {
  __shared__ float part[PC_FIN_G][PC_FIN_E];
  const int le = threadIdx.x % PC_FIN_E, zg = threadIdx.x / PC_FIN_E;
  const int e = blockIdx.x * PC_FIN_E + le;
  const bool ok = e < count + ndb;
  const int per = (Z + PC_FIN_G - 1) / PC_FIN_G, z0 = zg * per, z1 = min(Z, z0 + per);
  float s = 0.f;
  if (ok)
    for (int z = z0; z < z1; ++z) s += slabs[(long long)z * slab + e];
  part[zg][le] = s;
  __syncthreads();
  if (zg != 0 || !ok) return;
  float t = part[0][le];
#pragma unroll
  for (int q = 1; q < PC_FIN_G; ++q) t += part[q][le];
  float* o = e < count ? dW + e : db + (e - count);
  *o = accumulate ? *o + t : t;
}

int pc_shape(int Cu, int Cv) { return (Cu == 3 && Cv == 32) ? 0 : (Cu == 32 && Cv == 64) ? 1 : (Cu == 64 && Cv == 128) ? 2 : -1; }

template <bool UP>
int pc_launch_layer(const float* src, const float* Wref, const float* bias, float* dst, int n, int H, int W, int Cu, int Cv, int act,
                    int u_nchw, const float* msrc, int mact, void* stream) {
  if (!mvk_conv3s2_ok(H, W, Cu, Cv) || n < 0) return MVK_EINVAL;
  if (n == 0) return MVK_OK;
  if (!src || !Wref || !dst) return MVK_EINVAL;
  if (u_nchw && Cu != 3) return MVK_EINVAL;
  const int h = (H + 1) / 2, wd = (W + 1) / 2;
  if ((long long)n * H * W > 0x7fffffffLL / 4) return MVK_EINVAL;
  // the NHWC operand with 16-channel steps is read four channels at a time
  if ((UP || Cu != 3) && !mvk_aligned16(src)) return MVK_EINVAL;
  PcArgs g;
  g.src = src, g.w = Wref, g.bias = bias, g.msrc = msrc, g.dst = dst;
  g.act = act, g.mact = mact, g.H = H, g.W = W, g.h = h, g.wd = wd, g.n = n, g.u_nchw = u_nchw, g.wvec = mvk_aligned16(Wref) ? 1 : 0;
  long long tasks;
  if (UP) {
    tasks = 0;
    for (int cls = 0; cls < 4; ++cls) {
      const long long rows = (long long)n * ((H + 1 - (cls >> 1)) / 2) * ((W + 1 - (cls & 1)) / 2);
      tasks += (rows + 16 * PC_MT - 1) / (16 * PC_MT) * ((Cu + 15) / 16);
    }
  } else {
    tasks = ((long long)n * h * wd + 16 * PC_MT - 1) / (16 * PC_MT) * (Cv / 16);
  }
  long long blocks = (tasks + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks), tpb(256);
  hipStream_t s = mvk_stream(stream);
  switch (pc_shape(Cu, Cv)) {
    case 0: hipLaunchKernelGGL((pc_layer_kernel<3, 32, UP>), grid, tpb, 0, s, g); break;
    case 1: hipLaunchKernelGGL((pc_layer_kernel<32, 64, UP>), grid, tpb, 0, s, g); break;
    default: hipLaunchKernelGGL((pc_layer_kernel<64, 128, UP>), grid, tpb, 0, s, g); break;
  }
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

template <typename K>
int pc_launch_net(K kernel, const float* x, int64_t n, const float* w0, const float* b0, const float* w1, const float* b1,
                  const float* w2, const float* b2, float* out, void* stream) {
  if (n < 0) return MVK_EINVAL;
  if (n == 0) return MVK_OK;
  if (!x || !w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !out) return MVK_EINVAL;
  const long long tiles = ((long long)n + PC_T - 1) / PC_T;
  if (tiles > 0x7fffffffLL) return MVK_EINVAL;
  constexpr int lds = PC_LDS_FLOATS * (int)sizeof(float);
  static_assert(lds <= 160 * 1024, "one workgroup's LDS");
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  PcNetArgs g;
  g.x = x, g.w0 = w0, g.b0 = b0, g.w1 = w1, g.b1 = b1, g.w2 = w2, g.b2 = b2, g.out = out, g.n = n;
  g.wvec0 = mvk_aligned16(w0) ? 1 : 0, g.wvec1 = mvk_aligned16(w1) ? 1 : 0, g.wvec2 = mvk_aligned16(w2) ? 1 : 0;
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(PC_TPB), lds, mvk_stream(stream), g);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // namespace

extern "C" {

int mvk_conv3s2_ok(int H, int W, int Cu, int Cv) { return (H >= 1 && W >= 1 && H <= 4096 && W <= 4096 && pc_shape(Cu, Cv) >= 0) ? 1 : 0; }

int mvk_polyconv_tile(void) { return PC_T; }

int mvk_conv3s2_down(const float* U, const float* Wref, const float* bias, float* V, int n, int H, int W, int Cu, int Cv, int act,
                     int u_nchw, const float* v_act_src, int v_act, void* stream) {
  return pc_launch_layer<false>(U, Wref, bias, V, n, H, W, Cu, Cv, act, u_nchw, v_act_src, v_act, stream);
}

int mvk_conv3s2_up(const float* V, const float* Wref, const float* bias, float* U, int n, int H, int W, int Cu, int Cv, int act,
                   int u_nchw, const float* u_act_src, int u_act, void* stream) {
  return pc_launch_layer<true>(V, Wref, bias, U, n, H, W, Cu, Cv, act, u_nchw, u_act_src, u_act, stream);
}

int mvk_conv3s2_wgrad(const float* U, const float* V, float* dWref, float* db, int db_side, int n, int H, int W, int Cu, int Cv,
                      int u_nchw, int accumulate, float* ws, int64_t ws_floats, void* stream) {
  if (!mvk_conv3s2_ok(H, W, Cu, Cv) || n < 0 || db_side < 0 || db_side > 2 || (db_side != 0) != (db != nullptr)) return MVK_EINVAL;
  if (!dWref || !ws || (u_nchw && Cu != 3)) return MVK_EINVAL;
  if (n > 0 && (!U || !V)) return MVK_EINVAL;
  const int h = (H + 1) / 2, wd = (W + 1) / 2;
  if ((long long)n * H * W > 0x7fffffffLL / 4) return MVK_EINVAL;
  const int slab = 9 * Cu * Cv + 128, tiles = ((Cu + 15) / 16) * (Cv / 16);
  const long long rows = (long long)n * h * wd;
  // the slices depend on the shape alone: the same problem is always added up in the same order
  long long Z = (rows + 127) / 128;
  if (Z > 2048 / tiles) Z = 2048 / tiles;
  if (Z > ws_floats / slab) Z = ws_floats / slab;
  if (Z < 1) {
    if (ws_floats < slab) return MVK_EINVAL;
    Z = 1;
  }
  int chunk = (int)((rows + Z - 1) / Z);
  chunk = (chunk + 3) / 4 * 4;
  if (chunk < 4) chunk = 4;
  PcWgArgs g;
  g.U = U, g.V = V, g.slabs = ws, g.n = n, g.H = H, g.W = W, g.h = h, g.wd = wd, g.u_nchw = u_nchw, g.Z = (int)Z, g.chunk = chunk;
  g.db_side = db_side;
  const dim3 grid((unsigned)((tiles * Z + 3) / 4)), tpb(256);
  hipStream_t s = mvk_stream(stream);
  switch (pc_shape(Cu, Cv)) {
    case 0: hipLaunchKernelGGL((pc_wgrad_kernel<3, 32>), grid, tpb, 0, s, g); break;
    case 1: hipLaunchKernelGGL((pc_wgrad_kernel<32, 64>), grid, tpb, 0, s, g); break;
    default: hipLaunchKernelGGL((pc_wgrad_kernel<64, 128>), grid, tpb, 0, s, g); break;
  }
  MVK_CHECK_LAUNCH();
  const int count = 9 * Cu * Cv, ndb = db_side == 1 ? Cv : db_side == 2 ? Cu : 0;
  hipLaunchKernelGGL(pc_wgrad_finish_kernel, dim3((unsigned)((count + ndb + PC_FIN_E - 1) / PC_FIN_E)), dim3(PC_FIN_E * PC_FIN_G), 0, s,
                     ws, (int)Z, slab, count, ndb, dWref, db, accumulate);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_polyenc_fwd(const float* x, int64_t n, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* h3, void* stream) {
  return pc_launch_net(polyenc_kernel, x, n, w0, b0, w1, b1, w2, b2, h3, stream);
}

int mvk_polydec_fwd(const float* h0, int64_t n, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* out, void* stream) {
  if (n > 0 && !mvk_aligned16(h0)) return MVK_EINVAL;
  return pc_launch_net(polydec_kernel, h0, n, w0, b0, w1, b1, w2, b2, out, stream);
}

}  // extern "C"
