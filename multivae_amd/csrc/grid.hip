// The picture of a set of modality tensors: data/datasets/utils.py:50-91 (adapt_shape), torch.cat, torchvision.utils.make_grid
// (normalize=False) and the mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8) of metrics/visualization/
// visualization_class.py:93-108 and trainers/base/base_trainer.py:830-917, in ONE launch.  The definition is in DESIGN.md ("The image
// grid") and include/mvk.h.
//
// Layout of the work
//  * A gather over the OUTPUT.  Both outputs are flat arrays of n = 3 Hg Wg elements: the float grid [3,Hg,Wg] and the byte image
//    [Hg,Wg,3].  A thread owns one 4-element chunk of one of them: it finds, element by element, the (channel, row, column) of the
//    grid, from that the tile and the position inside it, from the tile its source (a table of at most MVK_GRID_MAX_SOURCES
//    entries in the kernel arguments: first tile, pointer, shape, centring offsets), reads the pixel -- or takes pad_value outside
//    the tiles, 0 inside a tile but outside its centred image -- and stores the chunk with one instruction: 16 bytes of the float
//    grid, 4 bytes of the image.  Neighbouring lanes own neighbouring chunks, so a wave stores 1 KiB / 256 contiguous bytes.
//  * Alignment.  Chunk j of an output covers the elements [4 j - shift, 4 j - shift + 4), shift = the elements between the last
//    aligned address and the base (float: (base / 4) % 4, bytes: base % 4): every whole chunk is an aligned wide store wherever the
//    caller's buffer begins, and the first and the last chunk, when they are cut by the ends of the array, store their elements
//    one by one.  Every element is written exactly once; nothing is cleared beforehand and nothing is added atomically.
//  * The first ceil((n + shift_f) / 4) chunks of the launch are the float grid's, the others the image's (either part may be
//    absent).  The two parts read the same pixels; the sources of one picture are a few MB and stay in the L2.
//  * The bytes are b = (uint8) clamp(fl(fl(255 x) + 0.5), 0, 255) with the product rounded before the sum (never contracted to
//    an fma, whatever -ffp-contract says: grid_quantise); fmaxf(NaN, 0) = 0 sends a NaN to 0.
#include "common.hpp"

namespace {

constexpr int GRID_TPB = 256;

struct GridSource {
  const float* data;
  unsigned tile0;    // first tile of this source
  int c, h, w;       // its images are [c, h, w]
  int top, left;     // rows above / columns left of the centred image inside the H x W tile
};

struct GridTable {
  GridSource src[MVK_GRID_MAX_SOURCES];
  int S;              // sources with at least one image
  unsigned T;         // tiles
  unsigned xmaps;     // tiles per grid row
  unsigned Hg, Wg;    // the grid
  unsigned H, W;      // a tile
  unsigned cellh, cellw;  // H + padding, W + padding
  unsigned off;       // rows / columns in front of the first cell: padding (0 for the borderless single image)
  float pad_value;
  unsigned n;         // 3 Hg Wg
  float* grid;        // [3, Hg, Wg] or NULL
  unsigned char* image;  // [Hg, Wg, 3] or NULL
  unsigned shift_f, shift_b;   // see above
  unsigned chunks_f;  // chunks of the float grid (0 without it)
};
static_assert(sizeof(GridTable) <= 4096, "kernel-argument limit");

// the value of grid pixel (channel ch, row y, column x)
__device__ __forceinline__ float grid_value(const GridTable& G, unsigned ch, unsigned y, unsigned x) {
  if (y < G.off || x < G.off) return G.pad_value;
  const unsigned yy = y - G.off, xx = x - G.off;
  const unsigned cy = yy / G.cellh, cx = xx / G.cellw;
  const unsigned ly = yy - cy * G.cellh, lx = xx - cx * G.cellw;
  const unsigned k = cy * G.xmaps + cx;  // cx < xmaps by construction of Wg
  if (ly >= G.H || lx >= G.W || k >= G.T) return G.pad_value;
  int s = 0;
  for (int j = 1; j < G.S; ++j)
    if (k >= G.src[j].tile0) s = j;
  const GridSource& R = G.src[s];
  const int iy = (int)ly - R.top, ix = (int)lx - R.left;
  if (iy < 0 || iy >= R.h || ix < 0 || ix >= R.w) return 0.f;  // the zeros of the centring belong to the tile
  int c = (int)ch;
  if (R.c == 1) c = 0;              // one channel: replicated
  else if (R.c == 2 && c == 2) return 0.f;  // two channels: the third is zero
  const long long img = (long long)(k - R.tile0);
  return R.data[((img * R.c + c) * R.h + iy) * (long long)R.w + ix];
}

// hipcc's __fmul_rn / __fadd_rn are a plain `x * y` / `x + y` (they round separately only in a build with
// OCML_BASIC_ROUNDED_OPERATIONS), so the contraction is switched off for this function instead: neither operation carries the
// `contract` flag and no later pass may fuse them.
__device__ __forceinline__ unsigned char grid_quantise(float v) {
#pragma clang fp contract(off)
  const float p = v * 255.f;
  const float q = p + 0.5f;
  return (unsigned char)(int)fminf(fmaxf(q, 0.f), 255.f);  // fmaxf(NaN, 0) = 0
}

__global__ __launch_bounds__(GRID_TPB) void image_grid_kernel(const GridTable G) {
  const unsigned chunk = blockIdx.x * GRID_TPB + threadIdx.x;
  const bool bytes = chunk >= G.chunks_f;
  if (bytes && !G.image) return;  // the last workgroup's threads past the float grid's chunks
  const unsigned j = bytes ? chunk - G.chunks_f : chunk;
  const unsigned shift = bytes ? G.shift_b : G.shift_f;
  // elements [e0, e0 + 4) of the output, cut to [0, n)
  const long long e0 = 4ll * j - shift;
  if (e0 >= (long long)G.n) return;  // past the last chunk of the launch's last part
  const unsigned lo = e0 < 0 ? 0u : (unsigned)e0;
  const unsigned hi = e0 + 4 > (long long)G.n ? G.n : (unsigned)(e0 + 4);
  // position of element `lo`: float grid (ch, y, x) with x fastest, image (y, x, ch) with ch fastest
  unsigned ch, y, x;
  if (bytes) {
    const unsigned p = lo / 3;
    ch = lo - 3 * p;
    y = p / G.Wg;
    x = p - y * G.Wg;
  } else {
    const unsigned plane = G.Hg * G.Wg;
    ch = lo / plane;
    const unsigned r = lo - ch * plane;
    y = r / G.Wg;
    x = r - y * G.Wg;
  }
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long e = e0 + u;
    if (e >= (long long)lo && e < (long long)hi) {
      v[u] = grid_value(G, ch, y, x);
      if (bytes) {
        if (++ch == 3) {
          ch = 0;
          if (++x == G.Wg) x = 0, ++y;
        }
      } else if (++x == G.Wg) {
        x = 0;
        if (++y == G.Hg) y = 0, ++ch;
      }
    }
  }
  const bool whole = hi - lo == 4;
  if (bytes) {
    unsigned char* out = G.image + e0;  // 4-byte aligned
    if (whole) {
      const unsigned word = (unsigned)grid_quantise(v[0]) | ((unsigned)grid_quantise(v[1]) << 8) |
                            ((unsigned)grid_quantise(v[2]) << 16) | ((unsigned)grid_quantise(v[3]) << 24);
      *reinterpret_cast<unsigned*>(out) = word;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u >= (long long)lo && e0 + u < (long long)hi) out[u] = grid_quantise(v[u]);
    }
  } else {
    float* out = G.grid + e0;  // 16-byte aligned
    if (whole) {
      typedef float v4 __attribute__((ext_vector_type(4)));
      v4 w;
      w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
      *reinterpret_cast<v4*>(out) = w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u >= (long long)lo && e0 + u < (long long)hi) out[u] = v[u];
    }
  }
}

// the geometry of a call; MVK_EINVAL for what the entry points refuse.  Fills the table when `G` is given.
int grid_geometry(const mvk_grid_src* srcs, int S, int nrow, int padding, GridTable* G, long long* T_out, long long* Hg_out,
                  long long* Wg_out) {
  if (S < 0 || S > MVK_GRID_MAX_SOURCES || nrow <= 0 || padding < 0 || (S > 0 && !srcs)) return MVK_EINVAL;
  long long T = 0, H = 0, W = 0;
  for (int i = 0; i < S; ++i) {
    const mvk_grid_src& s = srcs[i];
    if (s.n < 0 || s.c <= 0 || s.h <= 0 || s.w <= 0) return MVK_EINVAL;
    if (s.n == 0) continue;  // an empty tensor adds no tile and takes no part in the tile size
    T += s.n;
    H = s.h > H ? s.h : H;
    W = s.w > W ? s.w : W;
  }
  *T_out = T;
  *Hg_out = *Wg_out = 0;
  if (T == 0) return MVK_OK;
  const bool single = T == 1;  // make_grid hands a single image back as it is
  const long long xmaps = nrow < T ? nrow : T, ymaps = (T + xmaps - 1) / xmaps;
  const long long cellh = single ? H : H + padding, cellw = single ? W : W + padding, off = single ? 0 : padding;
  // every factor is below 2^32, so the products fit 64 bits; the grid itself must index with 31
  const long long Hg = ymaps * cellh + off, Wg = xmaps * cellw + off;
  if (Hg >= (1ll << 31) || Wg >= (1ll << 31) || Hg * Wg >= ((1ll << 31) + 2) / 3) return MVK_EINVAL;  // 3 Hg Wg >= 2^31
  *Hg_out = Hg;
  *Wg_out = Wg;
  if (!G) return MVK_OK;
  G->S = 0;
  unsigned tile0 = 0;
  for (int i = 0; i < S; ++i) {
    const mvk_grid_src& s = srcs[i];
    if (s.n == 0) continue;
    if (!s.data) return MVK_EINVAL;
    GridSource& R = G->src[G->S++];
    R.data = s.data;
    R.tile0 = tile0;
    R.c = s.c, R.h = s.h, R.w = s.w;
    R.top = (int)((H - s.h) / 2), R.left = (int)((W - s.w) / 2);  // floor in front, ceil behind
    tile0 += (unsigned)s.n;
  }
  G->T = (unsigned)T, G->xmaps = (unsigned)xmaps;
  G->Hg = (unsigned)Hg, G->Wg = (unsigned)Wg, G->H = (unsigned)H, G->W = (unsigned)W;
  G->cellh = (unsigned)cellh, G->cellw = (unsigned)cellw, G->off = (unsigned)off;
  G->n = (unsigned)(3 * Hg * Wg);
  return MVK_OK;
}

}  // namespace

extern "C" {

int mvk_image_grid_size(const mvk_grid_src* srcs, int S, int nrow, int padding, int64_t* T, int64_t* Hg, int64_t* Wg) {
  if (!T || !Hg || !Wg) return MVK_EINVAL;
  long long t, h, w;
  const int rc = grid_geometry(srcs, S, nrow, padding, nullptr, &t, &h, &w);
  if (rc != MVK_OK) return rc;
  *T = t, *Hg = h, *Wg = w;
  return MVK_OK;
}

int mvk_image_grid(const mvk_grid_src* srcs, int S, int nrow, int padding, float pad_value, float* grid, uint8_t* image,
                   void* stream) {
  GridTable G{};
  long long T, Hg, Wg;
  const int rc = grid_geometry(srcs, S, nrow, padding, &G, &T, &Hg, &Wg);  // the refusals come before any launch
  if (rc != MVK_OK) return rc;
  if (T == 0 || (!grid && !image)) return MVK_OK;
  if (grid && (reinterpret_cast<uintptr_t>(grid) & 3u)) return MVK_EINVAL;
  G.pad_value = pad_value;
  G.grid = grid;
  G.image = image;
  G.shift_f = grid ? (unsigned)((reinterpret_cast<uintptr_t>(grid) >> 2) & 3u) : 0u;
  G.shift_b = image ? (unsigned)(reinterpret_cast<uintptr_t>(image) & 3u) : 0u;
  G.chunks_f = grid ? (unsigned)(((long long)G.n + G.shift_f + 3) / 4) : 0u;
  const long long chunks = (long long)G.chunks_f + (image ? ((long long)G.n + G.shift_b + 3) / 4 : 0);
  const long long blocks = (chunks + GRID_TPB - 1) / GRID_TPB;  // n < 2^31: at most 2^30 + 2 chunks, 2^22 + 1 workgroups
  hipLaunchKernelGGL(image_grid_kernel, dim3((unsigned)blocks), dim3(GRID_TPB), 0, mvk_stream(stream), G);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
