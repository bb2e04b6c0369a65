// A batch of a device-resident dataset in one launch per modality (data/datasets/cub.py, CUB.device_batcher): the rows of a token
// store / a byte image store picked by a device index tensor, expanded to what the models take.  The definition is in DESIGN.md
// ("The CUB batch") and include/mvk.h.
//
// Layout of the work
//  * Both kernels scatter nothing and gather rows: output row b comes from store row index[b] (captions) or index[b] / div (images:
//    div captions share a picture).  The indices are taken on trust: the caller range-checks an epoch's order on the host.
//  * An output row (V one-hot floats, E pixel floats) starts wherever b V or b E puts it, so a row is cut in three: a HEAD of at
//    most three floats up to the next 16-byte boundary of the output, a BODY of whole 16-byte stores, one per lane, and a TAIL of at
//    most three floats.  Every element is written exactly once; nothing is cleared beforehand and nothing is added atomically.
//  * text_onehot_kernel: one wave per (b, l) row, grid-strided.  The row's one division (b = row / L) is the only one: a lane knows
//    the column of its four floats from the loop counter and compares it with the row's token.  Lane 0 writes the row's token and
//    mask element.  Without a one-hot output, text_tokens_kernel takes a thread per (b, l).
//  * u8_image_kernel: one workgroup per (row, segment of IMG_TPB body chunks), grid-strided; the division by the segments per row is
//    per workgroup.  A lane reads its four bytes as one 32-bit word when the store row's body starts on a 4-byte boundary, byte by
//    byte otherwise.  float(byte) / 255 is the IEEE division (the build has no fast-math flag: hipcc rounds fp32 division correctly),
//    which the tests compare bitwise with the host's for all 256 bytes.
//  * Grids are capped at DB_MAX_BLOCKS workgroups (256 CUs x 8) and stride over the rest.
#include "common.hpp"

namespace {

constexpr int DB_TPB = 256;
constexpr int DB_WAVES = DB_TPB / MVK_WAVE;
constexpr long long DB_MAX_BLOCKS = 2048;

typedef float f4 __attribute__((ext_vector_type(4)));

// floats between p and the next 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ int head_floats(const float* p) { return (int)((4u - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u); }

__global__ __launch_bounds__(DB_TPB) void text_tokens_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ lengths,
                                                             const int64_t* __restrict__ index, int B, int L,
                                                             int64_t* __restrict__ out_tokens, float* __restrict__ mask) {
  const long long rows = (long long)B * L;
  for (long long row = (long long)blockIdx.x * DB_TPB + threadIdx.x; row < rows; row += (long long)gridDim.x * DB_TPB) {
    const int b = (int)(row / L), l = (int)(row - (long long)b * L);
    const long long r = index[b];
    if (out_tokens) out_tokens[row] = tokens[r * L + l];
    mask[row] = l < lengths[r] ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(DB_TPB) void text_onehot_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ lengths,
                                                             const int64_t* __restrict__ index, int B, int L, int V,
                                                             int64_t* __restrict__ out_tokens, float* __restrict__ mask,
                                                             float* __restrict__ one_hot) {
  const int lane = threadIdx.x & (MVK_WAVE - 1);
  const long long rows = (long long)B * L;
  for (long long row = (long long)blockIdx.x * DB_WAVES + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * DB_WAVES) {
    const int b = (int)(row / L), l = (int)(row - (long long)b * L);
    const long long r = index[b];
    const int t = tokens[r * L + l];
    if (lane == 0) {
      if (out_tokens) out_tokens[row] = t;
      mask[row] = l < lengths[r] ? 1.f : 0.f;
    }
    float* p = one_hot + row * V;
    int head = head_floats(p);
    head = head < V ? head : V;
    const int nb = (V - head) >> 2, tail0 = head + 4 * nb;
    if (lane < head) p[lane] = lane == t ? 1.f : 0.f;
    for (int i = lane; i < nb; i += MVK_WAVE) {
      const int d = t - (head + 4 * i);  // the token's place inside this chunk, if 0 <= d < 4
      f4 w;
      w[0] = d == 0 ? 1.f : 0.f, w[1] = d == 1 ? 1.f : 0.f, w[2] = d == 2 ? 1.f : 0.f, w[3] = d == 3 ? 1.f : 0.f;
      *reinterpret_cast<f4*>(p + head + 4 * i) = w;  // 16-byte aligned
    }
    if (lane < V - tail0) p[tail0 + lane] = tail0 + lane == t ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(DB_TPB) void u8_image_kernel(const uint8_t* __restrict__ store, const int64_t* __restrict__ index, int B,
                                                          long long E, int div, int segs, float* __restrict__ out) {
  const long long items = (long long)B * segs;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = (int)(item / segs), seg = (int)(item - (long long)b * segs);
    const uint8_t* s = store + (index[b] / div) * E;
    float* p = out + b * E;
    long long head = head_floats(p);
    head = head < E ? head : E;
    const long long nb = (E - head) >> 2, tail0 = head + 4 * nb;
    if (seg == 0) {  // the first segment's lanes also write the ends of the row
      if (threadIdx.x < head) p[threadIdx.x] = (float)s[threadIdx.x] / 255.f;
      if (threadIdx.x < E - tail0) p[tail0 + threadIdx.x] = (float)s[tail0 + threadIdx.x] / 255.f;
    }
    const long long i = (long long)seg * DB_TPB + threadIdx.x;
    if (i < nb) {
      const uint8_t* q = s + head + 4 * i;
      unsigned word;
      if ((reinterpret_cast<uintptr_t>(s + head) & 3u) == 0)  // wave-uniform: the row's body begins on a 4-byte boundary
        word = *reinterpret_cast<const unsigned*>(q);
      else
        word = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
      f4 w;
      w[0] = (float)(word & 255u) / 255.f, w[1] = (float)((word >> 8) & 255u) / 255.f;
      w[2] = (float)((word >> 16) & 255u) / 255.f, w[3] = (float)(word >> 24) / 255.f;
      *reinterpret_cast<f4*>(p + head + 4 * i) = w;  // 16-byte aligned
    }
  }
}

}  // namespace

extern "C" {

int mvk_text_batch(const int32_t* tokens, const int32_t* lengths, const int64_t* index, int64_t N, int B, int L, int V,
                   int64_t* out_tokens, float* padding_mask, float* one_hot, void* stream) {
  if (B < 0 || N < 0 || L < 1 || V < 1) return MVK_EINVAL;
  if (B == 0) return MVK_OK;
  if (!tokens || !lengths || !index || !padding_mask || N < 1) return MVK_EINVAL;
  if ((reinterpret_cast<uintptr_t>(padding_mask) & 3u) || (reinterpret_cast<uintptr_t>(one_hot) & 3u) ||
      (reinterpret_cast<uintptr_t>(out_tokens) & 7u))
    return MVK_EINVAL;
  const long long rows = (long long)B * L;
  if (one_hot) {
    const long long blocks = (rows + DB_WAVES - 1) / DB_WAVES;
    hipLaunchKernelGGL(text_onehot_kernel, dim3((unsigned)(blocks < DB_MAX_BLOCKS ? blocks : DB_MAX_BLOCKS)), dim3(DB_TPB), 0,
                       mvk_stream(stream), tokens, lengths, index, B, L, V, out_tokens, padding_mask, one_hot);
  } else {
    const long long blocks = (rows + DB_TPB - 1) / DB_TPB;
    hipLaunchKernelGGL(text_tokens_kernel, dim3((unsigned)(blocks < DB_MAX_BLOCKS ? blocks : DB_MAX_BLOCKS)), dim3(DB_TPB), 0,
                       mvk_stream(stream), tokens, lengths, index, B, L, out_tokens, padding_mask);
  }
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

int mvk_u8_image_batch(const uint8_t* store, const int64_t* index, int64_t N, int B, int64_t E, int div, float* out, void* stream) {
  if (B < 0 || N < 0 || E < 1 || div < 1) return MVK_EINVAL;
  if (B == 0) return MVK_OK;
  if (!store || !index || !out || N < 1 || (reinterpret_cast<uintptr_t>(out) & 3u)) return MVK_EINVAL;
  // body chunks of a row: at most E / 4 whatever its head; a row with none still has one segment for its head and tail
  const long long chunks = E / 4, segs = chunks > DB_TPB ? (chunks + DB_TPB - 1) / DB_TPB : 1;
  if (segs >= (1ll << 31)) return MVK_EINVAL;
  const long long items = (long long)B * segs;
  hipLaunchKernelGGL(u8_image_kernel, dim3((unsigned)(items < DB_MAX_BLOCKS ? items : DB_MAX_BLOCKS)), dim3(DB_TPB), 0,
                     mvk_stream(stream), store, index, B, (long long)E, div, (int)segs, out);
  MVK_CHECK_LAUNCH();
  return MVK_OK;
}

}  // extern "C"
