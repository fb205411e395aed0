// Image grids for the epoch log: torchvision.utils.make_grid(torch.cat((a[:take], b[:take])), nrow, padding, pad_value=0) of the
// reference's Problem._write_images (problems.py:580-604), the sigmoid in front of it where the tensors are decoder logits, and its
// writer's float32 * 255 -> clip -> uint8 conversion, as ONE launch that writes the bytes of the file's scanlines:
//   out uint8 [Hg][Wg][3] (HWC), Hg = ymaps * (H + padding) + padding, Wg = xmaps * (W + padding) + padding,
//   xmaps = min(nrow, N), ymaps = ceil(N / xmaps); image k at row (k / xmaps) * (H + padding) + padding, column
//   (k % xmaps) * (W + padding) + padding; every other pixel 0 (the border, the gaps, the cells of a partly filled last row);
//   N == 1: the image alone (make_grid returns a single image as it is), which the launcher expresses as padding = 0.
// A pure gather, bound by memory traffic: the output is indexed as a flat byte range (a row is 3 * Wg bytes, in general no multiple
// of four), a lane forms four consecutive bytes -- they lie in exactly two consecutive pixels -- and stores them as one dword; the
// up to three bytes behind the last whole dword are stored one by one.  Every byte of the range is written, the pad included, so
// no memset runs in front; no byte outside it is.  No LDS, no scratch, no atomics.
#include "common.h"

namespace {

struct GridGeom {
  int m0;             // images taken from src0: the list is src0[0 .. m0) then src1[0 .. N - m0)
  int N, C, H, W;
  int xmaps, Wg;
  int pad, cell_h, cell_w;   // offset of the first tile, and the pitch of the tiles (H + padding, W + padding)
};

// float32 * 255, clip, truncate: the conversion of the reference's image writer.  NaN fails both comparisons and gives 0.
__device__ __forceinline__ uint32_t to_byte(float v) {
  const float t = v * 255.0f;
  return t >= 255.0f ? 255u : (t > 0.0f ? (uint32_t)t : 0u);
}

// Offset of channel 0 of output pixel `pix` in its source (src1 when the image index is >= m0), or -1 for a pad pixel
__device__ __forceinline__ int64_t pixel_source(const GridGeom& g, int pix, bool& second) {
  const int y = pix / g.Wg - g.pad, x = pix % g.Wg - g.pad;
  second = false;
  if (y < 0 || x < 0) return -1;
  const int ty = y / g.cell_h, iy = y % g.cell_h, tx = x / g.cell_w, ix = x % g.cell_w;
  const int k = ty * g.xmaps + tx;
  if (iy >= g.H || ix >= g.W || tx >= g.xmaps || k >= g.N) return -1;
  second = k >= g.m0;
  return (int64_t)(second ? k - g.m0 : k) * g.C * g.H * g.W + (int64_t)iy * g.W + ix;
}

template <bool LOGITS>
__device__ __forceinline__ uint32_t channel_byte(const float* __restrict__ src, int64_t off, int ch, const GridGeom& g) {
  if (off < 0) return 0u;
  const float x = src[off + (g.C == 3 ? (int64_t)ch * g.H * g.W : 0)];
  return to_byte(LOGITS ? sigmoid_exact(x) : x);
}

template <bool LOGITS>
__global__ __launch_bounds__(256) void image_grid_u8_kernel(const float* __restrict__ src0, const float* __restrict__ src1,
                                                            uint8_t* __restrict__ out, const GridGeom g, int total) {
  const int n4 = total / 4;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
  for (int q = tid; q < n4; q += nthreads) {
    const int e0 = 4 * q;
    const int pix = e0 / 3, ch0 = e0 % 3;
    bool second_a, second_b;
    const int64_t off_a = pixel_source(g, pix, second_a), off_b = pixel_source(g, pix + 1, second_b);
    const float* sa = second_a ? src1 : src0;
    const float* sb = second_b ? src1 : src0;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = ch0 + k;                  // 0 .. 5: the channels of pixel `pix`, then those of its right neighbour
      const uint32_t b = c < 3 ? channel_byte<LOGITS>(sa, off_a, c, g) : channel_byte<LOGITS>(sb, off_b, c - 3, g);
      word |= b << (8 * k);
    }
    // one dword store (out is 4-byte aligned -- checked by the launcher -- and e0 a multiple of four)
    __builtin_memcpy(__builtin_assume_aligned(out + e0, 4), &word, 4);
  }
  for (int64_t e = 4 * (int64_t)n4 + tid; e < total; e += nthreads) {
    bool second;
    const int64_t off = pixel_source(g, (int)(e / 3), second);
    out[e] = (uint8_t)channel_byte<LOGITS>(second ? src1 : src0, off, e % 3, g);
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mmdyn_image_grid_u8(const float* src0, const float* src1, uint8_t* out, int n0, int n1, int take, int C, int H, int W,
                                   int nrow, int padding, int logits, void* stream) {
  if (!src0 || !out) return MMDYN_ERR_NULL;
  if ((src1 && n1 <= 0) || (!src1 && n1 != 0)) return MMDYN_ERR_SHAPE;
  if ((C != 1 && C != 3) || H < 1 || W < 1 || take < 1 || nrow < 1 || padding < 0 || n0 < 1) return MMDYN_ERR_SHAPE;
  if ((((uintptr_t)src0 | (uintptr_t)src1 | (uintptr_t)out) & 3) != 0) return MMDYN_ERR_SHAPE;
  // every product below stays under 2^63: each factor is checked against 2^31 before it enters the next one
  const int64_t LIM = 1LL << 31;
  const int64_t chw = (int64_t)H * W;
  if (chw >= LIM || chw * C >= LIM || chw * C * n0 >= LIM || chw * C * n1 >= LIM) return MMDYN_ERR_RANGE;
  const int m0 = n0 < take ? n0 : take, m1 = n1 < take ? n1 : take;
  const int64_t N = (int64_t)m0 + m1;
  const int pad = N == 1 ? 0 : padding;       // a single image comes back alone, with no border
  const int64_t xmaps = nrow < N ? nrow : N, ymaps = (N + xmaps - 1) / xmaps;
  const int64_t cell_h = (int64_t)H + pad, cell_w = (int64_t)W + pad;
  if (cell_h >= LIM || cell_w >= LIM) return MMDYN_ERR_RANGE;
  const int64_t Hg = ymaps * cell_h + pad, Wg = xmaps * cell_w + pad;
  if (Hg >= LIM || Wg >= LIM || Hg * Wg >= LIM || Hg * Wg * 3 >= LIM) return MMDYN_ERR_RANGE;
  const int total = (int)(Hg * Wg * 3);
  GridGeom g;
  g.m0 = m0;
  g.N = (int)N;
  g.C = C;
  g.H = H;
  g.W = W;
  g.xmaps = (int)xmaps;
  g.Wg = (int)Wg;
  g.pad = pad;
  g.cell_h = (int)cell_h;
  g.cell_w = (int)cell_w;
  const int blocks = ew_grid(total / 4 ? total / 4 : total);
  if (logits)
    hipLaunchKernelGGL(image_grid_u8_kernel<true>, dim3(blocks), dim3(256), 0, ST, src0, src1, out, g, total);
  else
    hipLaunchKernelGGL(image_grid_u8_kernel<false>, dim3(blocks), dim3(256), 0, ST, src0, src1, out, g, total);
  MMDYN_LAUNCH_CHECK();
}
