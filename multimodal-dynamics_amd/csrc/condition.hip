// The operand join of the conditional models (the reference's torch.cat((x, c.float()), dim=-1), vae.py:231-237, 286-291, with the
// one-hot of its categorical branch, vae.py:337-344): out[r] = [x[r] | condition of row r | 0] as one [rows][width] fp32 matrix,
// width = K + cd padded to the MFMA K-step, in ONE launch (before: a memset and two strided block copies per consumer).
//   - the condition is either real-valued rows (cond [rows][cd]) or one class index per row (cond_idx [rows]); the kernel writes
//     the one-hot row itself, so no one-hot tensor exists in memory;
//   - an index outside [0, cd) is ordinary input: the row's condition block is all zero and bit 0 of *bad_index is set (a vector
//     atomic, by the one thread that owns the row's first condition column); nothing is read or written out of bounds;
//   - EVERY element of out is written (the padding too: the padded weight columns are zero, but 0 * NaN is not).
// A streaming copy: one thread per 16 bytes of out, grid-stride, no LDS; 16-byte loads of x where K, ldx and the pointers allow,
// an element-per-thread kernel otherwise.
// Tiled form (mmdyn_concat_condition_tiled): x holds x_rows rows and out row r reads x[r % x_rows] -- the features of a batch joined
// to N candidate conditions per row without the features being repeated in memory.  The same two kernels: x_rows == rows is the
// plain join (the row index is then used as it is; the choice is uniform over the launch).
#include "common.h"

namespace {

// value of out[r][col] for col >= K
__device__ __forceinline__ float cond_elem(const float* __restrict__ cond, int64_t idx, int r, int j, int cd) {
  if (j >= cd) return 0.f;
  if (cond) return cond[(size_t)r * cd + j];
  return idx == (int64_t)j ? 1.f : 0.f;
}

// the row of x that out row r reads
__device__ __forceinline__ int x_row(int r, int rows, int x_rows) { return x_rows == rows ? r : r % x_rows; }

// K % 4 == 0, ldx % 4 == 0, x and out 16-byte aligned: a quad of out never straddles the x | condition border
__global__ __launch_bounds__(256) void concat_condition_vec_kernel(const float* __restrict__ x, const float* __restrict__ cond,
                                                                   const int64_t* __restrict__ cond_idx, float* __restrict__ out,
                                                                   int* __restrict__ bad_index, int rows, int x_rows, int K, int ldx,
                                                                   int cd, int width) {
  const int wq = width >> 2;
  const int64_t quads = (int64_t)rows * wq;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int r = (int)(q / wq), c0 = 4 * (int)(q - (int64_t)r * wq);
    f32x4 v;
    if (c0 < K) {
      v = *reinterpret_cast<const f32x4*>(x + (size_t)x_row(r, rows, x_rows) * ldx + c0);
    } else if (c0 < K + cd) {
      int64_t idx = -1;
      if (cond_idx) {
        idx = cond_idx[r];
        if (idx < 0 || idx >= cd) {
          idx = -1;
          if (c0 == K && bad_index) atomicOr(bad_index, 1);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = cond_elem(cond, idx, r, c0 - K + k, cd);
    } else {
      v = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    *reinterpret_cast<f32x4*>(out + (size_t)r * width + c0) = v;
  }
}

// any K / ldx / alignment: one element per thread
__global__ __launch_bounds__(256) void concat_condition_elem_kernel(const float* __restrict__ x, const float* __restrict__ cond,
                                                                    const int64_t* __restrict__ cond_idx, float* __restrict__ out,
                                                                    int* __restrict__ bad_index, int rows, int x_rows, int K, int ldx,
                                                                    int cd, int width) {
  const int64_t n = (int64_t)rows * width;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / width), c = (int)(i - (int64_t)r * width);
    float v = 0.f;
    if (c < K) {
      v = x[(size_t)x_row(r, rows, x_rows) * ldx + c];
    } else if (c < K + cd) {
      int64_t idx = -1;
      if (cond_idx) {
        idx = cond_idx[r];
        if (idx < 0 || idx >= cd) {
          idx = -1;
          if (c == K && bad_index) atomicOr(bad_index, 1);
        }
      }
      v = cond_elem(cond, idx, r, c - K, cd);
    }
    out[i] = v;
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mmdyn_concat_condition_tiled(const float* x, const float* cond, const int64_t* cond_idx, float* out, int* bad_index,
                                            int rows, int x_rows, int K, int ldx, int cd, int width, void* stream) {
  if (!x || !out || (cond == nullptr) == (cond_idx == nullptr)) return MMDYN_ERR_NULL;          // exactly one condition source
  if (rows <= 0 || K <= 0 || ldx < K || cd <= 0 || width <= 0 || width % 32 || (int64_t)K + cd > width) return MMDYN_ERR_SHAPE;
  if (x_rows <= 0 || rows % x_rows) return MMDYN_ERR_SHAPE;
  if ((int64_t)rows * width >= (1LL << 31) || (int64_t)x_rows * ldx >= (1LL << 31)) return MMDYN_ERR_RANGE;
  const bool vec = K % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(concat_condition_vec_kernel, dim3(ew_grid((int64_t)rows * width / 4)), dim3(256), 0, ST, x, cond, cond_idx,
                       out, bad_index, rows, x_rows, K, ldx, cd, width);
  else
    hipLaunchKernelGGL(concat_condition_elem_kernel, dim3(ew_grid((int64_t)rows * width)), dim3(256), 0, ST, x, cond, cond_idx, out,
                       bad_index, rows, x_rows, K, ldx, cd, width);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_concat_condition(const float* x, const float* cond, const int64_t* cond_idx, float* out, int* bad_index,
                                      int rows, int K, int ldx, int cd, int width, void* stream) {
  return mmdyn_concat_condition_tiled(x, cond, cond_idx, out, bad_index, rows, rows, K, ldx, cd, width, stream);
}
