// Per-sample ELBO terms (the reduce=False branch of the reference's problems.py:401-458): every loss kernel of
// latent_elbo.hip folds the batch into one slot; these keep one value per SAMPLE.
//   - BCE-with-logits rows for the G decoder passes that share one target (and one loss mask): a block owns a piece of ONE sample's
//     row and walks all G passes over it, so the target / mask piece is read from HBM once for all of them;
//   - MSE rows (the 7-DoF pose term) and KL rows: one wavefront per row;
//   - the assembly of the [B] result from the three tables, with the reference's KL (the batch total in every row,
//     problems.py:429, 456) or the per-sample one.
// Evaluation only: no gradient outputs.  Element arithmetic = bce_elem (common.h), the expression of bce_logits_groups_kernel;
// per-thread fp32 sums of 4 elements, fp64 from there on, 64-lane shuffle reduction, one double atomic per (block, pass).
#include "common.h"

namespace {

struct RowGroups {
  int slot[MMDYN_BCE_GROUPS_MAX];
};

template <bool MASKED>
__global__ __launch_bounds__(256) void bce_rows_groups_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                              const float* __restrict__ mask, double* __restrict__ rows,
                                                              double* __restrict__ unmasked, const RowGroups gs, int G, int Bg,
                                                              int chw, int hw, int mask_c) {
  constexpr int GM = MMDYN_BCE_GROUPS_MAX;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int chw4 = chw >> 2;
  const float* __restrict__ tg = target + (size_t)b * chw;
  double acc[GM], acc_u[MASKED ? GM : 1];          // (the plain sums beside the masked ones exist in the MASKED instance only)
#pragma unroll
  for (int g = 0; g < GM; ++g) {
    acc[g] = 0.0;
    if constexpr (MASKED) acc_u[g] = 0.0;
  }
  for (int i = blockIdx.x * 256 + tid; i < chw4; i += gridDim.x * 256) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(tg + 4 * (size_t)i);
    f32x4 mk = {1.f, 1.f, 1.f, 1.f};
    if constexpr (MASKED) {
      // the loss mask multiplies logits and target (problems.py:445-447): [Bg][1 or C][H][W] (mask_c == 1: broadcast over channels)
      const int e0 = 4 * i, ch = e0 / hw, pix = e0 - ch * hw;
      mk = *reinterpret_cast<const f32x4*>(mask + ((size_t)b * mask_c + (mask_c == 1 ? 0 : ch)) * hw + pix);
    }
#pragma unroll
    for (int g = 0; g < GM; ++g) {
      if (g < G && gs.slot[g] >= 0) {          // (block-uniform)
        const f32x4 xv = *reinterpret_cast<const f32x4*>(logits + ((size_t)g * Bg + b) * chw + 4 * (size_t)i);
        float part = 0.f;
        if constexpr (MASKED) {
          float part_u = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float xm = xv[k] * mk[k], tm = t[k] * mk[k];
            float l, sg, lu, su;
            bce_elem(xm, tm, l, sg);
            bce_elem(xv[k], t[k], lu, su);
            part += l;
            part_u += lu;
          }
          acc_u[g] += (double)part_u;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float l, sg;
            bce_elem(xv[k], t[k], l, sg);
            part += l;
          }
        }
        acc[g] += (double)part;
      }
    }
  }
  __shared__ double red[2][GM][4];
  const bool with_u = MASKED && unmasked != nullptr;
#pragma unroll
  for (int g = 0; g < GM; ++g) {
    if (g < G && gs.slot[g] >= 0) {
      const double s = wave_sum_d(acc[g]);
      if ((tid & 63) == 0) red[0][g][tid >> 6] = s;
      if constexpr (MASKED) {
        if (with_u) {
          const double su = wave_sum_d(acc_u[g]);
          if ((tid & 63) == 0) red[1][g][tid >> 6] = su;
        }
      }
    }
  }
  __syncthreads();
  if (tid < G && gs.slot[tid] >= 0) {          // two passes may share a slot: atomics, like the scalar kernels
    const size_t o = (size_t)gs.slot[tid] * Bg + b;
    atomicAdd(rows + o, red[0][tid][0] + red[0][tid][1] + red[0][tid][2] + red[0][tid][3]);
    if (with_u) atomicAdd(unmasked + o, red[1][tid][0] + red[1][tid][1] + red[1][tid][2] + red[1][tid][3]);
  }
}

// rows[slot[g]][b] += sum_n (r[g][b][:] - t[b][:])^2: one wavefront per (g, b); same element expression as mse_groups_kernel
__global__ __launch_bounds__(256) void mse_rows_groups_kernel(const float* __restrict__ r, const float* __restrict__ t,
                                                              double* __restrict__ rows, const RowGroups gs, int G, int Bg, int n) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
  for (int row = wave; row < G * Bg; row += nwaves) {
    const int g = row / Bg, b = row - g * Bg;
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) {
      const float d = r[(size_t)row * n + k] - t[(size_t)b * n + k];
      acc += (double)(d * d);
    }
    acc = wave_sum_d(acc);
    if (lane == 0) atomicAdd(rows + (size_t)gs.slot[g] * Bg + b, acc);
  }
}

// kl_rows[row] = -0.5 * sum_L (1 + lv - mu^2 - exp(lv)): one wavefront per row of the [rows][L] tables; the element expression of
// poe_fwd_kernel / reparam_fwd_kernel (fp32 terms, fp64 sums), so the rows of a pass add up to its kl_sum to fp64 rounding
__global__ __launch_bounds__(256) void kl_rows_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                      double* __restrict__ kl_rows, int rows, int L) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
  for (int row = wave; row < rows; row += nwaves) {
    double kl = 0.0;
    for (int l = lane; l < L; l += 64) {
      const float m = mu[(size_t)row * L + l], v = lv[(size_t)row * L + l];
      kl += (double)(1.f + v - m * m - expf(v));
    }
    kl = wave_sum_d(kl);
    if (lane == 0) kl_rows[row] = -0.5 * kl;
  }
}

// partials[p][b] = bce_rows[p][b] + pose_multiplier * mse_rows[p][b] + kl_weight * (kl_mode ? kl_rows[p][b] : kl_sum[p]);
// out[b] = sum_p.  No division by B (problems.py:415-417, 455-456).
__global__ void elbo_assemble_rows_kernel(const double* __restrict__ bce, const double* __restrict__ mse,
                                          const double* __restrict__ kl_rows, const double* __restrict__ kl_sum,
                                          float* __restrict__ out, float* __restrict__ partials, int P, int B, float kl_weight_arg,
                                          float pose_multiplier, const float* __restrict__ kl_weight_dev, int kl_mode) {
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    double tot = 0.0;
    for (int p = 0; p < P; ++p) {
      const size_t o = (size_t)p * B + b;
      const double kl = kl_mode ? (kl_rows ? kl_rows[o] : 0.0) : (kl_sum ? kl_sum[p] : 0.0);
      const double v = (bce ? bce[o] : 0.0) + (double)pose_multiplier * (mse ? mse[o] : 0.0) + (double)kl_weight * kl;
      if (partials) partials[o] = (float)v;
      tot += v;
    }
    out[b] = (float)tot;
  }
}

int copy_slots(const int* slot_of_group, int G, int n_slots, bool negative_ok, RowGroups* gs) {
  if (G <= 0 || G > MMDYN_BCE_GROUPS_MAX || n_slots <= 0) return MMDYN_ERR_SHAPE;
  for (int i = 0; i < G; ++i) {
    if (slot_of_group[i] >= n_slots || (slot_of_group[i] < 0 && !negative_ok)) return MMDYN_ERR_SHAPE;
    gs->slot[i] = slot_of_group[i];
  }
  return MMDYN_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mmdyn_bce_logits_rows_groups(const float* logits, const float* target, const float* mask, int mask_channels,
                                            double* rows_out, double* unmasked_rows, const int* slot_of_group, int n_slots, int G,
                                            int Bg, int chw, int hw, void* stream) {
  if (!logits || !target || !rows_out || !slot_of_group) return MMDYN_ERR_NULL;
  RowGroups gs{};
  if (int e = copy_slots(slot_of_group, G, n_slots, true, &gs)) return e;
  if (Bg <= 0 || Bg > 65535 || chw <= 0 || chw % 4) return MMDYN_ERR_SHAPE;
  if (mask && (hw <= 0 || hw % 4 || chw % hw || (mask_channels != 1 && mask_channels != chw / hw))) return MMDYN_ERR_SHAPE;
  // enough blocks per sample row to fill the machine at small batch sizes, at most one per 256 float4 of the row
  int bpr = ceil_div(1024, Bg);
  const int most = ceil_div(chw / 4, 256);
  if (bpr > most) bpr = most;
  if (mask)
    hipLaunchKernelGGL(bce_rows_groups_kernel<true>, dim3(bpr, Bg), dim3(256), 0, ST, logits, target, mask, rows_out, unmasked_rows,
                       gs, G, Bg, chw, hw, mask_channels);
  else
    hipLaunchKernelGGL(bce_rows_groups_kernel<false>, dim3(bpr, Bg), dim3(256), 0, ST, logits, target, mask, rows_out,
                       (double*)nullptr, gs, G, Bg, chw, 0, 1);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_mse_rows_groups(const float* r, const float* t, double* rows_out, const int* slot_of_group, int n_slots, int G,
                                     int Bg, int n, void* stream) {
  if (!r || !t || !rows_out || !slot_of_group) return MMDYN_ERR_NULL;
  RowGroups gs{};
  if (int e = copy_slots(slot_of_group, G, n_slots, false, &gs)) return e;
  if (Bg <= 0 || n <= 0 || (int64_t)G * Bg * n >= (1LL << 31)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(mse_rows_groups_kernel, dim3(ew_grid((int64_t)G * Bg * 64)), dim3(256), 0, ST, r, t, rows_out, gs, G, Bg, n);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_kl_rows(const float* mu, const float* logvar, double* kl_rows, int P, int B, int L, void* stream) {
  if (!mu || !logvar || !kl_rows) return MMDYN_ERR_NULL;
  if (P <= 0 || B <= 0 || L <= 0 || (int64_t)P * B * L >= (1LL << 31)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(kl_rows_kernel, dim3(ew_grid((int64_t)P * B * 64)), dim3(256), 0, ST, mu, logvar, kl_rows, P * B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble_rows(const double* bce_rows, const double* mse_rows, const double* kl_rows, const double* kl_sum,
                                        float* out, float* partials, int P, int B, float kl_weight, float pose_multiplier,
                                        const float* kl_weight_dev, int kl_mode, void* stream) {
  if (!out) return MMDYN_ERR_NULL;
  if (P <= 0 || B <= 0 || (kl_mode != 0 && kl_mode != 1)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(elbo_assemble_rows_kernel, dim3(ew_grid(B)), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, kl_sum, out,
                     partials, P, B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}
