// Importance-weighted K-sample bound (Burda et al., "Importance Weighted Autoencoders"; no reference op: the reference scores a
// sample with ONE draw and the analytic KL, problems.py:401-458):
//   L_K(x) = log (1/K) sum_k p(x|z_k) p(z_k) / q(z_k|x),  z_k ~ q(z|x)
// per request row, from K draws that share ONE encoder pass.  Two small kernels around the existing decoders and row kernels:
//   - iw_latent: z_k = eps_k * exp(lv / 2) + mu for the K draws of every row -- the fp32 expression of poe_fwd_kernel /
//     reparam_fwd_kernel, so the same (mu, lv, eps) give the same bits -- and beside it the density ratio of each draw,
//     ratio_k = log q(z_k|x) - log p(z_k) = sum_l 0.5 (z^2 - eps^2 - lv) (the 2 pi terms cancel; E_q[ratio] is the analytic KL),
//     in fp64 from the fp32 z the decoders will read.  One wavefront per (k, b) row, 16-byte lane accesses, a fixed-order fp64
//     reduction (lane-local in l order, then the xor butterfly): no atomics, the same bits in every run;
//   - iw_assemble_rows: log_w_k = -rec_k - kl_weight * ratio_k from the [K][B] row tables the row kernels (elbo_rows.hip) filled,
//     out[b] = -(logsumexp_k log_w_k - log K) and the effective sample size of the weights, max-subtracted, fp64.  One thread per
//     row b walks k, so the table reads coalesce across b.
// Both are memory-bound and tiny beside the decoders they bracket.
#include "common.h"

#include <math.h>

namespace {

// row = k * B + b of the [K][B] tables; eps / z rows of L floats, mu / lv rows of stride ld
template <bool VEC>
__global__ __launch_bounds__(256) void iw_latent_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int ld,
                                                        const float* __restrict__ eps_noise, float* __restrict__ z,
                                                        double* __restrict__ ratio, int rows, int B, int L) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row % B;
    const float* __restrict__ m_row = mu + (size_t)b * ld;
    const float* __restrict__ v_row = lv + (size_t)b * ld;
    const float* __restrict__ e_row = eps_noise + (size_t)row * L;
    float* __restrict__ z_row = z + (size_t)row * L;
    double acc = 0.0;
    if constexpr (VEC) {
      for (int q = lane; q < (L >> 2); q += 64) {
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(m_row + 4 * q);
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(v_row + 4 * q);
        const f32x4 e4 = *reinterpret_cast<const f32x4*>(e_row + 4 * q);
        f32x4 z4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float m = m4[k], v = v4[k];
          const float zv = e4[k] * expf(0.5f * v) + m;          // (the expression of reparam_fwd_kernel, term for term)
          z4[k] = zv;
          acc += 0.5 * ((double)zv * (double)zv - (double)e4[k] * (double)e4[k] - (double)v);
        }
        *reinterpret_cast<f32x4*>(z_row + 4 * q) = z4;
      }
    } else {
      for (int l = lane; l < L; l += 64) {
        const float m = m_row[l], v = v_row[l], e = e_row[l];
        const float zv = e * expf(0.5f * v) + m;
        z_row[l] = zv;
        acc += 0.5 * ((double)zv * (double)zv - (double)e * (double)e - (double)v);
      }
    }
    acc = wave_sum_d(acc);
    if (lane == 0) ratio[row] = acc;
  }
}

__device__ __forceinline__ bool present(uint32_t word, int m) { return ((word >> (8 * m)) & 0xffu) != 0u; }

// log_w[k][b] = -(bce[0][k][b] + bce[1][k][b] + pose_multiplier * mse[k][b]) - kl_weight * ratio[k][b] over the terms whose target the
// row holds (products and sums rounded one by one: no contraction, so K = 1 returns exactly the fp32 rounding of that fp64 sum)
__device__ __forceinline__ double iw_log_w(const double* bce, const double* mse, const double* ratio, int n_bce, bool on0, bool on1,
                                           bool on2, size_t KB, size_t o, double pm, double klw) {
  double rec = 0.0;
  if (n_bce > 0 && on0) rec = __dadd_rn(rec, bce[o]);
  if (n_bce > 1 && on1) rec = __dadd_rn(rec, bce[KB + o]);
  if (mse && on2) rec = __dadd_rn(rec, __dmul_rn(pm, mse[o]));
  return -__dadd_rn(rec, __dmul_rn(klw, ratio[o]));
}

__global__ __launch_bounds__(256) void iw_assemble_rows_kernel(double* __restrict__ bce, double* __restrict__ mse,
                                                               const double* __restrict__ ratio, const uint32_t* __restrict__ tavail,
                                                               float* __restrict__ out, float* __restrict__ ess,
                                                               double* __restrict__ log_w, int n_bce, int K, int B,
                                                               float pose_multiplier, float kl_weight_arg,
                                                               const float* __restrict__ kl_weight_dev) {
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  const double pm = (double)pose_multiplier, klw = (double)kl_weight;
  const size_t KB = (size_t)K * B;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    const uint32_t word = tavail ? tavail[b] : 0x01010101u;
    const bool on0 = present(word, 0), on1 = present(word, 1), on2 = present(word, 2);
    // pass 1: the weights' maximum (NaN kept aside: fmax drops it), the published log_w, zeros into the entries of absent terms
    double mx = -INFINITY;
    bool nan = false;
    for (int k = 0; k < K; ++k) {
      const size_t o = (size_t)k * B + b;
      const double lw = iw_log_w(bce, mse, ratio, n_bce, on0, on1, on2, KB, o, pm, klw);
      if (log_w) log_w[o] = lw;
      nan = nan || (lw != lw);
      mx = fmax(mx, lw);
    }
    // pass 2: sum_k exp(lw_k - mx) and sum_k exp(2 (lw_k - mx)); a weight of -inf adds exp(-inf) = 0
    double s1 = 0.0, s2 = 0.0;
    const bool finite_max = mx > -INFINITY && mx < INFINITY;
    if (finite_max && !nan) {
      for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * B + b;
        const double e = exp(iw_log_w(bce, mse, ratio, n_bce, on0, on1, on2, KB, o, pm, klw) - mx);
        s1 += e;
        s2 += e * e;
      }
    }
    for (int k = 0; k < K; ++k) {          // (after the last read of the tables)
      const size_t o = (size_t)k * B + b;
      if (n_bce > 0 && !on0) bce[o] = 0.0;
      if (n_bce > 1 && !on1) bce[KB + o] = 0.0;
      if (mse && !on2) mse[o] = 0.0;
    }
    double res, n_eff;
    if (nan) {
      res = NAN;
      n_eff = NAN;
    } else if (!finite_max) {              // every weight zero: out = +inf; a weight of +inf: out = -inf; no sample size either way
      res = -mx;
      n_eff = NAN;
    } else {
      res = -((mx + log(s1)) - log((double)K));
      n_eff = s1 * s1 / s2;                // exp(2 lse(log_w) - lse(2 log_w)) with the common 2 mx taken out
    }
    out[b] = (float)res;
    if (ess) ess[b] = (float)n_eff;
  }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mmdyn_iw_latent(const float* mu, const float* lv, int ld, const float* eps, float* z, double* ratio, int K, int B,
                               int L, void* stream) {
  if (!mu || !lv || !eps || !z || !ratio) return MMDYN_ERR_NULL;
  if (K <= 0 || B <= 0 || L <= 0 || ld < L) return MMDYN_ERR_SHAPE;
  if ((int64_t)K * B * L >= (1LL << 31)) return MMDYN_ERR_RANGE;
  const int rows = K * B;
  const bool vec = L % 4 == 0 && ld % 4 == 0 && (((uintptr_t)mu | (uintptr_t)lv | (uintptr_t)eps | (uintptr_t)z) & 15) == 0;
  const int grid = ew_grid((int64_t)rows * 64);
  if (vec)
    hipLaunchKernelGGL(iw_latent_kernel<true>, dim3(grid), dim3(256), 0, ST, mu, lv, ld, eps, z, ratio, rows, B, L);
  else
    hipLaunchKernelGGL(iw_latent_kernel<false>, dim3(grid), dim3(256), 0, ST, mu, lv, ld, eps, z, ratio, rows, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_iw_assemble_rows(double* bce_rows, double* mse_rows, const double* ratio, const uint8_t* tavail, float* out,
                                      float* ess, double* log_w, int n_bce, int K, int B, float pose_multiplier, float kl_weight,
                                      const float* kl_weight_dev, void* stream) {
  if (!ratio || !out) return MMDYN_ERR_NULL;
  if (K <= 0 || B <= 0 || n_bce < 0 || n_bce > 2 || ((uintptr_t)tavail & 3)) return MMDYN_ERR_SHAPE;
  if ((int64_t)K * B >= (1LL << 31)) return MMDYN_ERR_RANGE;
  hipLaunchKernelGGL(iw_assemble_rows_kernel, dim3(ew_grid(B)), dim3(256), 0, ST, bce_rows, mse_rows, ratio,
                     reinterpret_cast<const uint32_t*>(tavail), out, ess, log_w, bce_rows ? n_bce : 0, K, B, pose_multiplier,
                     kl_weight, kl_weight_dev);
  MMDYN_LAUNCH_CHECK();
}
