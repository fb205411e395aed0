// Reconstruction losses and the assembly of the ELBO (the reference's problems.py:401-458).  Element arithmetic of every BCE kernel =
// bce_elem (common.h, shared with the last decoder layer's fused loss epilogue, tconv_out3.hip); per-thread fp32 sums of 4
// elements, fp64 from there on, 64-lane shuffle reduction, fp64 atomics.
//   - batch sums (problems.py:433-449): BCE-with-logits / MSE with their gradients in the same pass, for one decoder pass or for
//     the G passes that share ONE target; one double atomic per block; elbo_assemble = (sum recon + kl_weight * KL) / B;
//   - per-sample rows (the reduce=False branch): bce_rows_groups / mse_rows_groups keep one value per SAMPLE.  A BCE block owns a
//     piece of ONE sample's row and walks all G passes over it, so the target / mask piece is read from HBM once for all of them;
//     MSE rows (the 7-DoF pose term): one wavefront per row.  Flags: MASKED -- a loss mask multiplies logits and target, and the
//     unmasked sums are kept beside the masked ones; GRAD -- the gradient of the WEIGHTED per-sample ELBO, (1/B) sum_b w_b * row_b,
//     in the same pass: dlogit = ((sigmoid - t) * grad_scale) * w_rec[b] (the twin of the last decoder layer's weighted epilogue),
//     dr = (2 (r - t) * grad_scale) * w_rec[b], zeros for a discarded pass.  The scale products are written in that order so that
//     w = 1 reproduces the batch kernels' gradients bit for bit (x * 1.f == x).  The sums are NOT weighted.  Weights are not
//     inspected: NaN / Inf propagate;
//   - assemblies of the [B] result from the row tables: elbo_assemble_rows with the reference's KL (the batch total in every row,
//     problems.py:429, 456) or the per-sample one -- flag AVAIL: a target-availability word per row, a (row, term) whose target
//     is absent is written as 0 into its table and left out of the row sum; elbo_assemble_weighted: the weighted scalar, its
//     per-pass partials and the [B] vector of sum_b w_b that the reference's KL mode hands to the latent backward -- flag AVAIL (the
//     training step on a mixed batch): one table per term and a target-availability word per row, counts and per-term sums beside
//     the loss; term_weights: the three gradient seeds' weight vectors of such a step, present ? w_b : 0 by selection;
//     iw_assemble_rows: the importance-weighted K-sample bound L_K(x) = log (1/K) sum_k p(x|z_k) p(z_k) / q(z_k|x) from the
//     [K][B] row tables and the density ratios of latent.hip's iw_latent: log_w_k = -rec_k - kl_weight * ratio_k,
//     out[b] = -(logsumexp_k log_w_k - log K) and the effective sample size of the weights, max-subtracted, fp64.
#include "common.h"

#include <math.h>

#include <type_traits>

namespace {

// loss slot of each of the passes that share one target; a negative slot is a discarded reconstruction
struct RowGroups {
  int slot[MMDYN_BCE_GROUPS_MAX];
};

// The same reconstruction term for several decoder passes that share ONE target (the live passes of a modality in the
// multi-subset ELBO): logits [G][n], target [n], one loss slot per pass; blockIdx.y = pass.  A pass whose slot is negative
// is a discarded reconstruction: its logit gradient is zero and it adds nothing to the loss.
template <bool MASKED>
__global__ __launch_bounds__(256) void bce_logits_groups_kernel(const float* __restrict__ logits,
                                                                const float* __restrict__ target,
                                                                const float* __restrict__ mask,
                                                                float* __restrict__ dlogit, double* __restrict__ loss,
                                                                double* __restrict__ unmasked, const RowGroups gs,
                                                                int64_t n, int chw, int hw, int mask_c, float grad_scale) {
  const int grp = blockIdx.y, slot = gs.slot[grp];
  const float* __restrict__ lg = logits + (size_t)grp * n;
  float* __restrict__ dl = dlogit ? dlogit + (size_t)grp * n : nullptr;
  const int64_t n4 = n >> 2;
  if (slot < 0) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (dl)
      for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<f32x4*>(dl)[i] = zero;
    return;
  }
  double acc = 0.0, acc_u = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 xv = reinterpret_cast<const f32x4*>(lg)[i], t = reinterpret_cast<const f32x4*>(target)[i];
    f32x4 d;
    float part = 0.f;
    if constexpr (MASKED) {
      // the loss mask multiplies logits and target (problems.py:445-447): [B][1 or C][H][W] (mask_c == 1: broadcast over channels)
      const int64_t e0 = i * 4, b = e0 / chw;
      const int rem = (int)(e0 - b * chw);
      const int ch = rem / hw, pix = rem - ch * hw;
      const f32x4 mk = *reinterpret_cast<const f32x4*>(mask + (b * mask_c + (mask_c == 1 ? 0 : ch)) * hw + pix);
      float part_u = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xm = xv[k] * mk[k], tm = t[k] * mk[k];
        float l, sg, lu, su;
        bce_elem(xm, tm, l, sg);
        bce_elem(xv[k], t[k], lu, su);
        part += l;
        d[k] = mk[k] * (sg - tm) * grad_scale;
        part_u += lu;
      }
      acc_u += (double)part_u;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float l, sg;
        bce_elem(xv[k], t[k], l, sg);
        part += l;
        d[k] = (sg - t[k]) * grad_scale;
      }
    }
    acc += (double)part;
    if (dl) reinterpret_cast<f32x4*>(dl)[i] = d;
  }
  block_atomic_add(acc, loss + slot);
  if constexpr (MASKED) {
    if (unmasked) {
      __syncthreads();          // block_atomic_add's scratch is reused
      block_atomic_add(acc_u, unmasked + slot);
    }
  }
}

__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ r, const float* __restrict__ t,
                                                  float* __restrict__ dr, double* __restrict__ loss, int64_t n,
                                                  float grad_scale) {
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float d = r[i] - t[i];
    acc += (double)(d * d);
    if (dr) dr[i] = 2.f * d * grad_scale;
  }
  block_atomic_add(acc, loss);
}

// the pose term of several passes against ONE target (the pose-bearing subsets of the multi-subset ELBO): r / dr [G][n], t [n],
// one loss slot per pass; blockIdx.y = pass.  Same arithmetic per pass as mse_kernel.
__global__ __launch_bounds__(256) void mse_groups_kernel(const float* __restrict__ r, const float* __restrict__ t,
                                                         float* __restrict__ dr, double* __restrict__ loss, const RowGroups gs,
                                                         int64_t n, float grad_scale) {
  const int grp = blockIdx.y;
  r += (size_t)grp * n;
  if (dr) dr += (size_t)grp * n;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = r[i] - t[i];
    acc += (double)(d * d);
    if (dr) dr[i] = 2.f * d * grad_scale;
  }
  block_atomic_add(acc, loss + gs.slot[grp]);
}

// rows[slot[g]][b] (+ unmasked[slot[g]][b]) += the BCE sum of sample b in pass g: logits [G][Bg][chw], target [Bg][chw].
// GRAD: dlogit [G][Bg][chw] is written for every pass g < G, w_rec [Bg].
template <bool MASKED, bool GRAD>
__global__ __launch_bounds__(256) void bce_rows_groups_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                              const float* __restrict__ mask, float* __restrict__ dlogit,
                                                              const float* __restrict__ w_rec, double* __restrict__ rows,
                                                              double* __restrict__ unmasked, const RowGroups gs, int G, int Bg,
                                                              int chw, int hw, int mask_c, float grad_scale) {
  constexpr int GM = MMDYN_BCE_GROUPS_MAX;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int chw4 = chw >> 2;
  const float* __restrict__ tg = target + (size_t)b * chw;
  float wr = 1.f;
  if constexpr (GRAD) wr = w_rec[b];               // (block-uniform: a block owns a piece of ONE sample's row)
  double acc[GM], acc_u[MASKED ? GM : 1];          // (the plain sums beside the masked ones exist in the MASKED instances only)
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
      if (g < G) {                                 // (block-uniform, like the slot test)
        const size_t o = ((size_t)g * Bg + b) * chw + 4 * (size_t)i;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};            // a discarded pass (slot < 0): zero gradient, no loss
        if (gs.slot[g] >= 0) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(logits + o);
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
              if constexpr (GRAD) d[k] = (mk[k] * (sg - tm) * grad_scale) * wr;
            }
            acc_u[g] += (double)part_u;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              float l, sg;
              bce_elem(xv[k], t[k], l, sg);
              part += l;
              if constexpr (GRAD) d[k] = ((sg - t[k]) * grad_scale) * wr;
            }
          }
          acc[g] += (double)part;
        }
        if constexpr (GRAD) *reinterpret_cast<f32x4*>(dlogit + o) = d;
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
  if (tid < G && gs.slot[tid] >= 0) {          // two passes may share a slot: atomics, like the batch kernels
    const size_t o = (size_t)gs.slot[tid] * Bg + b;
    atomicAdd(rows + o, red[0][tid][0] + red[0][tid][1] + red[0][tid][2] + red[0][tid][3]);
    if (with_u) atomicAdd(unmasked + o, red[1][tid][0] + red[1][tid][1] + red[1][tid][2] + red[1][tid][3]);
  }
}

// rows[slot[g]][b] += sum_n (r[g][b][:] - t[b][:])^2: one wavefront per (g, b); same element expression as mse_groups_kernel.
// GRAD: dr = (2 (r - t) * grad_scale) * w_rec[b]
template <bool GRAD>
__global__ __launch_bounds__(256) void mse_rows_groups_kernel(const float* __restrict__ r, const float* __restrict__ t,
                                                              float* __restrict__ dr, const float* __restrict__ w_rec,
                                                              double* __restrict__ rows, const RowGroups gs, int G, int Bg, int n,
                                                              float grad_scale) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
  for (int row = wave; row < G * Bg; row += nwaves) {
    const int g = row / Bg, b = row - g * Bg;
    float wr = 1.f;
    if constexpr (GRAD) wr = w_rec[b];
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) {
      const float d = r[(size_t)row * n + k] - t[(size_t)b * n + k];
      acc += (double)(d * d);
      if constexpr (GRAD) dr[(size_t)row * n + k] = (2.f * d * grad_scale) * wr;
    }
    acc = wave_sum_d(acc);
    if (lane == 0) atomicAdd(rows + (size_t)gs.slot[g] * Bg + b, acc);
  }
}

__global__ void elbo_assemble_kernel(const double* __restrict__ bce, const double* __restrict__ mse,
                                     const double* __restrict__ kl, float* __restrict__ loss,
                                     float* __restrict__ partials, int P, int B, float kl_weight_arg,
                                     float pose_multiplier, const float* __restrict__ kl_weight_dev) {
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double tot = 0.0;
    for (int p = 0; p < P; ++p) {
      double v = ((bce ? bce[p] : 0.0) + (double)pose_multiplier * (mse ? mse[p] : 0.0) +
                  (double)kl_weight * (kl ? kl[p] : 0.0)) /
                 (double)B;
      if (partials) partials[p] = (float)v;
      tot += v;
    }
    loss[0] = (float)tot;
  }
}

// target modality of slot p of the bce / mse table (negative: the slot has no target modality and always counts)
struct TermModal {
  int bce[MMDYN_MAX_PASSES], mse[MMDYN_MAX_PASSES];
};

// partials[p][b] = bce_rows[p][b] + pose_multiplier * mse_rows[p][b] + kl_weight * (kl_mode ? kl_rows[p][b] : kl_sum[p]);
// out[b] = sum_p.  No division by B (problems.py:415-417, 455-456).  AVAIL: an entry whose target the row does not hold is selected
// out of the sum (it may hold anything) and written back as 0 -- the tables are then outputs too.
template <bool AVAIL>
__global__ void elbo_assemble_rows_kernel(std::conditional_t<AVAIL, double, const double>* __restrict__ bce,
                                          std::conditional_t<AVAIL, double, const double>* __restrict__ mse,
                                          const double* __restrict__ kl_rows, const double* __restrict__ kl_sum,
                                          float* __restrict__ out, float* __restrict__ partials, const uint32_t* __restrict__ avail,
                                          const TermModal tm, int P, int B, float kl_weight_arg, float pose_multiplier,
                                          const float* __restrict__ kl_weight_dev, int kl_mode) {
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    uint32_t word = ALL_PRESENT;
    if constexpr (AVAIL) word = avail[b];
    double tot = 0.0;
    for (int p = 0; p < P; ++p) {
      const size_t o = (size_t)p * B + b;
      const double kl = kl_mode ? (kl_rows ? kl_rows[o] : 0.0) : (kl_sum ? kl_sum[p] : 0.0);
      double vb = 0.0, vm = 0.0;
      if (bce) {
        if (!AVAIL || tm.bce[p] < 0 || has(word, tm.bce[p])) vb = bce[o];
        else if constexpr (AVAIL) bce[o] = 0.0;
      }
      if (mse) {
        if (!AVAIL || tm.mse[p] < 0 || has(word, tm.mse[p])) vm = mse[o];
        else if constexpr (AVAIL) mse[o] = 0.0;
      }
      const double v = vb + (double)pose_multiplier * vm + (double)kl_weight * kl;
      if (partials) partials[o] = (float)v;
      tot += v;
    }
    out[b] = (float)tot;
  }
}

// ONE block.  Thread t owns the samples t, t + 256, ...: it writes their unweighted rows / partials (elbo_assemble_rows_kernel's
// expression) and adds w_b * term into its own fp64 sums in increasing b; the 256 sums of a quantity are then added by the fixed
// shuffle tree of wave_sum_d and the four wave totals in wave order -- no atomics, the same order in every run.
//   S[p]  = sum_b w_b * (bce[p][b] + pose_multiplier * mse[p][b]),  K[p] = sum_b w_b * kl_rows[p][b],  W = sum_b w_b
//   wpartials[p] = (S[p] + kl_weight * (kl_mode ? K[p] : W * kl_sum[p])) / B,  loss = sum_p wpartials[p]
// AVAIL (the training step on a mixed batch): one table per TERM -- bce is the visual term's, bce_t the tactile term's, mse the pose
// term's -- and a target-availability word per row (null table: all present); a (row, term) whose target is absent is selected out
// of every sum and its table entries are written back as 0.  w may then be null (= 1).  Beside the loss: present[m] = the number of
// rows that hold target m, term_sums[m][p] = the unweighted sum of term m's table over those rows.  The flag only adds statements:
// all present, the tactile table null, gives the bits of the plain instance.
template <bool AVAIL>
__global__ __launch_bounds__(256) void elbo_assemble_weighted_kernel(
    std::conditional_t<AVAIL, double, const double>* __restrict__ bce, std::conditional_t<AVAIL, double, const double>* __restrict__ mse,
    const double* __restrict__ kl_rows, const double* __restrict__ kl_sum, const float* __restrict__ w, float* __restrict__ loss,
    float* __restrict__ wpartials, float* __restrict__ out, float* __restrict__ partials, float* __restrict__ w_sum_out,
    double* __restrict__ bce_t, const uint32_t* __restrict__ tavail, double* __restrict__ present, double* __restrict__ term_sums, int P,
    int B, float kl_weight_arg, float pose_multiplier, const float* __restrict__ kl_weight_dev, int kl_mode) {
  constexpr int PM = MMDYN_MAX_PASSES;
  constexpr int NT = 3;                  // terms with a target of their own: visual BCE, tactile BCE, pose MSE
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  const int tid = threadIdx.x;
  double S[PM], K[PM], W = 0.0;
  double T[AVAIL ? NT * PM : 1], C[AVAIL ? NT : 1];
#pragma unroll
  for (int p = 0; p < PM; ++p) S[p] = K[p] = 0.0;
  if constexpr (AVAIL) {
#pragma unroll
    for (int i = 0; i < NT * PM; ++i) T[i] = 0.0;
#pragma unroll
    for (int m = 0; m < NT; ++m) C[m] = 0.0;
  }
  for (int b = tid; b < B; b += 256) {
    const double wb = (!AVAIL || w) ? (double)w[b] : 1.0;
    uint32_t word = ALL_PRESENT;
    if constexpr (AVAIL) {
      if (tavail) word = tavail[b];
#pragma unroll
      for (int m = 0; m < NT; ++m) C[m] += has(word, m) ? 1.0 : 0.0;
    }
    W += wb;
    double tot = 0.0;
#pragma unroll
    for (int p = 0; p < PM; ++p) {
      if (p < P) {
        const size_t o = (size_t)p * B + b;
        double bs = bce ? bce[o] : 0.0, ms = mse ? mse[o] : 0.0;
        if constexpr (AVAIL) {
          double bt = bce_t ? bce_t[o] : 0.0;
          if (!has(word, 0)) {           // (selections: what the entry of an absent target held reaches nothing)
            bs = 0.0;
            if (bce) bce[o] = 0.0;
          }
          if (!has(word, 1)) {
            bt = 0.0;
            if (bce_t) bce_t[o] = 0.0;
          }
          if (!has(word, 2)) {
            ms = 0.0;
            if (mse) mse[o] = 0.0;
          }
          T[0 * PM + p] += bs;
          T[1 * PM + p] += bt;
          T[2 * PM + p] += ms;
          bs = bs + bt;
        }
        const double rec = bs + (double)pose_multiplier * ms;
        const double klr = kl_rows ? kl_rows[o] : 0.0;
        const double kl = kl_mode ? klr : (kl_sum ? kl_sum[p] : 0.0);
        const double v = rec + (double)kl_weight * kl;
        if (partials) partials[o] = (float)v;
        tot += v;
        S[p] += wb * rec;
        K[p] += wb * klr;
      }
    }
    if (out) out[b] = (float)tot;
  }
  __shared__ double red[2 * PM + 1 + (AVAIL ? NT * PM + NT : 0)][4];
  const int wv = tid >> 6;
#pragma unroll
  for (int p = 0; p < PM; ++p) {
    const double s = wave_sum_d(S[p]), k = wave_sum_d(K[p]);
    if ((tid & 63) == 0) {
      red[p][wv] = s;
      red[PM + p][wv] = k;
    }
  }
  W = wave_sum_d(W);
  if ((tid & 63) == 0) red[2 * PM][wv] = W;
  if constexpr (AVAIL) {
#pragma unroll
    for (int i = 0; i < NT * PM; ++i) {
      const double t = wave_sum_d(T[i]);
      if ((tid & 63) == 0) red[2 * PM + 1 + i][wv] = t;
    }
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const double c = wave_sum_d(C[m]);
      if ((tid & 63) == 0) red[2 * PM + 1 + NT * PM + m][wv] = c;
    }
  }
  __syncthreads();
  const double Wt = red[2 * PM][0] + red[2 * PM][1] + red[2 * PM][2] + red[2 * PM][3];
  if (tid == 0) {
    double tot = 0.0;
    for (int p = 0; p < P; ++p) {
      const double Sp = red[p][0] + red[p][1] + red[p][2] + red[p][3];
      const double Kp = red[PM + p][0] + red[PM + p][1] + red[PM + p][2] + red[PM + p][3];
      const double kl = kl_mode ? Kp : Wt * (kl_sum ? kl_sum[p] : 0.0);
      const double v = (Sp + (double)kl_weight * kl) / (double)B;
      if (wpartials) wpartials[p] = (float)v;
      tot += v;
    }
    loss[0] = (float)tot;
  }
  if constexpr (AVAIL) {
    if (tid < NT * PM && term_sums) {                      // term_sums [NT][P]
      const int m = tid / PM, p = tid - m * PM;
      const double* r = red[2 * PM + 1 + tid];
      if (p < P) term_sums[m * P + p] = r[0] + r[1] + r[2] + r[3];
    }
    if (tid >= 64 && tid < 64 + NT && present) {
      const double* r = red[2 * PM + 1 + NT * PM + (tid - 64)];
      present[tid - 64] = r[0] + r[1] + r[2] + r[3];
    }
  }
  if (w_sum_out)
    for (int b = tid; b < B; b += 256) w_sum_out[b] = (float)Wt;
}

// w_term[m][b] = present(b, m) ? (w ? w[b] : 1) : 0 for the three target modalities (visual, tactile, pose): the weight vectors of
// the three gradient seeds of a mixed batch.  A select, never a product: the weight of an absent row (it may be NaN) reaches nothing.
// One 32-bit word per row, coalesced.
__global__ __launch_bounds__(256) void term_weights_kernel(const uint32_t* __restrict__ tavail, const float* __restrict__ w,
                                                           float* __restrict__ w_term, int B) {
  for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
    const uint32_t word = tavail ? tavail[b] : ALL_PRESENT;
    const float wb = w ? w[b] : 1.f;
#pragma unroll
    for (int m = 0; m < 3; ++m) w_term[(size_t)m * B + b] = has(word, m) ? wb : 0.f;
  }
}

// log_w[k][b] = -(bce[0][k][b] + bce[1][k][b] + pose_multiplier * mse[k][b]) - kl_weight * ratio[k][b] over the terms whose target the
// row holds (products and sums rounded one by one: no contraction, so K = 1 returns exactly the fp32 rounding of that fp64 sum)
__device__ __forceinline__ double iw_log_w(const double* bce, const double* mse, const double* ratio, int n_bce, bool has0, bool has1,
                                           bool has2, size_t KB, size_t o, double pm, double klw) {
  double rec = 0.0;
  if (n_bce > 0 && has0) rec = __dadd_rn(rec, bce[o]);
  if (n_bce > 1 && has1) rec = __dadd_rn(rec, bce[KB + o]);
  if (mse && has2) rec = __dadd_rn(rec, __dmul_rn(pm, mse[o]));
  return -__dadd_rn(rec, __dmul_rn(klw, ratio[o]));
}

// one thread per row b walks k, so the table reads coalesce across b
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
    const uint32_t word = tavail ? tavail[b] : ALL_PRESENT;
    const bool has0 = has(word, 0), has1 = has(word, 1), has2 = has(word, 2);
    // pass 1: the weights' maximum (NaN kept aside: fmax drops it), the published log_w, zeros into the entries of absent terms
    double mx = -INFINITY;
    bool nan = false;
    for (int k = 0; k < K; ++k) {
      const size_t o = (size_t)k * B + b;
      const double lw = iw_log_w(bce, mse, ratio, n_bce, has0, has1, has2, KB, o, pm, klw);
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
        const double e = exp(iw_log_w(bce, mse, ratio, n_bce, has0, has1, has2, KB, o, pm, klw) - mx);
        s1 += e;
        s2 += e * e;
      }
    }
    for (int k = 0; k < K; ++k) {          // (after the last read of the tables)
      const size_t o = (size_t)k * B + b;
      if (n_bce > 0 && !has0) bce[o] = 0.0;
      if (n_bce > 1 && !has1) bce[KB + o] = 0.0;
      if (mse && !has2) mse[o] = 0.0;
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

int copy_slots(const int* slot_of_group, int G, int n_slots, bool negative_ok, RowGroups* gs) {
  if (G <= 0 || G > MMDYN_BCE_GROUPS_MAX || n_slots <= 0) return MMDYN_ERR_SHAPE;
  for (int i = 0; i < G; ++i) {
    if (slot_of_group[i] >= n_slots || (slot_of_group[i] < 0 && !negative_ok)) return MMDYN_ERR_SHAPE;
    gs->slot[i] = slot_of_group[i];
  }
  return MMDYN_OK;
}

// enough blocks per sample row of chw floats to fill the machine at small batch sizes, at most one per 256 float4 of the row
int bce_rows_bpr(int Bg, int chw) {
  const int bpr = ceil_div(1024, Bg), most = ceil_div(chw / 4, 256);
  return bpr > most ? most : bpr;
}

}  // namespace

#define ST ((hipStream_t)stream)

static int bce_groups_launch(const float* logits, const float* target, const float* mask, float* dlogit,
                             double* loss_slots, double* unmasked_slots, const int* slot_of_group, int G, int64_t n,
                             int chw, int hw, int mask_channels, float grad_scale, void* stream) {
  if (!logits || !target || !loss_slots || !slot_of_group) return MMDYN_ERR_NULL;
  if (G <= 0 || G > MMDYN_BCE_GROUPS_MAX || n <= 0 || n % 4) return MMDYN_ERR_SHAPE;
  if (mask && (hw <= 0 || hw % 4 || chw <= 0 || chw % hw || n % chw || (mask_channels != 1 && mask_channels != chw / hw)))
    return MMDYN_ERR_SHAPE;
  RowGroups gs{};
  for (int i = 0; i < G; ++i) gs.slot[i] = slot_of_group[i];
  int g = ew_grid(n / 4);
  if (g > 512) g = 512;
  if (mask)
    hipLaunchKernelGGL(bce_logits_groups_kernel<true>, dim3(g, G), dim3(256), 0, ST, logits, target, mask, dlogit,
                       loss_slots, unmasked_slots, gs, n, chw, hw, mask_channels, grad_scale);
  else
    hipLaunchKernelGGL(bce_logits_groups_kernel<false>, dim3(g, G), dim3(256), 0, ST, logits, target, mask, dlogit,
                       loss_slots, unmasked_slots, gs, n, 0, 0, 1, grad_scale);
  MMDYN_LAUNCH_CHECK();
}

/* one pass: the grouped kernel with a single group (the same arithmetic, to the last bit, as a multi-pass launch) */
extern "C" int mmdyn_bce_logits(const float* logits, const float* target, const float* mask, float* dlogit,
                                double* loss_sum, int64_t n, int chw, int hw, int mask_channels, float grad_scale,
                                void* stream) {
  const int slot0 = 0;
  return bce_groups_launch(logits, target, mask, dlogit, loss_sum, nullptr, &slot0, 1, n, chw, hw, mask_channels, grad_scale,
                           stream);
}

extern "C" int mmdyn_bce_logits_groups(const float* logits, const float* target, float* dlogit, double* loss_slots,
                                       const int* slot_of_group, int G, int64_t n, float grad_scale, void* stream) {
  return bce_groups_launch(logits, target, nullptr, dlogit, loss_slots, nullptr, slot_of_group, G, n, 0, 0, 1, grad_scale,
                           stream);
}

extern "C" int mmdyn_bce_logits_groups_masked(const float* logits, const float* target, const float* mask, float* dlogit,
                                              double* loss_slots, double* unmasked_slots, const int* slot_of_group, int G,
                                              int64_t n, int chw, int hw, int mask_channels, float grad_scale,
                                              void* stream) {
  if (!mask) return MMDYN_ERR_NULL;
  return bce_groups_launch(logits, target, mask, dlogit, loss_slots, unmasked_slots, slot_of_group, G, n, chw, hw,
                           mask_channels, grad_scale, stream);
}

extern "C" int mmdyn_mse(const float* r, const float* t, float* dr, double* loss_sum, int64_t n,
                         float grad_scale, void* stream) {
  if (!r || !t || !loss_sum) return MMDYN_ERR_NULL;
  int g = ew_grid(n);
  if (g > 256) g = 256;
  hipLaunchKernelGGL(mse_kernel, dim3(g), dim3(256), 0, ST, r, t, dr, loss_sum, n, grad_scale);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_mse_groups(const float* r, const float* t, float* dr, double* loss_slots, const int* slot_of_group, int G,
                                int64_t n, float grad_scale, void* stream) {
  if (!r || !t || !loss_slots || !slot_of_group) return MMDYN_ERR_NULL;
  if (G <= 0 || G > MMDYN_BCE_GROUPS_MAX || n <= 0) return MMDYN_ERR_SHAPE;
  RowGroups gs{};
  for (int i = 0; i < G; ++i) {
    if (slot_of_group[i] < 0) return MMDYN_ERR_SHAPE;
    gs.slot[i] = slot_of_group[i];
  }
  int g = ew_grid(n);
  if (g > 64) g = 64;
  hipLaunchKernelGGL(mse_groups_kernel, dim3(g, G), dim3(256), 0, ST, r, t, dr, loss_slots, gs, n, grad_scale);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_bce_logits_rows_groups(const float* logits, const float* target, const float* mask, int mask_channels,
                                            double* rows_out, double* unmasked_rows, const int* slot_of_group, int n_slots, int G,
                                            int Bg, int chw, int hw, void* stream) {
  if (!logits || !target || !rows_out || !slot_of_group) return MMDYN_ERR_NULL;
  RowGroups gs{};
  if (int e = copy_slots(slot_of_group, G, n_slots, true, &gs)) return e;
  if (Bg <= 0 || Bg > 65535 || chw <= 0 || chw % 4) return MMDYN_ERR_SHAPE;
  if (mask && (hw <= 0 || hw % 4 || chw % hw || (mask_channels != 1 && mask_channels != chw / hw))) return MMDYN_ERR_SHAPE;
  const dim3 grid(bce_rows_bpr(Bg, chw), Bg);
  if (mask)
    hipLaunchKernelGGL((bce_rows_groups_kernel<true, false>), grid, dim3(256), 0, ST, logits, target, mask, (float*)nullptr,
                       (const float*)nullptr, rows_out, unmasked_rows, gs, G, Bg, chw, hw, mask_channels, 0.f);
  else
    hipLaunchKernelGGL((bce_rows_groups_kernel<false, false>), grid, dim3(256), 0, ST, logits, target, mask, (float*)nullptr,
                       (const float*)nullptr, rows_out, (double*)nullptr, gs, G, Bg, chw, 0, 1, 0.f);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_bce_logits_rows_groups_grad(const float* logits, const float* target, const float* mask, int mask_channels,
                                                 float* dlogit, const float* w_rec, double* rows_out, double* unmasked_rows,
                                                 const int* slot_of_group, int n_slots, float grad_scale, int G, int Bg, int chw,
                                                 int hw, void* stream) {
  if (!logits || !target || !dlogit || !w_rec || !rows_out || !slot_of_group) return MMDYN_ERR_NULL;
  RowGroups gs{};
  if (int e = copy_slots(slot_of_group, G, n_slots, true, &gs)) return e;
  if (Bg <= 0 || Bg > 65535 || chw <= 0 || chw % 4) return MMDYN_ERR_SHAPE;
  if (mask && (hw <= 0 || hw % 4 || chw % hw || (mask_channels != 1 && mask_channels != chw / hw))) return MMDYN_ERR_SHAPE;
  if ((int64_t)G * Bg * chw >= (1LL << 31)) return MMDYN_ERR_RANGE;
  const dim3 grid(bce_rows_bpr(Bg, chw), Bg);
  if (mask)
    hipLaunchKernelGGL((bce_rows_groups_kernel<true, true>), grid, dim3(256), 0, ST, logits, target, mask, dlogit, w_rec,
                       rows_out, unmasked_rows, gs, G, Bg, chw, hw, mask_channels, grad_scale);
  else
    hipLaunchKernelGGL((bce_rows_groups_kernel<false, true>), grid, dim3(256), 0, ST, logits, target, mask, dlogit, w_rec,
                       rows_out, (double*)nullptr, gs, G, Bg, chw, 0, 1, grad_scale);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_mse_rows_groups(const float* r, const float* t, double* rows_out, const int* slot_of_group, int n_slots, int G,
                                     int Bg, int n, void* stream) {
  if (!r || !t || !rows_out || !slot_of_group) return MMDYN_ERR_NULL;
  RowGroups gs{};
  if (int e = copy_slots(slot_of_group, G, n_slots, false, &gs)) return e;
  if (Bg <= 0 || n <= 0 || (int64_t)G * Bg * n >= (1LL << 31)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(mse_rows_groups_kernel<false>, dim3(ew_grid((int64_t)G * Bg * 64)), dim3(256), 0, ST, r, t, (float*)nullptr,
                     (const float*)nullptr, rows_out, gs, G, Bg, n, 0.f);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_mse_rows_groups_grad(const float* r, const float* t, float* dr, const float* w_rec, double* rows_out,
                                          const int* slot_of_group, int n_slots, float grad_scale, int G, int Bg, int n,
                                          void* stream) {
  if (!r || !t || !dr || !w_rec || !rows_out || !slot_of_group) return MMDYN_ERR_NULL;
  RowGroups gs{};
  if (int e = copy_slots(slot_of_group, G, n_slots, false, &gs)) return e;
  if (Bg <= 0 || n <= 0) return MMDYN_ERR_SHAPE;
  if ((int64_t)G * Bg * n >= (1LL << 31)) return MMDYN_ERR_RANGE;
  hipLaunchKernelGGL(mse_rows_groups_kernel<true>, dim3(ew_grid((int64_t)G * Bg * 64)), dim3(256), 0, ST, r, t, dr, w_rec, rows_out,
                     gs, G, Bg, n, grad_scale);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble(const double* bce, const double* mse, const double* kl, float* loss,
                                   float* partials, int P, int B, float kl_weight, float pose_multiplier,
                                   const float* kl_weight_dev, void* stream) {
  if (!loss) return MMDYN_ERR_NULL;
  hipLaunchKernelGGL(elbo_assemble_kernel, dim3(1), dim3(64), 0, ST, bce, mse, kl, loss, partials, P, B,
                     kl_weight, pose_multiplier, kl_weight_dev);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble_rows(const double* bce_rows, const double* mse_rows, const double* kl_rows, const double* kl_sum,
                                        float* out, float* partials, int P, int B, float kl_weight, float pose_multiplier,
                                        const float* kl_weight_dev, int kl_mode, void* stream) {
  if (!out) return MMDYN_ERR_NULL;
  if (P <= 0 || B <= 0 || (kl_mode != 0 && kl_mode != 1)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(elbo_assemble_rows_kernel<false>, dim3(ew_grid(B)), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, kl_sum, out,
                     partials, (const uint32_t*)nullptr, TermModal{}, P, B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble_rows_avail(double* bce_rows, double* mse_rows, const double* kl_rows, const double* kl_sum,
                                              float* out, float* partials, const uint8_t* avail, const int* bce_modality,
                                              const int* mse_modality, int P, int B, float kl_weight, float pose_multiplier,
                                              const float* kl_weight_dev, int kl_mode, void* stream) {
  if (!out || !avail || !bce_modality || !mse_modality) return MMDYN_ERR_NULL;
  if (P <= 0 || P > MMDYN_MAX_PASSES || B <= 0 || (kl_mode != 0 && kl_mode != 1) || ((uintptr_t)avail & 3)) return MMDYN_ERR_SHAPE;
  TermModal tm{};
  for (int p = 0; p < P; ++p) {
    if (bce_modality[p] >= MMDYN_MAX_EXPERTS || mse_modality[p] >= MMDYN_MAX_EXPERTS) return MMDYN_ERR_SHAPE;
    tm.bce[p] = bce_modality[p];
    tm.mse[p] = mse_modality[p];
  }
  hipLaunchKernelGGL(elbo_assemble_rows_kernel<true>, dim3(ew_grid(B)), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, kl_sum, out,
                     partials, reinterpret_cast<const uint32_t*>(avail), tm, P, B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble_weighted(const double* bce_rows, const double* mse_rows, const double* kl_rows,
                                            const double* kl_sum, const float* w, float* loss, float* wpartials, float* out,
                                            float* partials, float* w_sum_out, int P, int B, float kl_weight, float pose_multiplier,
                                            const float* kl_weight_dev, int kl_mode, void* stream) {
  if (!w || !loss) return MMDYN_ERR_NULL;
  if (P <= 0 || P > MMDYN_MAX_PASSES || B <= 0 || (kl_mode != 0 && kl_mode != 1)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(elbo_assemble_weighted_kernel<false>, dim3(1), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, kl_sum, w, loss,
                     wpartials, out, partials, w_sum_out, (double*)nullptr, (const uint32_t*)nullptr, (double*)nullptr,
                     (double*)nullptr, P, B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble_avail_weighted(double* bce_v_rows, double* bce_t_rows, double* mse_rows, const double* kl_rows,
                                                  const double* kl_sum, const float* w, const uint8_t* tavail, float* loss,
                                                  float* wpartials, float* out, float* partials, float* w_sum_out, double* present,
                                                  double* term_sums, int P, int B, float kl_weight, float pose_multiplier,
                                                  const float* kl_weight_dev, int kl_mode, void* stream) {
  if (!loss) return MMDYN_ERR_NULL;
  if (P <= 0 || P > MMDYN_MAX_PASSES || B <= 0 || (kl_mode != 0 && kl_mode != 1) || ((uintptr_t)tavail & 3)) return MMDYN_ERR_SHAPE;
  if (bce_v_rows && bce_v_rows == bce_t_rows) return MMDYN_ERR_SHAPE;      // (one table per term: a shared one would count twice)
  hipLaunchKernelGGL(elbo_assemble_weighted_kernel<true>, dim3(1), dim3(256), 0, ST, bce_v_rows, mse_rows, kl_rows, kl_sum, w, loss,
                     wpartials, out, partials, w_sum_out, bce_t_rows, reinterpret_cast<const uint32_t*>(tavail), present, term_sums, P,
                     B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_term_weights(const uint8_t* tavail, const float* w, float* w_term, int B, void* stream) {
  if (!w_term) return MMDYN_ERR_NULL;
  if (B <= 0 || ((uintptr_t)tavail & 3)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(term_weights_kernel, dim3(ew_grid(B)), dim3(256), 0, ST, reinterpret_cast<const uint32_t*>(tavail), w, w_term, B);
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
