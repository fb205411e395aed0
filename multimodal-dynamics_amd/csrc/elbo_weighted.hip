// Gradients of the WEIGHTED per-sample ELBO: L = (1/B) sum_b w_b * row_b (the reference's (w * rows).sum() / B on the reduce=False
// branch of problems.py:415-417, 451-456, or the same with each sample's own KL).  Every backward chain of the step starts from one
// of three seeds -- the BCE gradient, the MSE gradient, the KL term of the latent backward -- and each took ONE scalar scale; here the
// scale is a vector indexed by the sample:
//   - BCE-with-logits rows of G passes against one target WITH dlogit = ((sigmoid - t) * grad_scale) * w[b] (the twin of the last
//     decoder layer's weighted epilogue, tconv_out3.hip): bce_rows_groups_kernel of elbo_rows.hip plus the store;
//   - MSE rows with dr = (2 (r - t) * grad_scale) * w[b];
//   - poe_bwd_kernel / reparam_bwd_kernel of latent_elbo.hip with kl_scale * w_kl[b] in place of kl_scale;
//   - the assembly: the weighted scalar and its per-pass partials from the fp64 row tables, with the unweighted rows / partials of
//     elbo_assemble_rows_kernel, and the [B] vector of sum_b w_b that the reference's KL mode hands to the latent backward.
// The scale products are written in that order so that w = 1 reproduces the unweighted kernels' gradients bit for bit (x * 1.f == x).
// The sums are NOT weighted: the row tables are those of elbo_rows.hip.  Weights are not inspected: NaN / Inf propagate.
#include "common.h"

namespace {

struct RowGroups {
  int slot[MMDYN_BCE_GROUPS_MAX];
};

template <bool MASKED>
__global__ __launch_bounds__(256) void bce_rows_groups_grad_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                   const float* __restrict__ mask, float* __restrict__ dlogit,
                                                                   const float* __restrict__ w_rec, double* __restrict__ rows,
                                                                   double* __restrict__ unmasked, const RowGroups gs, int G, int Bg,
                                                                   int chw, int hw, int mask_c, float grad_scale) {
  constexpr int GM = MMDYN_BCE_GROUPS_MAX;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int chw4 = chw >> 2;
  const float* __restrict__ tg = target + (size_t)b * chw;
  const float wr = w_rec[b];                       // (block-uniform: a block owns a piece of ONE sample's row)
  double acc[GM], acc_u[MASKED ? GM : 1];
#pragma unroll
  for (int g = 0; g < GM; ++g) {
    acc[g] = 0.0;
    if constexpr (MASKED) acc_u[g] = 0.0;
  }
  for (int i = blockIdx.x * 256 + tid; i < chw4; i += gridDim.x * 256) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(tg + 4 * (size_t)i);
    f32x4 mk = {1.f, 1.f, 1.f, 1.f};
    if constexpr (MASKED) {
      const int e0 = 4 * i, ch = e0 / hw, pix = e0 - ch * hw;
      mk = *reinterpret_cast<const f32x4*>(mask + ((size_t)b * mask_c + (mask_c == 1 ? 0 : ch)) * hw + pix);
    }
#pragma unroll
    for (int g = 0; g < GM; ++g) {
      if (g < G) {                                 // (block-uniform)
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
              d[k] = (mk[k] * (sg - tm) * grad_scale) * wr;
            }
            acc_u[g] += (double)part_u;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              float l, sg;
              bce_elem(xv[k], t[k], l, sg);
              part += l;
              d[k] = ((sg - t[k]) * grad_scale) * wr;
            }
          }
          acc[g] += (double)part;
        }
        *reinterpret_cast<f32x4*>(dlogit + o) = d;
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
  if (tid < G && gs.slot[tid] >= 0) {
    const size_t o = (size_t)gs.slot[tid] * Bg + b;
    atomicAdd(rows + o, red[0][tid][0] + red[0][tid][1] + red[0][tid][2] + red[0][tid][3]);
    if (with_u) atomicAdd(unmasked + o, red[1][tid][0] + red[1][tid][1] + red[1][tid][2] + red[1][tid][3]);
  }
}

// one wavefront per (g, b): rows[slot[g]][b] += sum_n (r - t)^2, dr = (2 (r - t) * grad_scale) * w[b]
__global__ __launch_bounds__(256) void mse_rows_groups_grad_kernel(const float* __restrict__ r, const float* __restrict__ t,
                                                                   float* __restrict__ dr, const float* __restrict__ w_rec,
                                                                   double* __restrict__ rows, const RowGroups gs, int G, int Bg, int n,
                                                                   float grad_scale) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
  for (int row = wave; row < G * Bg; row += nwaves) {
    const int g = row / Bg, b = row - g * Bg;
    const float wr = w_rec[b];
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) {
      const float d = r[(size_t)row * n + k] - t[(size_t)b * n + k];
      acc += (double)(d * d);
      dr[(size_t)row * n + k] = (2.f * d * grad_scale) * wr;
    }
    acc = wave_sum_d(acc);
    if (lane == 0) atomicAdd(rows + (size_t)gs.slot[g] * Bg + b, acc);
  }
}

struct PoeArgs {
  mmdyn_pass_experts pass[MMDYN_MAX_PASSES];
};

constexpr float POE_EPS = 1e-8f;

// poe_bwd_kernel (latent_elbo.hip) with the KL scale of row b multiplied by w_kl[b]; everything else -- expressions, order, the
// zero-dz shortcuts -- as there.  dz arrives already weighted through the decoders and is not scaled again.
__global__ __launch_bounds__(256) void poe_bwd_weighted_kernel(PoeArgs args, const float* __restrict__ eps_noise,
                                                               const float* __restrict__ mu_pd, const float* __restrict__ lv_pd,
                                                               const float* __restrict__ dz, const float* __restrict__ g_mu,
                                                               const float* __restrict__ g_lv, float kl_scale_arg,
                                                               const float* __restrict__ kl_weight_dev,
                                                               const float* __restrict__ w_kl, int with_prior, int B, int L) {
  const float kl_scale0 = kl_weight_dev ? kl_scale_arg * kl_weight_dev[0] : kl_scale_arg;
  const int p = blockIdx.y;
  const mmdyn_pass_experts& e = args.pass[p];
  const int64_t n = (int64_t)B * L;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    const float kl_scale = kl_scale0 * w_kl[b];
    const size_t o = (size_t)p * n + i;
    const float mu = mu_pd[o], lv = lv_pd[o];
    float g = dz ? dz[o] : 0.f;
    bool any_dz = dz != nullptr;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (e.dz[k]) {
        g += e.dz[k][i];
        any_dz = true;
      }
    float dmu_pd = g + kl_scale * mu;
    float dlv_pd = -0.5f * kl_scale * (1.f - expf(lv));
    if (any_dz) dlv_pd += g * eps_noise[o] * 0.5f * expf(0.5f * lv);
    if (g_mu) dmu_pd += g_mu[o];
    if (g_lv) dlv_pd += g_lv[o];
    float Tm[MMDYN_MAX_EXPERTS], mum[MMDYN_MAX_EXPERTS], ex[MMDYN_MAX_EXPERTS];
    float var0 = 1.f + POE_EPS;
    float S = with_prior ? 1.f / (var0 + POE_EPS) : 0.f, N = 0.f;
#pragma unroll
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m) {
      Tm[m] = 0.f;
      mum[m] = 0.f;
      ex[m] = 0.f;
      if (e.mu[m]) {
        mum[m] = e.mu[m][(size_t)b * e.ld[m] + l];
        ex[m] = expf(e.lv[m][(size_t)b * e.ld[m] + l]);
        Tm[m] = 1.f / (ex[m] + POE_EPS + POE_EPS);
        S += Tm[m];
        N += mum[m] * Tm[m];
      }
    }
    const float pd_var = 1.f / S;
    const float dvar = dlv_pd / (pd_var + POE_EPS);
    const float invS2 = pd_var * pd_var;
    const float dS = -dvar * invS2 - dmu_pd * N * invS2;
    const float dN = dmu_pd * pd_var;
#pragma unroll
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m) {
      if (e.mu[m]) {
        const float dT = dS + dN * mum[m];
        e.dmu[m][(size_t)b * e.ld[m] + l] = dN * Tm[m];
        e.dlv[m][(size_t)b * e.ld[m] + l] = -dT * Tm[m] * Tm[m] * ex[m];
      }
    }
  }
}

// reparam_bwd_kernel (latent_elbo.hip) with kl_scale * w_kl[b]
__global__ __launch_bounds__(256) void reparam_bwd_weighted_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                   const float* __restrict__ eps_noise, const float* __restrict__ dz,
                                                                   float kl_scale_arg, const float* __restrict__ w_kl,
                                                                   float* __restrict__ dmu, float* __restrict__ dlv, int B, int L,
                                                                   int ld) {
  const int64_t n = (int64_t)B * L;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    const float kl_scale = kl_scale_arg * w_kl[b];
    const float m = mu[(size_t)b * ld + l], v = lv[(size_t)b * ld + l];
    const float g = dz ? dz[i] : 0.f;
    float gm = g + kl_scale * m;
    float gv = -0.5f * kl_scale * (1.f - expf(v));
    if (dz) gv += g * eps_noise[i] * 0.5f * expf(0.5f * v);
    dmu[(size_t)b * ld + l] = gm;
    dlv[(size_t)b * ld + l] = gv;
  }
}

// ONE block.  Thread t owns the samples t, t + 256, ...: it writes their unweighted rows / partials (elbo_assemble_rows_kernel's
// expression) and adds w_b * term into its own fp64 sums in increasing b; the 256 sums of a quantity are then added by the fixed
// shuffle tree of wave_sum_d and the four wave totals in wave order -- no atomics, the same order in every run.
//   S[p]  = sum_b w_b * (bce[p][b] + pose_multiplier * mse[p][b]),  K[p] = sum_b w_b * kl_rows[p][b],  W = sum_b w_b
//   wpartials[p] = (S[p] + kl_weight * (kl_mode ? K[p] : W * kl_sum[p])) / B,  loss = sum_p wpartials[p]
__global__ __launch_bounds__(256) void elbo_assemble_weighted_kernel(const double* __restrict__ bce, const double* __restrict__ mse,
                                                                     const double* __restrict__ kl_rows,
                                                                     const double* __restrict__ kl_sum, const float* __restrict__ w,
                                                                     float* __restrict__ loss, float* __restrict__ wpartials,
                                                                     float* __restrict__ out, float* __restrict__ partials,
                                                                     float* __restrict__ w_sum_out, int P, int B, float kl_weight_arg,
                                                                     float pose_multiplier, const float* __restrict__ kl_weight_dev,
                                                                     int kl_mode) {
  constexpr int PM = MMDYN_MAX_PASSES;
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  const int tid = threadIdx.x;
  double S[PM], K[PM], W = 0.0;
#pragma unroll
  for (int p = 0; p < PM; ++p) S[p] = K[p] = 0.0;
  for (int b = tid; b < B; b += 256) {
    const double wb = (double)w[b];
    W += wb;
    double tot = 0.0;
#pragma unroll
    for (int p = 0; p < PM; ++p) {
      if (p < P) {
        const size_t o = (size_t)p * B + b;
        const double rec = (bce ? bce[o] : 0.0) + (double)pose_multiplier * (mse ? mse[o] : 0.0);
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
  __shared__ double red[2 * PM + 1][4];
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
  if (w_sum_out)
    for (int b = tid; b < B; b += 256) w_sum_out[b] = (float)Wt;
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
  int bpr = ceil_div(1024, Bg);
  const int most = ceil_div(chw / 4, 256);
  if (bpr > most) bpr = most;
  if (mask)
    hipLaunchKernelGGL(bce_rows_groups_grad_kernel<true>, dim3(bpr, Bg), dim3(256), 0, ST, logits, target, mask, dlogit, w_rec,
                       rows_out, unmasked_rows, gs, G, Bg, chw, hw, mask_channels, grad_scale);
  else
    hipLaunchKernelGGL(bce_rows_groups_grad_kernel<false>, dim3(bpr, Bg), dim3(256), 0, ST, logits, target, mask, dlogit, w_rec,
                       rows_out, (double*)nullptr, gs, G, Bg, chw, 0, 1, grad_scale);
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
  hipLaunchKernelGGL(mse_rows_groups_grad_kernel, dim3(ew_grid((int64_t)G * Bg * 64)), dim3(256), 0, ST, r, t, dr, w_rec, rows_out, gs,
                     G, Bg, n, grad_scale);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_poe_bwd_weighted(const mmdyn_pass_experts* passes, const float* eps_noise, const float* mu, const float* logvar,
                                      const float* dz, const float* g_mu, const float* g_lv, float kl_scale, const float* w_kl,
                                      int with_prior, int P, int B, int L, const float* kl_weight_dev, void* stream) {
  if (!passes || !mu || !logvar || !w_kl || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  if (P < 1 || P > MMDYN_MAX_PASSES || B <= 0 || L <= 0) return MMDYN_ERR_SHAPE;
  PoeArgs a{};
  for (int p = 0; p < P; ++p) {
    a.pass[p] = passes[p];
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m)
      if (a.pass[p].mu[m] && (!a.pass[p].lv[m] || !a.pass[p].dmu[m] || !a.pass[p].dlv[m])) return MMDYN_ERR_NULL;
    for (int k = 0; k < 3; ++k)
      if (a.pass[p].dz[k] && !eps_noise) return MMDYN_ERR_NULL;
  }
  int gx = ew_grid((int64_t)B * L);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(poe_bwd_weighted_kernel, dim3(gx, P), dim3(256), 0, ST, a, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale,
                     kl_weight_dev, w_kl, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_reparam_bwd_weighted(const float* mu, const float* lv, const float* eps_noise, const float* dz, float kl_scale,
                                          const float* w_kl, float* dmu, float* dlv, int B, int L, int ld, void* stream) {
  if (!mu || !lv || !w_kl || !dmu || !dlv || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  if (B <= 0 || L <= 0 || ld < L) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(reparam_bwd_weighted_kernel, dim3(ew_grid((int64_t)B * L)), dim3(256), 0, ST, mu, lv, eps_noise, dz, kl_scale,
                     w_kl, dmu, dlv, B, L, ld);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_elbo_assemble_weighted(const double* bce_rows, const double* mse_rows, const double* kl_rows,
                                            const double* kl_sum, const float* w, float* loss, float* wpartials, float* out,
                                            float* partials, float* w_sum_out, int P, int B, float kl_weight, float pose_multiplier,
                                            const float* kl_weight_dev, int kl_mode, void* stream) {
  if (!w || !loss) return MMDYN_ERR_NULL;
  if (P <= 0 || P > MMDYN_MAX_PASSES || B <= 0 || (kl_mode != 0 && kl_mode != 1)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(elbo_assemble_weighted_kernel, dim3(1), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, kl_sum, w, loss, wpartials,
                     out, partials, w_sum_out, P, B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}
