// Latent-space kernels of the cnn-mvae step (the reference's vae.py:311-318, 52-61, 126-165; problems.py:406, 429):
//   - product of experts + reparametrisation + KL, forward and backward, all P modality-subset passes in one launch.
//     Flags: AVAIL -- a per-row availability word: expert m takes part in row b iff the pass holds it AND avail[b][m] != 0, so one
//     batch holds every modality subset and row b is bitwise the result of a pass that holds row b's subset.  An absent
//     (row, expert) is never LOADED (a branch, not a multiplication by zero: its words may hold NaN / Inf) and the backward writes
//     exact zeros into its dmu / dlv.  With L % 64 == 0 a wavefront never spans two rows, so the per-expert branches are
//     wave-uniform.  WEIGHTED (backward) -- the KL scale of row b is kl_scale * w_kl[b] (the gradient of the weighted per-sample
//     ELBO, (1/B) sum_b w_b * row_b); dz arrives already weighted through the decoders and is not scaled again.  The flags only
//     add statements, so every instance evaluates the same expressions in the same order: all rows present, or w = 1
//     (x * 1.f == x), give the bits of the plain instance.  Both flags together are the backward of the training step on a mixed
//     batch (mmdyn_poe_bwd_avail_weighted).  With L % 64 != 0 a wavefront spans rows and the per-expert branches diverge: every
//     statement inside them is per-lane (no cross-lane operation sits in the row loop), so each lane follows its own row's word;
//   - reparametrisation alone (z = eps * exp(lv/2) + mu and/or KL), forward and backward (WEIGHTED as above);
//   - kl_rows: one KL value per SAMPLE (the reduce=False branch of problems.py:401-458), one wavefront per row;
//   - iw_latent: the K draws of the importance-weighted bound (Burda et al., "Importance Weighted Autoencoders") from ONE encoder
//     pass, z_k = eps_k * exp(lv / 2) + mu, and beside each draw its density ratio
//     ratio_k = log q(z_k|x) - log p(z_k) = sum_l 0.5 (z^2 - eps^2 - lv) (the 2 pi terms cancel; E_q[ratio] is the analytic KL)
//     in fp64 from the fp32 z the decoders will read.
// One fp32 element expression for z and for the KL term in all of them (fp64 sums), so the same (mu, lv, eps) give the same bits.
#include "common.h"

namespace {

// the passes by value; the AVAIL form adds their availability tables ([B] words; null = every row holds every expert of the pass)
template <bool AVAIL>
struct PoeArgs {
  mmdyn_pass_experts pass[MMDYN_MAX_PASSES];
};
template <>
struct PoeArgs<true> : PoeArgs<false> {
  const uint32_t* avail[MMDYN_MAX_PASSES];
};

template <bool AVAIL>
__global__ __launch_bounds__(256) void poe_fwd_kernel(PoeArgs<AVAIL> args, const float* __restrict__ eps_noise,
                                                      float* __restrict__ mu_out, float* __restrict__ lv_out,
                                                      float* __restrict__ z_out, double* __restrict__ kl_sum,
                                                      int with_prior, int B, int L) {
  const int p = blockIdx.y;
  const mmdyn_pass_experts& e = args.pass[p];
  const uint32_t* __restrict__ av = nullptr;
  if constexpr (AVAIL) av = args.avail[p];
  const int64_t n = (int64_t)B * L;
  double kl = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    uint32_t word = ALL_PRESENT;
    if constexpr (AVAIL) word = av ? av[b] : ALL_PRESENT;
    // universal prior expert N(0, 1) first, then the modalities the pass (AVAIL: this ROW) holds, in the reference's order
    float var0 = 1.f + POE_EPS;
    float sumT = with_prior ? 1.f / (var0 + POE_EPS) : 0.f, sumMuT = 0.f;
#pragma unroll
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m) {
      if (e.mu[m] && (!AVAIL || has(word, m))) {
        float mu_m = e.mu[m][(size_t)b * e.ld[m] + l];
        float lv_m = e.lv[m][(size_t)b * e.ld[m] + l];
        float var = expf(lv_m) + POE_EPS;
        float Tm = 1.f / (var + POE_EPS);
        sumT += Tm;
        sumMuT += mu_m * Tm;
      }
    }
    float pd_mu = sumMuT / sumT;
    float pd_var = 1.f / sumT;
    float pd_lv = logf(pd_var + POE_EPS);
    const size_t o = (size_t)p * n + i;
    mu_out[o] = pd_mu;
    lv_out[o] = pd_lv;
    if (z_out) {
      const float zv = eps_noise[o] * expf(0.5f * pd_lv) + pd_mu;
      z_out[o] = zv;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (e.zdst[k]) e.zdst[k][i] = zv;
        if (e.zpl[k]) {                  // ... and as a plane row block: hi | mid | lo of the exact three-term split
          uint32_t h, m, lo;
          split3_bf16(zv, 0.f, h, m, lo);
          bf16_t* pr = reinterpret_cast<bf16_t*>(e.zpl[k]) + (size_t)b * 3 * L + l;
          pr[0] = (bf16_t)(h & 0xffffu);
          pr[L] = (bf16_t)(m & 0xffffu);
          pr[2 * L] = (bf16_t)(lo & 0xffffu);
        }
      }
    }
    kl += (double)(1.f + pd_lv - pd_mu * pd_mu - expf(pd_lv));
  }
  if (kl_sum) block_atomic_add(kl, &kl_sum[p], -0.5);
}

template <bool AVAIL, bool WEIGHTED>
__global__ __launch_bounds__(256) void poe_bwd_kernel(PoeArgs<AVAIL> args, const float* __restrict__ eps_noise,
                                                      const float* __restrict__ mu_pd,
                                                      const float* __restrict__ lv_pd,
                                                      const float* __restrict__ dz,
                                                      const float* __restrict__ g_mu,
                                                      const float* __restrict__ g_lv, float kl_scale_arg,
                                                      const float* __restrict__ kl_weight_dev,
                                                      const float* __restrict__ w_kl, int with_prior, int B, int L) {
  // kl_weight_dev (optional): the KL weight lives in device memory and multiplies kl_scale -- a captured launch then
  // follows the annealing schedule (problems.py:212-216) without being re-captured
  const float kl_scale0 = kl_weight_dev ? kl_scale_arg * kl_weight_dev[0] : kl_scale_arg;
  const int p = blockIdx.y;
  const mmdyn_pass_experts& e = args.pass[p];
  const uint32_t* __restrict__ av = nullptr;
  if constexpr (AVAIL) av = args.avail[p];
  const int64_t n = (int64_t)B * L;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    uint32_t word = ALL_PRESENT;
    if constexpr (AVAIL) word = av ? av[b] : ALL_PRESENT;
    float kl_scale = kl_scale0;
    if constexpr (WEIGHTED) kl_scale = kl_scale0 * w_kl[b];
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
    // z = eps * exp(lv/2) + mu ;  KL = -0.5 * sum(1 + lv - mu^2 - exp(lv))
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
      if (e.mu[m] && (!AVAIL || has(word, m))) {
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
        if (!AVAIL || has(word, m)) {
          const float dT = dS + dN * mum[m];
          e.dmu[m][(size_t)b * e.ld[m] + l] = dN * Tm[m];
          e.dlv[m][(size_t)b * e.ld[m] + l] = -dT * Tm[m] * Tm[m] * ex[m];
        } else {                         // the expert did not take part in this row: a defined zero, whatever the buffer held
          e.dmu[m][(size_t)b * e.ld[m] + l] = 0.f;
          e.dlv[m][(size_t)b * e.ld[m] + l] = 0.f;
        }
      }
    }
  }
}

// z = eps * exp(lv/2) + mu and/or KL(mu, lv); mu/lv rows of stride ld (vae.py:57-59, problems.py:406)
__global__ __launch_bounds__(256) void reparam_fwd_kernel(const float* __restrict__ mu,
                                                          const float* __restrict__ lv,
                                                          const float* __restrict__ eps_noise,
                                                          float* __restrict__ z, double* __restrict__ kl_sum,
                                                          int B, int L, int ld) {
  const int64_t n = (int64_t)B * L;
  double kl = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    const float m = mu[(size_t)b * ld + l], v = lv[(size_t)b * ld + l];
    if (z) z[i] = eps_noise[i] * expf(0.5f * v) + m;
    kl += (double)(1.f + v - m * m - expf(v));
  }
  if (kl_sum) block_atomic_add(kl, kl_sum, -0.5);
}

// (launch bounds: the plain instance has always been compiled for the default 1024 threads, the WEIGHTED one for the 256 it gets)
template <bool WEIGHTED>
__global__ __launch_bounds__(WEIGHTED ? 256 : 1024) void reparam_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                            const float* __restrict__ eps_noise,
                                                                            const float* __restrict__ dz, float kl_scale_arg,
                                                                            const float* __restrict__ w_kl, float* __restrict__ dmu,
                                                                            float* __restrict__ dlv, int B, int L, int ld) {
  const int64_t n = (int64_t)B * L;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    float kl_scale = kl_scale_arg;
    if constexpr (WEIGHTED) kl_scale = kl_scale_arg * w_kl[b];
    const float m = mu[(size_t)b * ld + l], v = lv[(size_t)b * ld + l];
    const float g = dz ? dz[i] : 0.f;
    float gm = g + kl_scale * m;
    float gv = -0.5f * kl_scale * (1.f - expf(v));
    if (dz) gv += g * eps_noise[i] * 0.5f * expf(0.5f * v);
    dmu[(size_t)b * ld + l] = gm;
    dlv[(size_t)b * ld + l] = gv;
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

// row = k * B + b of the [K][B] tables; eps / z rows of L floats, mu / lv rows of stride ld.  One wavefront per row, 16-byte lane
// accesses (VEC), a fixed-order fp64 reduction (lane-local in l order, then the xor butterfly): no atomics, the same bits in every run
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

// The pass table of a PoE launch, by value, checked in the order the entry points report: no table -> NULL; P out of range, a
// refused B x L (rows_ok: the entry points differ in whether they look) or a bad availability table -> SHAPE; then an expert
// without its partner pointers, or (backward) a dz without the noise -> NULL.  A table needs with_prior (a row may hold no expert
// at all: without the prior it would divide by zero, and finding such a row needs the table's contents) and 4-byte alignment.
template <bool AVAIL>
int copy_passes(const mmdyn_pass_experts* passes, const uint8_t* const* avail, int with_prior, int P, bool rows_ok, bool backward,
                const float* eps_noise, PoeArgs<AVAIL>* out) {
  if (!passes) return MMDYN_ERR_NULL;
  if (P < 1 || P > MMDYN_MAX_PASSES || !rows_ok) return MMDYN_ERR_SHAPE;
  for (int p = 0; p < P; ++p) {
    out->pass[p] = passes[p];
    if constexpr (AVAIL) {
      const uint8_t* t = avail ? avail[p] : nullptr;
      if (t && (!with_prior || ((uintptr_t)t & 3))) return MMDYN_ERR_SHAPE;
      out->avail[p] = reinterpret_cast<const uint32_t*>(t);
    }
  }
  for (int p = 0; p < P; ++p) {
    const mmdyn_pass_experts& e = out->pass[p];
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m)
      if (backward ? e.mu[m] && (!e.lv[m] || !e.dmu[m] || !e.dlv[m]) : (e.mu[m] != nullptr) != (e.lv[m] != nullptr))
        return MMDYN_ERR_NULL;
    for (int k = 0; k < 3; ++k)
      if (backward && e.dz[k] && !eps_noise) return MMDYN_ERR_NULL;
  }
  return MMDYN_OK;
}

// blocks along x of the launches that walk B x L elements once per pass: 64 at the most
int latent_gx(int B, int L) {
  const int gx = ew_grid((int64_t)B * L);
  return gx > 64 ? 64 : gx;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mmdyn_poe_fwd(const mmdyn_pass_experts* passes, const float* eps_noise, float* mu,
                             float* logvar, float* z, double* kl_sum, int with_prior, int P, int B, int L,
                             void* stream) {
  if (!mu || !logvar || (z && !eps_noise)) return MMDYN_ERR_NULL;
  PoeArgs<false> a{};
  if (int e = copy_passes(passes, nullptr, with_prior, P, true, false, eps_noise, &a)) return e;
  hipLaunchKernelGGL(poe_fwd_kernel<false>, dim3(latent_gx(B, L), P), dim3(256), 0, ST, a, eps_noise, mu, logvar, z, kl_sum,
                     with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

/* avail == null, or a null table: every row holds every expert of the pass (still the AVAIL instance) */
extern "C" int mmdyn_poe_fwd_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise, float* mu,
                                   float* logvar, float* z, double* kl_sum, int with_prior, int P, int B, int L, void* stream) {
  if (!mu || !logvar || (z && !eps_noise)) return MMDYN_ERR_NULL;
  PoeArgs<true> a{};
  if (int e = copy_passes(passes, avail, with_prior, P, B > 0 && L > 0, false, eps_noise, &a)) return e;
  hipLaunchKernelGGL(poe_fwd_kernel<true>, dim3(latent_gx(B, L), P), dim3(256), 0, ST, a, eps_noise, mu, logvar, z, kl_sum,
                     with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_poe_bwd(const mmdyn_pass_experts* passes, const float* eps_noise, const float* mu,
                             const float* logvar, const float* dz, const float* g_mu, const float* g_lv,
                             float kl_scale, int with_prior, int P, int B, int L, const float* kl_weight_dev,
                             void* stream) {
  if (!mu || !logvar || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  PoeArgs<false> a{};
  if (int e = copy_passes(passes, nullptr, with_prior, P, true, true, eps_noise, &a)) return e;
  hipLaunchKernelGGL((poe_bwd_kernel<false, false>), dim3(latent_gx(B, L), P), dim3(256), 0, ST, a, eps_noise, mu, logvar, dz, g_mu,
                     g_lv, kl_scale, kl_weight_dev, (const float*)nullptr, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_poe_bwd_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise,
                                   const float* mu, const float* logvar, const float* dz, const float* g_mu, const float* g_lv,
                                   float kl_scale, int with_prior, int P, int B, int L, const float* kl_weight_dev, void* stream) {
  if (!mu || !logvar || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  PoeArgs<true> a{};
  if (int e = copy_passes(passes, avail, with_prior, P, B > 0 && L > 0, true, eps_noise, &a)) return e;
  hipLaunchKernelGGL((poe_bwd_kernel<true, false>), dim3(latent_gx(B, L), P), dim3(256), 0, ST, a, eps_noise, mu, logvar, dz, g_mu,
                     g_lv, kl_scale, kl_weight_dev, (const float*)nullptr, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_poe_bwd_weighted(const mmdyn_pass_experts* passes, const float* eps_noise, const float* mu, const float* logvar,
                                      const float* dz, const float* g_mu, const float* g_lv, float kl_scale, const float* w_kl,
                                      int with_prior, int P, int B, int L, const float* kl_weight_dev, void* stream) {
  if (!mu || !logvar || !w_kl || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  PoeArgs<false> a{};
  if (int e = copy_passes(passes, nullptr, with_prior, P, B > 0 && L > 0, true, eps_noise, &a)) return e;
  hipLaunchKernelGGL((poe_bwd_kernel<false, true>), dim3(latent_gx(B, L), P), dim3(256), 0, ST, a, eps_noise, mu, logvar, dz, g_mu,
                     g_lv, kl_scale, kl_weight_dev, w_kl, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

/* both flags: the tables of mmdyn_poe_bwd_avail and the row weights of mmdyn_poe_bwd_weighted (the training step on a mixed batch) */
extern "C" int mmdyn_poe_bwd_avail_weighted(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise,
                                            const float* mu, const float* logvar, const float* dz, const float* g_mu,
                                            const float* g_lv, float kl_scale, const float* w_kl, int with_prior, int P, int B, int L,
                                            const float* kl_weight_dev, void* stream) {
  if (!mu || !logvar || !w_kl || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  PoeArgs<true> a{};
  if (int e = copy_passes(passes, avail, with_prior, P, B > 0 && L > 0, true, eps_noise, &a)) return e;
  hipLaunchKernelGGL((poe_bwd_kernel<true, true>), dim3(latent_gx(B, L), P), dim3(256), 0, ST, a, eps_noise, mu, logvar, dz, g_mu,
                     g_lv, kl_scale, kl_weight_dev, w_kl, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_reparam_fwd(const float* mu, const float* lv, const float* eps_noise, float* z,
                                 double* kl_sum, int B, int L, int ld, void* stream) {
  if (!mu || !lv || (z && !eps_noise)) return MMDYN_ERR_NULL;
  if (ld < L) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(reparam_fwd_kernel, dim3(latent_gx(B, L)), dim3(256), 0, ST, mu, lv, eps_noise, z, kl_sum, B, L, ld);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_reparam_bwd(const float* mu, const float* lv, const float* eps_noise, const float* dz,
                                 float kl_scale, float* dmu, float* dlv, int B, int L, int ld, void* stream) {
  if (!mu || !lv || !dmu || !dlv || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  if (ld < L) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(reparam_bwd_kernel<false>, dim3(ew_grid((int64_t)B * L)), dim3(256), 0, ST, mu, lv, eps_noise,
                     dz, kl_scale, (const float*)nullptr, dmu, dlv, B, L, ld);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_reparam_bwd_weighted(const float* mu, const float* lv, const float* eps_noise, const float* dz, float kl_scale,
                                          const float* w_kl, float* dmu, float* dlv, int B, int L, int ld, void* stream) {
  if (!mu || !lv || !w_kl || !dmu || !dlv || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  if (B <= 0 || L <= 0 || ld < L) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(reparam_bwd_kernel<true>, dim3(ew_grid((int64_t)B * L)), dim3(256), 0, ST, mu, lv, eps_noise, dz, kl_scale,
                     w_kl, dmu, dlv, B, L, ld);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_kl_rows(const float* mu, const float* logvar, double* kl_rows, int P, int B, int L, void* stream) {
  if (!mu || !logvar || !kl_rows) return MMDYN_ERR_NULL;
  if (P <= 0 || B <= 0 || L <= 0 || (int64_t)P * B * L >= (1LL << 31)) return MMDYN_ERR_SHAPE;
  hipLaunchKernelGGL(kl_rows_kernel, dim3(ew_grid((int64_t)P * B * 64)), dim3(256), 0, ST, mu, logvar, kl_rows, P * B, L);
  MMDYN_LAUNCH_CHECK();
}

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
