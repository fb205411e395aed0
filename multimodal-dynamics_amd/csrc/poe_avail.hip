// Mixed-modality batches: the modalities of a request differ from ROW TO ROW (the dataset's per-frame availability vector,
// utils/datasets.py: a frame whose image is constant counts as missing).  The reference runs MVAE.forward (vae.py:126-165) once per
// modality subset; here one batch holds every subset:
//   - product of experts + reparametrisation + KL, forward and backward, with a per-row availability word: expert m takes part
//     in row b iff the pass holds it AND avail[b][m] != 0.  The arithmetic and its order are those of poe_fwd_kernel /
//     poe_bwd_kernel (latent_elbo.hip) statement for statement, so row b is bitwise the result of a pass that holds row b's
//     subset.  An absent (row, expert) is never LOADED (a branch, not a multiplication by zero): its words may hold NaN / Inf.
//     The backward writes exact zeros into the dmu / dlv rows of an absent (row, expert).
//   - the completion select: out[b] = avail[b][m] ? x[b] : (logits ? sigmoid(recon[b]) : recon[b]), 16-byte accesses;
//   - the per-sample ELBO assembly with a target-availability word per row: a (row, term) whose target is absent is written as 0
//     into its table and left out of the row sum.
// The availability table is uint8 [B][MMDYN_MAX_EXPERTS], read as ONE 32-bit word per row (byte m = expert m, little endian);
// with L % 64 == 0 a wavefront never spans two rows, so the per-expert branches are wave-uniform.
// The kernels are separate from those of latent_elbo.hip / elbo_rows.hip (not a template parameter of them): the existing
// instantiations keep their code, registers and arguments untouched.
#include "common.h"

namespace {

struct PoeAvailArgs {
  mmdyn_pass_experts pass[MMDYN_MAX_PASSES];
  const uint32_t* avail[MMDYN_MAX_PASSES];          // [B] words; null = every row holds every expert of the pass
};

constexpr float POE_EPS = 1e-8f;
constexpr uint32_t ALL_PRESENT = 0x01010101u;

__device__ __forceinline__ bool has(uint32_t word, int m) { return ((word >> (8 * m)) & 0xffu) != 0u; }

__global__ __launch_bounds__(256) void poe_fwd_avail_kernel(PoeAvailArgs args, const float* __restrict__ eps_noise,
                                                            float* __restrict__ mu_out, float* __restrict__ lv_out,
                                                            float* __restrict__ z_out, double* __restrict__ kl_sum, int with_prior,
                                                            int B, int L) {
  const int p = blockIdx.y;
  const mmdyn_pass_experts& e = args.pass[p];
  const uint32_t* __restrict__ av = args.avail[p];
  const int64_t n = (int64_t)B * L;
  double kl = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    const uint32_t word = av ? av[b] : ALL_PRESENT;
    // universal prior expert N(0, 1) first, then the modalities this ROW holds, in the reference's order
    float var0 = 1.f + POE_EPS;
    float sumT = with_prior ? 1.f / (var0 + POE_EPS) : 0.f, sumMuT = 0.f;
#pragma unroll
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m) {
      if (e.mu[m] && has(word, m)) {
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
  if (kl_sum) {
    kl = wave_sum_d(kl);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kl;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&kl_sum[p], -0.5 * (red[0] + red[1] + red[2] + red[3]));
  }
}

__global__ __launch_bounds__(256) void poe_bwd_avail_kernel(PoeAvailArgs args, const float* __restrict__ eps_noise,
                                                            const float* __restrict__ mu_pd, const float* __restrict__ lv_pd,
                                                            const float* __restrict__ dz, const float* __restrict__ g_mu,
                                                            const float* __restrict__ g_lv, float kl_scale_arg,
                                                            const float* __restrict__ kl_weight_dev, int with_prior, int B, int L) {
  const float kl_scale = kl_weight_dev ? kl_scale_arg * kl_weight_dev[0] : kl_scale_arg;
  const int p = blockIdx.y;
  const mmdyn_pass_experts& e = args.pass[p];
  const uint32_t* __restrict__ av = args.avail[p];
  const int64_t n = (int64_t)B * L;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
    const uint32_t word = av ? av[b] : ALL_PRESENT;
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
      if (e.mu[m] && has(word, m)) {
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
        if (has(word, m)) {
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

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

// out [B][row_len] as one flat array of n = B * row_len floats: quads [0, n4) by 16-byte accesses (n4 = 0 when a pointer is not
// 16-byte aligned), the elements from 4 * n4 on one by one.  A quad inside ONE row reads only the side it takes; a quad that
// straddles rows (row_len % 4 != 0: the 7-DoF pose) reads both and selects per element.  x == null: no row is present.
__global__ __launch_bounds__(256) void complete_select_kernel(const float* __restrict__ x, const float* __restrict__ recon,
                                                              const uint32_t* __restrict__ avail, int modality,
                                                              float* __restrict__ out, int64_t n, int64_t n4, int row_len,
                                                              int logits) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = tid; q < n4; q += nthreads) {
    const int64_t e0 = 4 * q;
    const int b0 = (int)(e0 / row_len), b3 = (int)((e0 + 3) / row_len);
    f32x4 v;
    if (b0 == b3) {
      const bool present = x != nullptr && (!avail || has(avail[b0], modality));
      if (present) {
        v = *reinterpret_cast<const f32x4*>(x + e0);
      } else {
        v = *reinterpret_cast<const f32x4*>(recon + e0);
        if (logits) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = sigmoid_f(v[k]);
        }
      }
    } else {
      const f32x4 r = *reinterpret_cast<const f32x4*>(recon + e0);
      f32x4 xv = r;
      if (x) xv = *reinterpret_cast<const f32x4*>(x + e0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = (int)((e0 + k) / row_len);
        const bool present = x != nullptr && (!avail || has(avail[b], modality));
        v[k] = present ? xv[k] : (logits ? sigmoid_f(r[k]) : r[k]);
      }
    }
    *reinterpret_cast<f32x4*>(out + e0) = v;
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nthreads) {
    const int b = (int)(i / row_len);
    const bool present = x != nullptr && (!avail || has(avail[b], modality));
    float v;
    if (present) {
      v = x[i];
    } else {
      v = recon[i];
      if (logits) v = sigmoid_f(v);
    }
    out[i] = v;
  }
}

struct TermModal {
  int bce[MMDYN_MAX_PASSES], mse[MMDYN_MAX_PASSES];
};

// elbo_assemble_rows_kernel (elbo_rows.hip) with a target-availability word per row: slot p of the bce / mse table belongs to the
// target modality tm.bce[p] / tm.mse[p] (negative: the slot has no target modality and always counts).  An excluded entry is
// selected out of the sum (it may hold anything) and written back as 0.
__global__ void elbo_assemble_rows_avail_kernel(double* __restrict__ bce, double* __restrict__ mse, const double* __restrict__ kl_rows,
                                                const double* __restrict__ kl_sum, float* __restrict__ out,
                                                float* __restrict__ partials, const uint32_t* __restrict__ avail, const TermModal tm,
                                                int P, int B, float kl_weight_arg, float pose_multiplier,
                                                const float* __restrict__ kl_weight_dev, int kl_mode) {
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    const uint32_t word = avail[b];
    double tot = 0.0;
    for (int p = 0; p < P; ++p) {
      const size_t o = (size_t)p * B + b;
      const double kl = kl_mode ? (kl_rows ? kl_rows[o] : 0.0) : (kl_sum ? kl_sum[p] : 0.0);
      double vb = 0.0, vm = 0.0;
      if (bce) {
        if (tm.bce[p] < 0 || has(word, tm.bce[p])) vb = bce[o];
        else bce[o] = 0.0;
      }
      if (mse) {
        if (tm.mse[p] < 0 || has(word, tm.mse[p])) vm = mse[o];
        else mse[o] = 0.0;
      }
      const double v = vb + (double)pose_multiplier * vm + (double)kl_weight * kl;
      if (partials) partials[o] = (float)v;
      tot += v;
    }
    out[b] = (float)tot;
  }
}

// the passes by value + their availability tables as row words; a table needs with_prior (a row may hold no expert at all: without
// the prior it would divide by zero, and finding such a row needs the table's contents)
int copy_passes_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, int with_prior, int P, PoeAvailArgs* out) {
  if (!passes) return MMDYN_ERR_NULL;
  if (P < 1 || P > MMDYN_MAX_PASSES) return MMDYN_ERR_SHAPE;
  for (int p = 0; p < P; ++p) {
    out->pass[p] = passes[p];
    const uint8_t* t = avail ? avail[p] : nullptr;
    if (t && (!with_prior || ((uintptr_t)t & 3))) return MMDYN_ERR_SHAPE;
    out->avail[p] = reinterpret_cast<const uint32_t*>(t);
  }
  return MMDYN_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int mmdyn_poe_fwd_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise, float* mu,
                                   float* logvar, float* z, double* kl_sum, int with_prior, int P, int B, int L, void* stream) {
  if (!mu || !logvar || (z && !eps_noise)) return MMDYN_ERR_NULL;
  PoeAvailArgs a{};
  if (int e = copy_passes_avail(passes, avail, with_prior, P, &a)) return e;
  if (B <= 0 || L <= 0) return MMDYN_ERR_SHAPE;
  for (int p = 0; p < P; ++p)
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m)
      if ((a.pass[p].mu[m] != nullptr) != (a.pass[p].lv[m] != nullptr)) return MMDYN_ERR_NULL;
  int gx = ew_grid((int64_t)B * L);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(poe_fwd_avail_kernel, dim3(gx, P), dim3(256), 0, ST, a, eps_noise, mu, logvar, z, kl_sum, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_poe_bwd_avail(const mmdyn_pass_experts* passes, const uint8_t* const* avail, const float* eps_noise,
                                   const float* mu, const float* logvar, const float* dz, const float* g_mu, const float* g_lv,
                                   float kl_scale, int with_prior, int P, int B, int L, const float* kl_weight_dev, void* stream) {
  if (!mu || !logvar || (dz && !eps_noise)) return MMDYN_ERR_NULL;
  PoeAvailArgs a{};
  if (int e = copy_passes_avail(passes, avail, with_prior, P, &a)) return e;
  if (B <= 0 || L <= 0) return MMDYN_ERR_SHAPE;
  for (int p = 0; p < P; ++p) {
    for (int m = 0; m < MMDYN_MAX_EXPERTS; ++m)
      if (a.pass[p].mu[m] && (!a.pass[p].lv[m] || !a.pass[p].dmu[m] || !a.pass[p].dlv[m])) return MMDYN_ERR_NULL;
    for (int k = 0; k < 3; ++k)
      if (a.pass[p].dz[k] && !eps_noise) return MMDYN_ERR_NULL;
  }
  int gx = ew_grid((int64_t)B * L);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(poe_bwd_avail_kernel, dim3(gx, P), dim3(256), 0, ST, a, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale,
                     kl_weight_dev, with_prior, B, L);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_complete_select(const float* x, const float* recon, const uint8_t* avail, int modality, float* out, int B,
                                     int row_len, int logits, void* stream) {
  if (!recon || !out) return MMDYN_ERR_NULL;
  if (B <= 0 || row_len <= 0 || modality < 0 || modality >= MMDYN_MAX_EXPERTS || ((uintptr_t)avail & 3)) return MMDYN_ERR_SHAPE;
  const int64_t n = (int64_t)B * row_len;
  if (n >= (1LL << 31)) return MMDYN_ERR_RANGE;
  const bool vec = (((uintptr_t)x | (uintptr_t)recon | (uintptr_t)out) & 15) == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  int g = ew_grid(n4 ? n4 : n);
  hipLaunchKernelGGL(complete_select_kernel, dim3(g), dim3(256), 0, ST, x, recon, reinterpret_cast<const uint32_t*>(avail), modality,
                     out, n, n4, row_len, logits);
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
  hipLaunchKernelGGL(elbo_assemble_rows_avail_kernel, dim3(ew_grid(B)), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, kl_sum, out,
                     partials, reinterpret_cast<const uint32_t*>(avail), tm, P, B, kl_weight, pose_multiplier, kl_weight_dev, kl_mode);
  MMDYN_LAUNCH_CHECK();
}
