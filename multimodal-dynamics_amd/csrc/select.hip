// Observed-or-reconstructed selects:
//   out[b][i] = observed(b) ? x[b][i] : (logits ? sigmoid(recon[b][i]) : recon[b][i]),
//   observed(b) = x != null && (avail == null || avail[b][column] != 0)
// (availability table: common.h; the reference runs MVAE.forward, vae.py:126-165, once per modality subset and takes image logits to
// image space on the host, problems.py:616-626).  ONE element scheme, select_rows, behind both entry points, so a rollout feed
// group has the bits of mmdyn_complete_select:
//   - complete_select: the completion of a mixed-modality batch, one launch per modality;
//   - rollout_feed: multi-step rollout of the one-step dynamics model (--problem-type dyn_modeling), the predictor applied to its
//     own output T times inside ONE captured graph.  The only launch a step adds to the forward is the feed: it turns the step's
//     decoder outputs into the NEXT step's inputs for up to MMDYN_FEED_GROUPS tensors at once (visual image, tactile image, pose),
//     one dependent launch per step.  out is the trajectory slot of the step, which the next step's encoders read in place.
//     A block belongs to ONE group (first_block[] is an exclusive scan of the groups' block counts, which follow their quad
//     counts: the pose group is 7 * B floats next to 12288 * B), so the group's pointers and flags are block-uniform and the
//     row's presence is wave-uniform wherever 256 consecutive floats lie in one row.
//   - plan_select / gather_best: N candidate conditions per request (MVAEInference.plan).  plan_select forms the fp64 cost of
//     every (candidate, row) from the row tables, writes the [N][B] cost table and each row's winner (index, cost, condition);
//     gather_best copies the winner's decoder rows out of the [N * B] candidate-major outputs, for up to MMDYN_FEED_GROUPS tensors
//     in one launch (images through sigmoid_exact, so a taken row has the bits of mmdyn_complete_select(x = null) on that row).
//     Both read best[] from device memory: the choice never visits the host and the request sits in one captured graph.
//   - plan_select_steps / gather_best_steps: N candidate condition SEQUENCES per request rolled out over T steps
//     (MVAEInference.plan_rollout).  plan_select_steps forms plan_select's cost per scored step, the weighted total over the steps
//     in fp64 and each row's winner (and, on request, the K best); gather_best_steps copies the winner's rows of all T steps out of
//     the [T][N * B] trajectory tensors in one launch, with gather_best's element scheme on every step slice.  One kernel per
//     pair: plan_select and gather_best are the T = 1 launches of these two.
//   - ensemble_feed: the rollout feed of N sampled trajectories per request row (MVAEInference.rollout(samples=N)).  The N * B
//     decoder rows of a step become the N * B next states under observations that exist once per request row, and the same read
//     of the logits leaves the ensemble's per-element mean and variance and each row's summed variance.  An element scheme of
//     its own (a thread walks the samples of one quad); its out has the bits of rollout_feed on the N * B rows.
//   - ensemble_quantiles: Q order statistics per element over the N samples of the same decoder outputs
//     (MVAEInference.rollout(samples=N, quantiles=...)): one launch after the step's ensemble_feed.  A wavefront ranks the samples
//     of 64 elements in LDS; a selected image value has the bits ensemble_feed wrote (the same sigmoid_exact).
//   - plan_sample / plan_refit: the two launches that turn the horizon planner into the cross-entropy method
//     (MVAEInference.plan_refine).  plan_sample writes an iteration's candidates mean + std * eps (slot 0: the incumbent), clamped,
//     straight into the [T][N * B][cd] layout the steps read; plan_refit ranks a row's [N] cost column in LDS, flags the K smallest
//     and refits mean / std over them in fp64, one block per row.
//   - plan_refit_weighted / plan_shift: MPPI and the receding horizon (plan_refine(temperature=..., warm_start=...)).
//     plan_refit_weighted is plan_refit with the weight exp(-(cost - cost_min) / temperature) on every elite (K == N: nothing is
//     ranked) -- the two instantiations of one kernel body; plan_shift moves a previous plan's mean / std / winner `shift` steps on
//     and fills the tail from the initial distribution, one launch in front of the loop.
// Memory-bound, no LDS (except plan_refit_kernel: 20 KB in its unweighted instantiation, 52 KB in the weighted one; and
// ensemble_quantiles: 256 bytes per sample, 32 KB at most), no scratch; no atomics except ensemble_feed's spread accumulator.
#include "common.h"

namespace {

// out [B][row_len] as one flat array of n = B * row_len floats: quads [0, n4) by 16-byte accesses (n4 = 0 when a pointer is not
// 16-byte aligned), the elements from 4 * n4 on one by one.  A quad inside ONE row reads only the side it takes (the other may hold
// NaN / Inf); a quad that straddles rows (row_len % 4 != 0: the 7-DoF pose) reads both and selects per element.  x == null: no row
// is present.  Thread tid of nthreads.
__device__ __forceinline__ void select_rows(const float* x, const float* recon, const uint32_t* avail, int column, float* out,
                                            int64_t n, int64_t n4, int row_len, int logits, int64_t tid, int64_t nthreads) {
  for (int64_t q = tid; q < n4; q += nthreads) {
    const int64_t e0 = 4 * q;
    const int b0 = (int)(e0 / row_len), b3 = (int)((e0 + 3) / row_len);
    f32x4 v;
    if (b0 == b3) {
      const bool present = x != nullptr && (!avail || has(avail[b0], column));
      if (present) {
        v = *reinterpret_cast<const f32x4*>(x + e0);
      } else {
        v = *reinterpret_cast<const f32x4*>(recon + e0);
        if (logits) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = sigmoid_exact(v[k]);
        }
      }
    } else {
      const f32x4 r = *reinterpret_cast<const f32x4*>(recon + e0);
      f32x4 xv = r;
      if (x) xv = *reinterpret_cast<const f32x4*>(x + e0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = (int)((e0 + k) / row_len);
        const bool present = x != nullptr && (!avail || has(avail[b], column));
        v[k] = present ? xv[k] : (logits ? sigmoid_exact(r[k]) : r[k]);
      }
    }
    *reinterpret_cast<f32x4*>(out + e0) = v;
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nthreads) {
    const int b = (int)(i / row_len);
    const bool present = x != nullptr && (!avail || has(avail[b], column));
    float v;
    if (present) {
      v = x[i];
    } else {
      v = recon[i];
      if (logits) v = sigmoid_exact(v);
    }
    out[i] = v;
  }
}

__global__ __launch_bounds__(256) void complete_select_kernel(const float* __restrict__ x, const float* __restrict__ recon,
                                                              const uint32_t* __restrict__ avail, int modality,
                                                              float* __restrict__ out, int64_t n, int64_t n4, int row_len,
                                                              int logits) {
  select_rows(x, recon, avail, modality, out, n, n4, row_len, logits, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
              (int64_t)gridDim.x * blockDim.x);
}

struct FeedArgs {
  const float* recon[MMDYN_FEED_GROUPS];
  const float* obs[MMDYN_FEED_GROUPS];
  float* out[MMDYN_FEED_GROUPS];
  int64_t n[MMDYN_FEED_GROUPS], n4[MMDYN_FEED_GROUPS];
  int row_len[MMDYN_FEED_GROUPS], logits[MMDYN_FEED_GROUPS], column[MMDYN_FEED_GROUPS];
  int first_block[MMDYN_FEED_GROUPS + 1];
};

__global__ __launch_bounds__(256) void rollout_feed_kernel(const FeedArgs a, const uint32_t* __restrict__ avail, int G) {
  int g = 0;
#pragma unroll
  for (int k = 1; k < MMDYN_FEED_GROUPS; ++k)
    if (k < G && (int)blockIdx.x >= a.first_block[k]) g = k;
  select_rows(a.obs[g], a.recon[g], avail, a.column[g], a.out[g], a.n[g], a.n4[g], a.row_len[g], a.logits[g],
              (int64_t)((int)blockIdx.x - a.first_block[g]) * blockDim.x + threadIdx.x,
              (int64_t)(a.first_block[g + 1] - a.first_block[g]) * blockDim.x);
}

// ---- ensemble rollout: the feed of N trajectories per request row, with the ensemble's statistics from the same read ----

// W consecutive floats: one 16-byte access (W = 4) or one element (W = 1)
template <int W> __device__ __forceinline__ void ld_w(const float* p, float* v);
template <> __device__ __forceinline__ void ld_w<4>(const float* p, float* v) {
  const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = q[k];
}
template <> __device__ __forceinline__ void ld_w<1>(const float* p, float* v) { v[0] = p[0]; }
template <int W> __device__ __forceinline__ void st_w(float* p, const float* v);
template <> __device__ __forceinline__ void st_w<4>(float* p, const float* v) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
}
template <> __device__ __forceinline__ void st_w<1>(float* p, const float* v) { p[0] = v[0]; }

struct EnsembleArgs {
  const float* recon[MMDYN_FEED_GROUPS];
  const float* obs[MMDYN_FEED_GROUPS];
  float* out[MMDYN_FEED_GROUPS];
  float* mean[MMDYN_FEED_GROUPS];
  float* var[MMDYN_FEED_GROUPS];
  double* spread[MMDYN_FEED_GROUPS];
  int64_t plane[MMDYN_FEED_GROUPS];          // B * row_len: the floats of one sample, the stride between samples
  int row_len[MMDYN_FEED_GROUPS], logits[MMDYN_FEED_GROUPS], column[MMDYN_FEED_GROUPS], vec[MMDYN_FEED_GROUPS];
  int first_block[MMDYN_FEED_GROUPS + 1];
};

constexpr int ENSEMBLE_UNROLL = 8;           // loads of one thread in flight while it walks the samples

// The [B][row_len] plane as items of W floats (W = 4: plane % 4 == 0 and every pointer 16-byte aligned; W = 1 otherwise).  A
// thread owns one item and walks the samples n = 0 .. N-1 of recon [N][plane]: every recon element is loaded once, its p =
// logits ? sigmoid_exact(r) : r goes to out[n] (or the observation, loaded once before the walk and only for the elements whose
// row takes it) and into the fp64 sums around c = p_0: d = p_n - c, S1 += d, S2 += d * d, in n order;
// mean = (float)(c + S1 / N), var = (float)max(0, (S2 - S1 * S1 / N) / N) (a NaN stays a NaN).  spread[b] += the fp32 var values
// of row b, widened: one atomic per wave where the wave's items lie in one row, one per item inside a row, one per element of
// an item that straddles rows.  `wave0` / `nthreads`: the first item of this wave and the items of one sweep of the group's
// blocks, so the trip count is wave-uniform and every lane reaches the shuffles.
template <int W>
__device__ __forceinline__ void ensemble_rows(const float* recon, const float* obs, const uint32_t* avail, int column, float* out,
                                              float* mean, float* var, double* spread, int64_t plane, int row_len, int logits,
                                              int N, int64_t wave0, int64_t nthreads) {
  const int64_t items = plane / W;
  const int lane = threadIdx.x & 63;
  const double inv_n = 1.0 / (double)N;
  for (int64_t base = wave0; base < items; base += nthreads) {
    const int64_t q = base + lane;
    const bool active = q < items;
    const int64_t e0 = active ? W * q : 0;
    const int b0 = (int)(e0 / row_len), b3 = (int)((e0 + W - 1) / row_len);
    float fvar[W];
#pragma unroll
    for (int k = 0; k < W; ++k) fvar[k] = 0.f;
    if (active) {
      bool taken[W];
      float ob[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const int b = b0 == b3 ? b0 : (int)((e0 + k) / row_len);
        taken[k] = obs != nullptr && (!avail || has(avail[b], column));
        ob[k] = 0.f;
      }
      if (b0 == b3) {
        if (taken[0]) ld_w<W>(obs + e0, ob);
      } else {
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (taken[k]) ob[k] = obs[e0 + k];
      }
      double c[W], s1[W], s2[W];
#pragma unroll
      for (int k = 0; k < W; ++k) c[k] = s1[k] = s2[k] = 0.0;
      auto sample = [&](int n, float* p) {
        float o[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if (logits) p[k] = sigmoid_exact(p[k]);
          if (n == 0) c[k] = (double)p[k];
          const double d = (double)p[k] - c[k];
          s1[k] += d;
          s2[k] += d * d;
          o[k] = taken[k] ? ob[k] : p[k];
        }
        st_w<W>(out + (int64_t)n * plane + e0, o);
      };
      const float* src = recon + e0;
      int n = 0;
      for (; n + ENSEMBLE_UNROLL <= N; n += ENSEMBLE_UNROLL) {
        float r[ENSEMBLE_UNROLL][W];
#pragma unroll
        for (int u = 0; u < ENSEMBLE_UNROLL; ++u) ld_w<W>(src + (int64_t)(n + u) * plane, r[u]);
#pragma unroll
        for (int u = 0; u < ENSEMBLE_UNROLL; ++u) sample(n + u, r[u]);
      }
      for (; n < N; ++n) {
        float r[W];
        ld_w<W>(src + (int64_t)n * plane, r);
        sample(n, r);
      }
      float fmean[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        fmean[k] = (float)(c[k] + s1[k] * inv_n);
        const double v = (s2[k] - s1[k] * s1[k] * inv_n) * inv_n;
        fvar[k] = (float)(v < 0.0 ? 0.0 : v);
      }
      st_w<W>(mean + e0, fmean);
      if (var) st_w<W>(var + e0, fvar);
    }
    if (spread) {
      // (wave-uniform: base and items are, and the vote covers every lane)
      const int bw = __builtin_amdgcn_readfirstlane(b0);
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) s += (double)fvar[k];
      if (__all(!active || (b0 == bw && b3 == bw))) {
        s = wave_sum_d(s);
        if (lane == 0) atomicAdd(spread + bw, s);
      } else if (active) {
        if (b0 == b3) {
          atomicAdd(spread + b0, s);
        } else {
#pragma unroll
          for (int k = 0; k < W; ++k) atomicAdd(spread + (int)((e0 + k) / row_len), (double)fvar[k]);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void ensemble_feed_kernel(const EnsembleArgs a, const uint32_t* __restrict__ avail, int G, int N) {
  int g = 0;
#pragma unroll
  for (int k = 1; k < MMDYN_FEED_GROUPS; ++k)
    if (k < G && (int)blockIdx.x >= a.first_block[k]) g = k;
  const int64_t wave0 = (int64_t)((int)blockIdx.x - a.first_block[g]) * blockDim.x + (threadIdx.x & ~63u);
  const int64_t nthreads = (int64_t)(a.first_block[g + 1] - a.first_block[g]) * blockDim.x;
  if (a.vec[g])
    ensemble_rows<4>(a.recon[g], a.obs[g], avail, a.column[g], a.out[g], a.mean[g], a.var[g], a.spread[g], a.plane[g], a.row_len[g],
                     a.logits[g], N, wave0, nthreads);
  else
    ensemble_rows<1>(a.recon[g], a.obs[g], avail, a.column[g], a.out[g], a.mean[g], a.var[g], a.spread[g], a.plane[g], a.row_len[g],
                     a.logits[g], N, wave0, nthreads);
}

// ---- ensemble rollout: order statistics of the N samples of every element ----

struct QuantileArgs {
  const float* src[MMDYN_FEED_GROUPS];
  float* out[MMDYN_FEED_GROUPS];
  int64_t plane[MMDYN_FEED_GROUPS];          // B * row_len: the floats of one sample, the stride between samples and between quantiles
  int logits[MMDYN_FEED_GROUPS], vec[MMDYN_FEED_GROUPS];
  int first_block[MMDYN_FEED_GROUPS + 1];
  int lo[MMDYN_QUANTILES_MAX], hi[MMDYN_QUANTILES_MAX];     // hi = min(lo + 1, N - 1), formed on the host
  double frac[MMDYN_QUANTILES_MAX];
};

constexpr int QUANTILE_CHUNK = 64;           // elements of one chunk: one per lane of the block's single wavefront
constexpr int QUANTILE_UNROLL = 4;           // loads of one thread in flight while the chunk is brought in

// s_lo + frac * (s_hi - s_lo) in fp64, the difference, the product and the sum rounded on their own (the pragma as in plan_cost),
// then one rounding to fp32.
__device__ __forceinline__ float quantile_lerp(float a, float b, double frac) {
#pragma clang fp contract(off)
  const double d = (double)b - (double)a;
  const double p = frac * d;
  return (float)((double)a + p);
}

// One block = one wavefront works on chunks of 64 consecutive elements of the plane.  A chunk's N x 64 values p go through LDS
// once: column `lane` of col[N4 / 4][64][4] (sample n of element c at (n / 4, c, n % 4); N4 = N rounded up to four, the pad NaN) is
// the sample vector of element c.  Bringing in: every src element is loaded once -- 16 bytes per lane where the group allows it
// (16 lanes cover the chunk, so one wave instruction brings four samples), one float per lane otherwise.  Selecting: lane c owns
// element c and walks its column four samples at a time; the rank of sample n is the number of samples in front of it -- a
// smaller value, or an equal one with a smaller n --, so the ranks of an element without NaN are a permutation of 0 .. N-1 and
// s_k is the sample of rank k.  The pad counts in front of nothing (every comparison with NaN is false) and is never selected
// (n < N).  Every loop bound is block-uniform (the barriers) and every index into the Q-sized register arrays is a compile-time
// constant (no scratch).  Writing: 4 bytes per lane, or through the first Q rows of LDS as 16-byte stores.
__global__ __launch_bounds__(QUANTILE_CHUNK) void ensemble_quantiles_kernel(const QuantileArgs a, int G, int Q, int N) {
  extern __shared__ __attribute__((aligned(16))) float col[];                 // max(N4, MMDYN_QUANTILES_MAX) * 64 floats
  int g = 0;
#pragma unroll
  for (int k = 1; k < MMDYN_FEED_GROUPS; ++k)
    if (k < G && (int)blockIdx.x >= a.first_block[k]) g = k;
  const float* __restrict__ src = a.src[g];
  float* __restrict__ out = a.out[g];
  const int64_t plane = a.plane[g];
  const int logits = a.logits[g], vec = a.vec[g];
  const int lane = threadIdx.x;
  const int N4 = (N + 3) & ~3;
  const int64_t chunks = (plane + QUANTILE_CHUNK - 1) / QUANTILE_CHUNK;
  const int nblocks = a.first_block[g + 1] - a.first_block[g];
  for (int64_t chunk = (int)blockIdx.x - a.first_block[g]; chunk < chunks; chunk += nblocks) {
    const int64_t e0 = chunk * QUANTILE_CHUNK;
    // ---- the chunk's samples into LDS ----
    if (vec) {
      const int quad = lane & 15, sub = lane >> 4;                            // this lane: elements 4 * quad .. + 3 of sample n0 + sub
      const int64_t e = e0 + 4 * quad;
      const bool inside = e < plane;                                          // (plane % 4 == 0: a quad is inside or outside)
      for (int n0 = 0; n0 < N4; n0 += 4 * QUANTILE_UNROLL) {
        float r[QUANTILE_UNROLL][4];
#pragma unroll
        for (int u = 0; u < QUANTILE_UNROLL; ++u) {
          const int n = n0 + 4 * u + sub;
#pragma unroll
          for (int k = 0; k < 4; ++k) r[u][k] = NAN;
          if (inside && n < N) ld_w<4>(src + (int64_t)n * plane + e, r[u]);
        }
#pragma unroll
        for (int u = 0; u < QUANTILE_UNROLL; ++u) {
          const int n = n0 + 4 * u + sub;
          if (n < N4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float p = (logits && n < N) ? sigmoid_exact(r[u][k]) : r[u][k];
              col[((n >> 2) * QUANTILE_CHUNK + 4 * quad + k) * 4 + (n & 3)] = p;
            }
          }
        }
      }
    } else {
      const bool inside = e0 + lane < plane;
      for (int n0 = 0; n0 < N4; n0 += 4) {
        float r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          r[u] = NAN;
          if (inside && n0 + u < N) ld_w<1>(src + (int64_t)(n0 + u) * plane + e0 + lane, &r[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (logits && n0 + u < N) r[u] = sigmoid_exact(r[u]);
        *reinterpret_cast<f32x4*>(col + ((n0 >> 2) * QUANTILE_CHUNK + lane) * 4) = f32x4{r[0], r[1], r[2], r[3]};
      }
    }
    __syncthreads();
    // ---- lane = element: ranks and the 2 Q order statistics ----
    float s_lo[MMDYN_QUANTILES_MAX], s_hi[MMDYN_QUANTILES_MAX];
#pragma unroll
    for (int j = 0; j < MMDYN_QUANTILES_MAX; ++j) s_lo[j] = s_hi[j] = 0.f;
    bool nan = false;
    for (int n0 = 0; n0 < N4; n0 += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(col + ((n0 >> 2) * QUANTILE_CHUNK + lane) * 4);
      int rank[4] = {0, 0, 0, 0};
      for (int m0 = 0; m0 < n0; m0 += 4) {                                    // earlier samples: an equal one is in front
        const f32x4 w = *reinterpret_cast<const f32x4*>(col + ((m0 >> 2) * QUANTILE_CHUNK + lane) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 4; ++k) rank[i] += w[k] <= v[i] ? 1 : 0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k != i) rank[i] += (k < i ? v[k] <= v[i] : v[k] < v[i]) ? 1 : 0;
      for (int m0 = n0 + 4; m0 < N4; m0 += 4) {                               // later samples: only a smaller one is
        const f32x4 w = *reinterpret_cast<const f32x4*>(col + ((m0 >> 2) * QUANTILE_CHUNK + lane) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 4; ++k) rank[i] += w[k] < v[i] ? 1 : 0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (n0 + i < N) {
          nan = nan || (v[i] != v[i]);
#pragma unroll
          for (int j = 0; j < MMDYN_QUANTILES_MAX; ++j) {
            if (j < Q) {
              s_lo[j] = rank[i] == a.lo[j] ? v[i] : s_lo[j];
              s_hi[j] = rank[i] == a.hi[j] ? v[i] : s_hi[j];
            }
          }
        }
      }
    }
    float res[MMDYN_QUANTILES_MAX];
#pragma unroll
    for (int j = 0; j < MMDYN_QUANTILES_MAX; ++j) {
      res[j] = 0.f;
      if (j < Q) {
        res[j] = a.frac[j] == 0.0 ? s_lo[j] : quantile_lerp(s_lo[j], s_hi[j], a.frac[j]);
        if (nan) res[j] = NAN;
      }
    }
    // ---- the Q results of the chunk ----
    if (vec) {
      __syncthreads();                                                        // every lane is done with its column
#pragma unroll
      for (int j = 0; j < MMDYN_QUANTILES_MAX; ++j)
        if (j < Q) col[j * QUANTILE_CHUNK + lane] = res[j];
      __syncthreads();
      for (int i = lane; i < Q * (QUANTILE_CHUNK / 4); i += QUANTILE_CHUNK) {
        const int j = i >> 4, quad = i & 15;
        const int64_t e = e0 + 4 * quad;
        if (e < plane) st_w<4>(out + (int64_t)j * plane + e, col + j * QUANTILE_CHUNK + 4 * quad);
      }
    } else if (e0 + lane < plane) {
#pragma unroll
      for (int j = 0; j < MMDYN_QUANTILES_MAX; ++j)
        if (j < Q) st_w<1>(out + (int64_t)j * plane + e0 + lane, &res[j]);
    }
    __syncthreads();                                                          // LDS is free for the next chunk
  }
}

// ---- candidate conditions: the cost table, the winner of each row, and the winner's rows ----

// The cost in its one written order, ((bce_v + bce_t) + pm * mse) + klw * kl, every product and every sum rounded on its own.
// Contraction is switched off for this function by the pragma: the device default fuses a * b + c into one v_fma_f64 / v_fmac_f64
// (one rounding instead of two), and the HIP headers' __dadd_rn / __dmul_rn are a plain + and * that fuse all the same.  The
// instructions keep the setting when the function is inlined: the kernel holds v_mul_f64 and v_add_f64 for this expression.
__device__ __forceinline__ double plan_cost(double bce_v, double bce_t, double mse, double kl, double pm, double klw) {
#pragma clang fp contract(off)
  const double rec = bce_v + bce_t;
  const double pose = pm * mse;
  const double klt = klw * kl;
  return (rec + pose) + klt;
}

// out [B][row_len] = f(src[best[b] * B + b]) over the flat out array, in the element scheme of select_rows with no observed side:
// quads [0, n4) by 16-byte stores, the elements from 4 * n4 on one by one.  The source of out element e of row b is element
// e + best[b] * n of src (n = B * row_len); a quad inside one row loads 16 bytes where that offset keeps the alignment and four
// floats otherwise (the same values either way).  A row whose index lies outside [0, N) is filled with NaN and reads nothing.
__device__ __forceinline__ void gather_rows(const float* src, const int* best, float* out, int64_t n, int64_t n4, int row_len, int N,
                                            int logits, int64_t tid, int64_t nthreads) {
  auto taken = [&](int b) {
    const int w = best[b];
    return (w < 0 || w >= N) ? (int64_t)-1 : (int64_t)w * n;
  };
  auto value = [&](int64_t off, int64_t e) {
    if (off < 0) return NAN;
    const float r = src[off + e];
    return logits ? sigmoid_exact(r) : r;
  };
  for (int64_t q = tid; q < n4; q += nthreads) {
    const int64_t e0 = 4 * q;
    const int b0 = (int)(e0 / row_len), b3 = (int)((e0 + 3) / row_len);
    f32x4 v;
    const int64_t off0 = taken(b0);
    if (b0 == b3 && off0 >= 0 && ((off0 & 3) == 0)) {
      v = *reinterpret_cast<const f32x4*>(src + off0 + e0);
      if (logits) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = sigmoid_exact(v[k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = (int)((e0 + k) / row_len);
        v[k] = value(b == b0 ? off0 : taken(b), e0 + k);
      }
    }
    *reinterpret_cast<f32x4*>(out + e0) = v;
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nthreads) out[i] = value(taken((int)(i / row_len)), i);
}

// ---- candidate condition SEQUENCES over T steps: the weighted total, the winner of each row, the winner's trajectory ----

// total + w * c (weighted) or total + c, the product and the sum rounded on their own: the pragma as in plan_cost.  `first`: the
// term starts the sum (w * c or c itself, no 0.0 + ...).
__device__ __forceinline__ double add_step(double total, double c, double w, bool weighted, bool first) {
#pragma clang fp contract(off)
  const double term = weighted ? w * c : c;
  return first ? term : total + term;
}

// The running list of the TOP smallest totals, ascending, equal totals in the order they came (n ascending): a fixed register
// array walked by fully unrolled loops only, so no element is addressed by a run-time index.  An empty slot holds index -1.
struct TopList {
  double c[MMDYN_PLAN_TOP_MAX];
  int n[MMDYN_PLAN_TOP_MAX];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < MMDYN_PLAN_TOP_MAX; ++k) {
      c[k] = NAN;
      n[k] = -1;
    }
  }
  // v is no NaN.  From the last slot down: a slot that v goes in front of takes its left neighbour if v goes in front of that one
  // too, and v otherwise (the left neighbour is read before its own turn changes it).
  __device__ __forceinline__ void insert(double v, int idx) {
#pragma unroll
    for (int k = MMDYN_PLAN_TOP_MAX - 1; k > 0; --k) {
      const bool before = n[k] < 0 || v < c[k], before_left = n[k - 1] < 0 || v < c[k - 1];
      if (before) {
        c[k] = before_left ? c[k - 1] : v;
        n[k] = before_left ? n[k - 1] : idx;
      }
    }
    if (n[0] < 0 || v < c[0]) {
      c[0] = v;
      n[0] = idx;
    }
  }
};

// One thread per row b walks the candidates n and, inside, the scored steps t: c_t = plan_cost of the step's table entries,
// total = sum_t w_t * c_t in t order.  The tables are [Tg][N][B] (bce: [2][Tg][N][B]), tavail [Tg][B] words, so every read
// coalesces across b.  A table that is not given, and an absent (row, term), enter plan_cost as +0.0 (x + 0.0 == x for every x
// the tables hold).  Selection on the fp64 total: smallest wins, the first of equals wins, NaN never wins (every comparison
// with it is false), +-Inf are ordinary values.  Tg = T = 1 without weights and without step_cost is the one-step planner's
// launch (mmdyn_plan_select): the total is c_0 itself and cost is the step's table.  STEPS = false makes T = Tg = 1 and the two
// null pointers compile-time facts: no step loop, no weight, no per-step store (measurements: docs/LAB_NOTES.md AD).
template <bool TOP, bool STEPS>
__global__ __launch_bounds__(256) void plan_select_steps_kernel(double* __restrict__ bce, double* __restrict__ mse,
                                                                const double* __restrict__ kl, const uint32_t* __restrict__ tavail,
                                                                const float* __restrict__ step_weight_arg, const float* __restrict__ cand,
                                                                const int64_t* __restrict__ cand_idx, int cd, float* __restrict__ cost,
                                                                float* __restrict__ step_cost_arg, int* __restrict__ best,
                                                                float* __restrict__ best_cost, float* __restrict__ best_cond,
                                                                int64_t* __restrict__ best_idx, int* __restrict__ top,
                                                                float* __restrict__ top_cost, int K, int N, int B, int T_arg, int Tg_arg,
                                                                float pose_multiplier, float kl_weight_arg,
                                                                const float* __restrict__ kl_weight_dev) {
  const float kl_weight = kl_weight_dev ? kl_weight_arg * kl_weight_dev[0] : kl_weight_arg;
  const double pm = (double)pose_multiplier, klw = (double)kl_weight;
  const int T = STEPS ? T_arg : 1, Tg = STEPS ? Tg_arg : 1;
  const float* step_weight = STEPS ? step_weight_arg : nullptr;
  float* step_cost = STEPS ? step_cost_arg : nullptr;
  const size_t NB = (size_t)N * B, TNB = (size_t)Tg * NB;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    double low = NAN;
    int win = -1;
    TopList list;
    if (TOP) list.clear();
    // step 0's word is read once per row, not once per candidate: with Tg = 1 no load of the table is left inside the walk, whose
    // table loads then wait for memory together
    const uint32_t word0 = tavail ? tavail[b] : ALL_PRESENT;
    for (int n = 0; n < N; ++n) {
      double total = 0.0;
      for (int t = 0; t < Tg; ++t) {
        const uint32_t word = (t == 0 || !tavail) ? word0 : tavail[(size_t)t * B + b];
        const bool has0 = has(word, 0), has1 = has(word, 1), has2 = has(word, 2);
        const size_t o = ((size_t)t * N + n) * B + b;
        const double v = bce && has0 ? bce[o] : 0.0, u = bce && has1 ? bce[TNB + o] : 0.0, p = mse && has2 ? mse[o] : 0.0;
        if (bce && !has0) bce[o] = 0.0;
        if (bce && !has1) bce[TNB + o] = 0.0;
        if (mse && !has2) mse[o] = 0.0;
        const double c = plan_cost(v, u, p, kl[o], pm, klw);
        if (step_cost) step_cost[o] = (float)c;
        total = add_step(total, c, step_weight ? (double)step_weight[t] : 1.0, step_weight != nullptr, t == 0);
      }
      cost[(size_t)n * B + b] = (float)total;
      if (total == total) {
        if (win < 0 || total < low) {
          low = total;
          win = n;
        }
        if (TOP) list.insert(total, n);
      }
    }
    best[b] = win;
    best_cost[b] = (float)low;
    for (int t = 0; t < T; ++t) {
      const size_t src = ((size_t)t * N + (win < 0 ? 0 : win)) * B + b, dst = (size_t)b * T + t;
      if (best_idx) best_idx[dst] = win < 0 ? (int64_t)-1 : cand_idx[src];
      if (best_cond)
        for (int j = 0; j < cd; ++j) best_cond[dst * cd + j] = win < 0 ? NAN : cand[src * cd + j];
    }
    if (TOP) {
#pragma unroll
      for (int k = 0; k < MMDYN_PLAN_TOP_MAX; ++k)
        if (k < K) {
          top[(size_t)k * B + b] = list.n[k];
          top_cost[(size_t)k * B + b] = (float)list.c[k];
        }
    }
  }
}

struct GatherStepsArgs {
  const float* src[MMDYN_FEED_GROUPS];
  float* out[MMDYN_FEED_GROUPS];
  int64_t n[MMDYN_FEED_GROUPS];               // B * row_len: the floats of one step's out; N * n those of one step's src
  int row_len[MMDYN_FEED_GROUPS], logits[MMDYN_FEED_GROUPS];
  int per_step[MMDYN_FEED_GROUPS];            // blocks that cover one step with one item per thread
  int first_block[MMDYN_FEED_GROUPS + 1];
};

// gather_rows on every step slice: the group's blocks walk its T * per_step (step, chunk) pieces, so the step -- and with it the
// slice pointers and whether they allow 16-byte accesses -- is block-uniform.  T = 1 is the one-step planner's launch
// (mmdyn_gather_best): a piece is then one chunk of its only slice, which STEPS = false makes a compile-time fact (no 64-bit
// division per piece; measurements: docs/LAB_NOTES.md AD).
template <bool STEPS>
__global__ __launch_bounds__(256) void gather_best_steps_kernel(const GatherStepsArgs a, const int* __restrict__ best, int G, int N,
                                                                int T) {
  int g = 0;
#pragma unroll
  for (int k = 1; k < MMDYN_FEED_GROUPS; ++k)
    if (k < G && (int)blockIdx.x >= a.first_block[k]) g = k;
  const int blocks = a.first_block[g + 1] - a.first_block[g], per_step = a.per_step[g];
  const int64_t n = a.n[g];
  for (int64_t piece = (int)blockIdx.x - a.first_block[g]; piece < (STEPS ? (int64_t)T * per_step : per_step); piece += blocks) {
    const int t = STEPS ? (int)(piece / per_step) : 0, chunk = STEPS ? (int)(piece % per_step) : (int)piece;
    const float* src = a.src[g] + (int64_t)t * N * n;
    float* out = a.out[g] + (int64_t)t * n;
    const bool vec = (((uintptr_t)src | (uintptr_t)out) & 15) == 0;
    gather_rows(src, best, out, n, vec ? n / 4 : 0, a.row_len[g], N, a.logits[g], (int64_t)chunk * blockDim.x + threadIdx.x,
                (int64_t)per_step * blockDim.x);
  }
}

// ---- iterative refinement of a candidate distribution (CEM): the candidates of an iteration, the elites and the refit ----

// c = mean + std * eps, the product and the sum rounded on their own: the pragma as in plan_cost.
__device__ __forceinline__ float sample_value(float mean, float std, float eps) {
#pragma clang fp contract(off)
  const float p = std * eps;
  return mean + p;
}

// cand [T][N * B][cd] as items of W floats (W = 4: cd % 4 == 0 and every pointer 16-byte aligned, so an item lies in one (t, n, b)
// row and every operand's offset is a multiple of four; W = 1 otherwise), one item per thread.  Item i of the output sits at
// ((t * N + n) * B + b) * cd + d; mean / std / keep are [B][T][cd], eps [N][B][T][cd].  Slot n = 0 is the incumbent: keep where it
// is given and no NaN, mean otherwise, and its eps is not loaded.
template <int W>
__global__ __launch_bounds__(256) void plan_sample_kernel(const float* __restrict__ mean, const float* __restrict__ std,
                                                          const float* __restrict__ eps, const float* __restrict__ keep,
                                                          const float* __restrict__ lo, const float* __restrict__ hi,
                                                          float* __restrict__ cand, int N, int B, int T, int cd, int64_t items) {
  const int per_row = cd / W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % per_row) * W;
    const int64_t row = i / per_row;                     // (t * N + n) * B + b
    const int b = (int)(row % B);
    const int64_t tn = row / B;
    const int n = (int)(tn % N), t = (int)(tn / N);
    const int64_t src = ((int64_t)b * T + t) * cd + d;
    float m[W], c[W];
    ld_w<W>(mean + src, m);
    if (n == 0) {
#pragma unroll
      for (int k = 0; k < W; ++k) c[k] = m[k];
      if (keep) {
        float kp[W];
        ld_w<W>(keep + src, kp);
#pragma unroll
        for (int k = 0; k < W; ++k) c[k] = kp[k] == kp[k] ? kp[k] : m[k];
      }
    } else {
      float s[W], e[W];
      ld_w<W>(std + src, s);
      ld_w<W>(eps + (((int64_t)n * B + b) * T + t) * cd + d, e);
#pragma unroll
      for (int k = 0; k < W; ++k) c[k] = sample_value(m[k], s[k], e[k]);
    }
    if (lo) {
      float l[W], h[W];
      ld_w<W>(lo + d, l);
      ld_w<W>(hi + d, h);
#pragma unroll
      for (int k = 0; k < W; ++k) c[k] = c[k] < l[k] ? l[k] : (c[k] > h[k] ? h[k] : c[k]);
    }
    st_w<W>(cand + row * cd + d, c);
  }
}

// The refit's arithmetic in its written order, every product, quotient and sum rounded on its own (the pragma as in plan_cost).
__device__ __forceinline__ double add_square(double acc, double c, double m) {
#pragma clang fp contract(off)
  const double d = c - m;
  const double sq = d * d;
  return acc + sq;
}
__device__ __forceinline__ double blend(double alpha, double prev, double fit) {
#pragma clang fp contract(off)
  const double a = alpha * prev;
  const double rest = 1.0 - alpha;
  const double f = rest * fit;
  return a + f;
}

// The weighted (MPPI) refit's arithmetic in its written order, every operation rounded on its own (the pragma as in plan_cost).
// w = exp(-(((double)c - (double)c_min) / (double)temperature)) for c != c_min.
__device__ __forceinline__ double mppi_weight(float c, float c_min, float temperature) {
#pragma clang fp contract(off)
  const double d = (double)c - (double)c_min;
  const double q = d / (double)temperature;
  return exp(-q);
}
__device__ __forceinline__ double add_weighted(double acc, double w, double c) {
#pragma clang fp contract(off)
  const double p = w * c;
  return acc + p;
}
__device__ __forceinline__ double add_weighted_square(double acc, double w, double c, double m) {
#pragma clang fp contract(off)
  const double d = c - m;
  const double sq = d * d;
  const double p = w * sq;
  return acc + p;
}
__device__ __forceinline__ float effective_samples(double W, double Q) {
#pragma clang fp contract(off)
  const double ww = W * W;
  return (float)(ww / Q);
}

constexpr int REFIT_WALK = 8;                // candidate loads of one thread in flight while it walks a weight column

// One block of 256 threads per row b.  The row's cost column goes into LDS (padded with NaN to a multiple of four, so the rank
// walk reads quads; every lane reads the same address: a broadcast); thread n counts the candidates in front of n -- a smaller
// cost, or an equal one with a smaller index; a NaN is in front of nothing and is itself never an elite -- and n is an elite iff
// fewer than K are (K == N: no candidate is cut, ahead <= N - 1 < K, so nothing is ranked and the flag is cost == cost).  The
// flags stay in LDS; their number K' is summed by the shuffle and four LDS words.  Each thread then owns elements (t, d) and
// walks n = 0 .. N-1 twice over a weight column, loading the candidates of non-zero weight only: one fixed summation order, no
// compaction.  mean_out / std_out may be mean_in / std_in (an element is read and written by the same thread).
//   WEIGHTED = false (CEM, mmdyn_plan_refit): the weight column is the flags and the divisor W is K'; 20 KB static LDS.
//   WEIGHTED = true (MPPI, mmdyn_plan_refit_weighted): c_min = the smallest elite cost (an order-free block reduction), the fp64
//     weight column in LDS (32 KB more: 52 KB static), W = sum w and Q = sum w * w walked by every thread in ascending n from LDS
//     broadcasts (the walk an element's sums take anyway; one order, no reduction tree).  All weights 1 (equal elite costs):
//     add_weighted(acc, 1, c) is acc + c and W is K', so the outputs have the other instantiation's bits.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void plan_refit_kernel(const float* __restrict__ cost, const float* __restrict__ cand,
                                                         const float* mean_in, const float* std_in, float* mean_out, float* std_out,
                                                         uint8_t* __restrict__ elite, int* __restrict__ count,
                                                         double* __restrict__ weight, float* __restrict__ ess, int K, int N, int B,
                                                         int T, int cd, float temperature, float alpha, float std_min) {
  __shared__ __attribute__((aligned(16))) float cost_s[MMDYN_REFIT_N_MAX];
  // w_s and low_s: every reference sits under `if constexpr (WEIGHTED)`, so the unweighted instantiation has none and the
  // compiler allocates neither (its 20496 bytes are cost_s + flag_s + part_s; the resource table of docs/LAB_NOTES.md AD, taken
  // with -Rpass-analysis=kernel-resource-usage, is the check to repeat when this body changes)
  __shared__ __attribute__((aligned(16))) double w_s[WEIGHTED ? MMDYN_REFIT_N_MAX : 1];
  __shared__ uint8_t flag_s[MMDYN_REFIT_N_MAX];
  __shared__ int part_s[4];
  __shared__ float low_s[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N4 = (N + 3) & ~3;
  for (int n = tid; n < N4; n += 256) cost_s[n] = n < N ? cost[(size_t)n * B + b] : NAN;
  __syncthreads();
  int mine = 0;
  float low = INFINITY;                                  // over this thread's elites; used only where K' > 0
  for (int n = tid; n < N; n += 256) {
    const float c = cost_s[n];
    int ahead = 0;
    if (K < N) {
      for (int m = 0; m < N4; m += 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(cost_s + m);
#pragma unroll
        for (int k = 0; k < 4; ++k) ahead += (q[k] < c || (q[k] == c && m + k < n)) ? 1 : 0;
      }
    }
    const int flag = (c == c && ahead < K) ? 1 : 0;
    flag_s[n] = (uint8_t)flag;
    if (elite) elite[(size_t)n * B + b] = (uint8_t)flag;
    mine += flag;
    if (WEIGHTED && flag && c < low) low = c;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mine += __shfl_xor(mine, off, 64);
    if constexpr (WEIGHTED) {
      const float other = __shfl_xor(low, off, 64);
      low = other < low ? other : low;
    }
  }
  if ((tid & 63) == 0) {
    part_s[tid >> 6] = mine;
    if constexpr (WEIGHTED) low_s[tid >> 6] = low;
  }
  __syncthreads();
  const int kp = part_s[0] + part_s[1] + part_s[2] + part_s[3];
  if (count && tid == 0) count[b] = kp;
  double W = (double)kp;                                 // unweighted: every elite weighs 1
  if constexpr (WEIGHTED) {
    float c_min = low_s[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) c_min = low_s[k] < c_min ? low_s[k] : c_min;
    for (int n = tid; n < N; n += 256) {
      const float c = cost_s[n];
      double w = 0.0;
      if (flag_s[n]) w = c == c_min ? 1.0 : mppi_weight(c, c_min, temperature);
      w_s[n] = w;
      if (weight) weight[(size_t)n * B + b] = w;
    }
    __syncthreads();
    double Q = 0.0;
    W = 0.0;
    if (kp != 0) {
      for (int n = 0; n < N; ++n) {
        const double w = w_s[n];
        W += w;
        Q = add_weighted(Q, w, w);
      }
    }
    if (ess && tid == 0) ess[b] = kp == 0 ? 0.f : effective_samples(W, Q);
  }
  auto weight_of = [&](int n) {
    if constexpr (WEIGHTED) return w_s[n];
    else return flag_s[n];
  };
  const double a = (double)alpha;
  const size_t step = (size_t)N * B * cd;                // the floats of one step slice of cand
  for (int e = tid; e < T * cd; e += 256) {
    const int t = e / cd, d = e % cd;
    const size_t o = ((size_t)b * T + t) * cd + d;
    const float m_in = mean_in[o], s_in = std_in[o];
    if (kp == 0) {
      mean_out[o] = m_in;
      std_out[o] = s_in;
      continue;
    }
    const float* src = cand + (size_t)t * step + (size_t)b * cd + d;    // + n * B * cd per candidate
    // One walk over n = 0 .. N-1 in ascending order, REFIT_WALK candidates at a time: their loads (only where the weight is
    // not zero) are all issued before the first is folded in, so a thread waits for memory once per group, not once per
    // candidate; the folds keep their order.  Every index into the register arrays is a compile-time constant (no scratch).
    auto walk = [&](auto&& fold) {
      int n = 0;
      for (; n + REFIT_WALK <= N; n += REFIT_WALK) {
        decltype(weight_of(0)) w[REFIT_WALK];
        float c[REFIT_WALK];
#pragma unroll
        for (int u = 0; u < REFIT_WALK; ++u) {
          w[u] = weight_of(n + u);
          c[u] = 0.f;
          if (w[u] != 0) c[u] = src[(size_t)(n + u) * B * cd];
        }
#pragma unroll
        for (int u = 0; u < REFIT_WALK; ++u)
          if (w[u] != 0) fold(w[u], (double)c[u]);
      }
      for (; n < N; ++n) {
        const auto w = weight_of(n);
        if (w != 0) fold(w, (double)src[(size_t)n * B * cd]);
      }
    };
    double sum = 0.0;
    walk([&](auto w, double c) {
      if constexpr (WEIGHTED) sum = add_weighted(sum, w, c);
      else sum += c;
    });
    const double m = sum / W;
    double acc = 0.0;
    walk([&](auto w, double c) {
      if constexpr (WEIGHTED) acc = add_weighted_square(acc, w, c, m);
      else acc = add_square(acc, c, m);
    });
    const double s = sqrt(acc / W);
    mean_out[o] = (float)blend(a, (double)m_in, m);
    std_out[o] = fmaxf((float)blend(a, (double)s_in, s), std_min);
  }
}

// widen * init_std as one fp32 product (the pragma as in plan_cost), then the larger of it and the shifted std.
__device__ __forceinline__ float widened(float prev, float widen, float init) {
#pragma clang fp contract(off)
  const float floor = widen * init;
  return fmaxf(prev, floor);
}

// [B][T][cd] as items of W floats (W = 4: cd % 4 == 0 and every pointer 16-byte aligned, so an item lies in one (b, t) row and the
// shifted offset is a multiple of four as well; W = 1 otherwise), one item per thread.  Step t of the output is step t + shift of
// the previous plan; past its end (the tail) the initial distribution.  keep / keep_out: both or neither.
template <int W>
__global__ __launch_bounds__(256) void plan_shift_kernel(const float* __restrict__ prev_mean, const float* __restrict__ prev_std,
                                                         const float* __restrict__ prev_keep, const float* __restrict__ init_mean,
                                                         const float* __restrict__ init_std, float* __restrict__ mean_out,
                                                         float* __restrict__ std_out, float* __restrict__ keep_out, int T, int cd,
                                                         int shift, float widen, int64_t items) {
  const int per_row = cd / W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = i * W;                             // (b * T + t) * cd + d
    const int t = (int)((i / per_row) % T);
    float m[W], s[W], k[W];
    if (t + shift < T) {
      const int64_t src = o + (int64_t)shift * cd;
      float is[W];
      ld_w<W>(prev_mean + src, m);
      ld_w<W>(prev_std + src, s);
      ld_w<W>(init_std + o, is);
#pragma unroll
      for (int j = 0; j < W; ++j) s[j] = widened(s[j], widen, is[j]);
      if (keep_out) ld_w<W>(prev_keep + src, k);
    } else {
      ld_w<W>(init_mean + o, m);
      ld_w<W>(init_std + o, s);
#pragma unroll
      for (int j = 0; j < W; ++j) k[j] = m[j];
    }
    st_w<W>(mean_out + o, m);
    st_w<W>(std_out + o, s);
    if (keep_out) st_w<W>(keep_out + o, k);
  }
}

// The aliasing rule of every launch here whose outputs are written while other threads read the inputs and write the other
// outputs: no output range may touch an input or another output.  A null pointer: not given.  own (one entry per output, -1:
// none): output i may be EXACTLY input own[i] -- the same address, where an element is read and written by one thread.
struct Range {
  const void* p;
  int64_t bytes;
};
bool ranges_overlap(const Range& x, const Range& y) {
  const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
  return x.p && y.p && a < b + (uintptr_t)y.bytes && b < a + (uintptr_t)x.bytes;
}
bool aliased(const Range* outs, int n_out, const Range* in, int n_in, const int* own = nullptr) {
  for (int i = 0; i < n_out; ++i) {
    for (int j = 0; j < n_in; ++j)
      if (!(own && own[i] == j && outs[i].p == in[j].p) && ranges_overlap(outs[i], in[j])) return true;
    for (int j = i + 1; j < n_out; ++j)
      if (ranges_overlap(outs[i], outs[j])) return true;
  }
  return false;
}

// The grid of a launch whose blocks belong to one group each: every group at least one block; past the element-wise cap the groups
// shrink in proportion to their work (work[g]: blocks of one item per thread).  first_block[g] for g <= MMDYN_FEED_GROUPS.
int split_blocks(const int64_t* work, int G, int* first_block) {
  int64_t total = 0;
  for (int g = 0; g < G; ++g) total += work[g];
  const int cap = ew_grid_cap();
  int blocks = 0;
  for (int g = 0; g < G; ++g) {
    int64_t nb = total > cap ? work[g] * cap / total : work[g];
    if (nb < 1) nb = 1;
    first_block[g] = blocks;
    blocks += (int)nb;
  }
  for (int g = G; g <= MMDYN_FEED_GROUPS; ++g) first_block[g] = blocks;
  return blocks;
}

}  // namespace

#define ST ((hipStream_t)stream)

// The launchers behind the paired entries: the one-step planner's entry is the T = 1 call of the horizon planner's, and the
// CEM refit the unweighted instantiation of the MPPI refit.

// step_cost may be null here (mmdyn_plan_select has none; mmdyn_plan_select_steps requires it before it calls).
static int launch_plan_select(double* bce_rows, double* mse_rows, const double* kl_rows, const uint8_t* tavail, const float* step_weight,
                              const float* cand, const int64_t* cand_idx, int cd, float* cost, float* step_cost, int* best,
                              float* best_cost, float* best_cond, int64_t* best_idx, int* top, float* top_cost, int K, int N, int B,
                              int T, int Tg, float pose_multiplier, float kl_weight, const float* kl_weight_dev, void* stream) {
  if (!kl_rows || !cost || !best || !best_cost) return MMDYN_ERR_NULL;
  // exactly one kind of candidates, and the winner's conditions in that kind; the list and its costs together
  if ((cand == nullptr) == (cand_idx == nullptr) || (cand != nullptr) != (best_cond != nullptr) ||
      (cand_idx != nullptr) != (best_idx != nullptr) || (top == nullptr) != (top_cost == nullptr))
    return MMDYN_ERR_NULL;
  if (N < 1 || B < 1 || T < 1 || Tg < 1 || cd < 1 || (Tg != 1 && Tg != T) || ((uintptr_t)tavail & 3)) return MMDYN_ERR_SHAPE;
  if (top && (K < 1 || K > MMDYN_PLAN_TOP_MAX)) return MMDYN_ERR_SHAPE;
  if ((int64_t)T * N * B * (cand ? cd : 1) >= (1LL << 31)) return MMDYN_ERR_RANGE;
  const uint32_t* tab = reinterpret_cast<const uint32_t*>(tavail);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(ew_grid(B)), dim3(256), 0, ST, bce_rows, mse_rows, kl_rows, tab, step_weight, cand, cand_idx, cd, cost,
                       step_cost, best, best_cost, best_cond, best_idx, top, top_cost, top ? K : 0, N, B, T, Tg, pose_multiplier, kl_weight,
                       kl_weight_dev);
  };
  if (top)
    launch(plan_select_steps_kernel<true, true>);
  else if (T == 1 && !step_weight && !step_cost)                       // (what mmdyn_plan_select asks for)
    launch(plan_select_steps_kernel<false, false>);
  else
    launch(plan_select_steps_kernel<false, true>);
  MMDYN_LAUNCH_CHECK();
}

static int launch_gather_best(const mmdyn_gather_groups* groups, int G, const int* best, int N, int B, int T, void* stream) {
  if (!groups || !best) return MMDYN_ERR_NULL;
  if (G < 1 || G > MMDYN_FEED_GROUPS || N < 1 || B < 1 || T < 1) return MMDYN_ERR_SHAPE;
  GatherStepsArgs a{};
  int64_t work[MMDYN_FEED_GROUPS];
  Range outs[MMDYN_FEED_GROUPS], in[MMDYN_FEED_GROUPS + 1];
  for (int g = 0; g < G; ++g) {
    if (!groups->src[g] || !groups->out[g]) return MMDYN_ERR_NULL;
    if (groups->row_len[g] < 1) return MMDYN_ERR_SHAPE;
    const int64_t n = (int64_t)B * groups->row_len[g];
    if (n * N * T >= (1LL << 31)) return MMDYN_ERR_RANGE;
    // (16-byte accesses are decided per step slice in the kernel; the blocks are counted for the slices that allow them)
    const bool vec = (((uintptr_t)groups->src[g] | (uintptr_t)groups->out[g]) & 15) == 0;
    a.src[g] = groups->src[g];
    a.out[g] = groups->out[g];
    a.n[g] = n;
    a.row_len[g] = groups->row_len[g];
    a.logits[g] = groups->logits[g];
    a.per_step[g] = (int)ceil_div64(vec && n >= 4 ? n / 4 : n, 256);
    work[g] = (int64_t)T * a.per_step[g];
    outs[g] = {a.out[g], n * T * 4};
    in[g] = {a.src[g], n * N * T * 4};
  }
  // the winner's rows of a group are written while other blocks read the indices and the candidates' rows of EVERY group and
  // write the other groups' rows: an out[g] may touch none of them
  in[G] = {best, (int64_t)B * 4};
  if (aliased(outs, G, in, G + 1)) return MMDYN_ERR_SHAPE;
  const int blocks = split_blocks(work, G, a.first_block);
  if (T == 1)
    hipLaunchKernelGGL(gather_best_steps_kernel<false>, dim3(blocks), dim3(256), 0, ST, a, best, G, N, T);
  else
    hipLaunchKernelGGL(gather_best_steps_kernel<true>, dim3(blocks), dim3(256), 0, ST, a, best, G, N, T);
  MMDYN_LAUNCH_CHECK();
}

// weight / ess / temperature: the weighted instantiation's only (its entry checks the temperature and the weight's alignment).
static int launch_plan_refit(bool weighted, const float* cost, const float* cand, const float* mean_in, const float* std_in,
                             float* mean_out, float* std_out, uint8_t* elite, int* count, double* weight, float* ess, int K, int N,
                             int B, int T, int cd, float temperature, float alpha, float std_min, void* stream) {
  if (!cost || !cand || !mean_in || !std_in || !mean_out || !std_out) return MMDYN_ERR_NULL;
  if (B < 1 || T < 1 || cd < 1 || N < 1 || N > MMDYN_REFIT_N_MAX || K < 1 || K > N) return MMDYN_ERR_SHAPE;
  if (!(alpha >= 0.f && alpha < 1.f) || !(std_min >= 0.f) || ((uintptr_t)weight & 7)) return MMDYN_ERR_SHAPE;
  if (weighted && (!(temperature > 0.f) || temperature == INFINITY)) return MMDYN_ERR_RANGE;
  const int64_t n = (int64_t)N * B * T * cd, row = (int64_t)B * T * cd, nb = (int64_t)N * B;
  if (n >= (1LL << 31)) return MMDYN_ERR_RANGE;
  // mean_out / std_out may be exactly their inputs (an element is read and written by one thread); every other overlap is refused
  const Range in[4] = {{cost, nb * 4}, {cand, n * 4}, {mean_in, row * 4}, {std_in, row * 4}};
  const Range outs[6] = {{mean_out, row * 4}, {std_out, row * 4}, {elite, nb}, {count, (int64_t)B * 4}, {weight, nb * 8},
                         {ess, (int64_t)B * 4}};
  const int own[6] = {2, 3, -1, -1, -1, -1};
  if (aliased(outs, 6, in, 4, own)) return MMDYN_ERR_SHAPE;
  if (weighted)
    hipLaunchKernelGGL(plan_refit_kernel<true>, dim3(B), dim3(256), 0, ST, cost, cand, mean_in, std_in, mean_out, std_out, elite, count,
                       weight, ess, K, N, B, T, cd, temperature, alpha, std_min);
  else
    hipLaunchKernelGGL(plan_refit_kernel<false>, dim3(B), dim3(256), 0, ST, cost, cand, mean_in, std_in, mean_out, std_out, elite, count,
                       weight, ess, K, N, B, T, cd, temperature, alpha, std_min);
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

extern "C" int mmdyn_rollout_feed(const mmdyn_feed_groups* groups, int G, const uint8_t* obs_avail, int B, void* stream) {
  if (!groups) return MMDYN_ERR_NULL;
  if (G < 1 || G > MMDYN_FEED_GROUPS || B < 1 || ((uintptr_t)obs_avail & 3)) return MMDYN_ERR_SHAPE;
  FeedArgs a{};
  int64_t work[MMDYN_FEED_GROUPS];
  for (int g = 0; g < G; ++g) {
    if (!groups->recon[g] || !groups->out[g]) return MMDYN_ERR_NULL;
    if (groups->row_len[g] < 1 || groups->column[g] < 0 || groups->column[g] >= MMDYN_MAX_EXPERTS) return MMDYN_ERR_SHAPE;
    const int64_t n = (int64_t)B * groups->row_len[g];
    if (n >= (1LL << 31)) return MMDYN_ERR_RANGE;
    // the next state is written while the step's outputs and the observation are read by other threads: no aliasing
    const Range out = {groups->out[g], n * 4}, in[2] = {{groups->recon[g], n * 4}, {groups->obs[g], n * 4}};
    if (aliased(&out, 1, in, 2)) return MMDYN_ERR_SHAPE;
    const bool vec = (((uintptr_t)groups->obs[g] | (uintptr_t)groups->recon[g] | (uintptr_t)groups->out[g]) & 15) == 0;
    a.recon[g] = groups->recon[g];
    a.obs[g] = groups->obs[g];
    a.out[g] = groups->out[g];
    a.n[g] = n;
    a.n4[g] = vec ? n / 4 : 0;
    a.row_len[g] = groups->row_len[g];
    a.logits[g] = groups->logits[g];
    a.column[g] = groups->column[g];
    work[g] = ceil_div64(a.n4[g] ? a.n4[g] : n, 256);           // blocks of one item per thread
  }
  const int blocks = split_blocks(work, G, a.first_block);
  hipLaunchKernelGGL(rollout_feed_kernel, dim3(blocks), dim3(256), 0, ST, a, reinterpret_cast<const uint32_t*>(obs_avail), G);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_plan_select(double* bce_rows, double* mse_rows, const double* kl_rows, const uint8_t* tavail, const float* cand,
                                 const int64_t* cand_idx, int cd, float* cost, int* best, float* best_cost, float* best_cond,
                                 int64_t* best_idx, int N, int B, float pose_multiplier, float kl_weight, const float* kl_weight_dev,
                                 void* stream) {
  return launch_plan_select(bce_rows, mse_rows, kl_rows, tavail, nullptr, cand, cand_idx, cd, cost, nullptr, best, best_cost,
                            best_cond, best_idx, nullptr, nullptr, 0, N, B, 1, 1, pose_multiplier, kl_weight, kl_weight_dev, stream);
}

extern "C" int mmdyn_gather_best(const mmdyn_gather_groups* groups, int G, const int* best, int N, int B, void* stream) {
  return launch_gather_best(groups, G, best, N, B, 1, stream);
}

extern "C" int mmdyn_ensemble_feed(const mmdyn_ensemble_groups* groups, int G, const uint8_t* obs_avail, int N, int B, void* stream) {
  if (!groups) return MMDYN_ERR_NULL;
  if (G < 1 || G > MMDYN_FEED_GROUPS || N < 1 || B < 1 || ((uintptr_t)obs_avail & 3)) return MMDYN_ERR_SHAPE;
  EnsembleArgs a{};
  int64_t work[MMDYN_FEED_GROUPS];
  for (int g = 0; g < G; ++g) {
    if (!groups->recon[g] || !groups->out[g] || !groups->mean[g]) return MMDYN_ERR_NULL;
    if (groups->row_len[g] < 1 || groups->column[g] < 0 || groups->column[g] >= MMDYN_MAX_EXPERTS) return MMDYN_ERR_SHAPE;
    if (groups->spread[g] && (!groups->var[g] || ((uintptr_t)groups->spread[g] & 7))) return MMDYN_ERR_SHAPE;
    const int64_t plane = (int64_t)B * groups->row_len[g];
    if (plane * N >= (1LL << 31)) return MMDYN_ERR_RANGE;
    // 16-byte accesses: every pointer of the group aligned and a sample stride that keeps the alignment
    const uintptr_t ptrs = (uintptr_t)groups->recon[g] | (uintptr_t)groups->obs[g] | (uintptr_t)groups->out[g] |
                           (uintptr_t)groups->mean[g] | (uintptr_t)groups->var[g];
    a.recon[g] = groups->recon[g];
    a.obs[g] = groups->obs[g];
    a.out[g] = groups->out[g];
    a.mean[g] = groups->mean[g];
    a.var[g] = groups->var[g];
    a.spread[g] = groups->spread[g];
    a.plane[g] = plane;
    a.row_len[g] = groups->row_len[g];
    a.logits[g] = groups->logits[g];
    a.column[g] = groups->column[g];
    a.vec[g] = (ptrs & 15) == 0 && plane % 4 == 0;
    work[g] = ceil_div64(a.vec[g] ? plane / 4 : plane, 256);      // blocks of one item per thread
  }
  // the outputs of a group are written while other blocks read the inputs of EVERY group and the table and write the other
  // outputs: an output may touch none of them
  Range in[2 * MMDYN_FEED_GROUPS + 1], outs[4 * MMDYN_FEED_GROUPS];
  for (int g = 0; g < G; ++g) {
    in[2 * g] = {a.recon[g], a.plane[g] * N * 4};
    in[2 * g + 1] = {a.obs[g], a.plane[g] * 4};
    outs[4 * g] = {a.out[g], a.plane[g] * N * 4};
    outs[4 * g + 1] = {a.mean[g], a.plane[g] * 4};
    outs[4 * g + 2] = {a.var[g], a.plane[g] * 4};
    outs[4 * g + 3] = {a.spread[g], (int64_t)B * 8};
  }
  in[2 * G] = {obs_avail, (int64_t)B * MMDYN_MAX_EXPERTS};
  if (aliased(outs, 4 * G, in, 2 * G + 1)) return MMDYN_ERR_SHAPE;
  const int blocks = split_blocks(work, G, a.first_block);
  hipLaunchKernelGGL(ensemble_feed_kernel, dim3(blocks), dim3(256), 0, ST, a, reinterpret_cast<const uint32_t*>(obs_avail), G, N);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_ensemble_quantiles(const mmdyn_quantile_groups* groups, int G, int Q, int N, int B, void* stream) {
  if (!groups) return MMDYN_ERR_NULL;
  if (G < 1 || G > MMDYN_FEED_GROUPS || Q < 1 || Q > MMDYN_QUANTILES_MAX || N < 1 || B < 1) return MMDYN_ERR_SHAPE;
  QuantileArgs a{};
  int64_t work[MMDYN_FEED_GROUPS];
  for (int g = 0; g < G; ++g) {
    if (!groups->src[g] || !groups->out[g]) return MMDYN_ERR_NULL;
    if (groups->row_len[g] < 1) return MMDYN_ERR_SHAPE;
  }
  for (int j = 0; j < Q; ++j) {
    if (groups->lo[j] < 0 || groups->lo[j] >= N || !(groups->frac[j] >= 0.0 && groups->frac[j] < 1.0)) return MMDYN_ERR_SHAPE;
    a.lo[j] = groups->lo[j];
    a.hi[j] = groups->lo[j] + 1 < N ? groups->lo[j] + 1 : N - 1;
    a.frac[j] = groups->frac[j];
  }
  if (N > MMDYN_QUANTILE_N_MAX) return MMDYN_ERR_RANGE;
  for (int g = 0; g < G; ++g) {
    const int64_t plane = (int64_t)B * groups->row_len[g];
    if (plane * N >= (1LL << 31) || plane * Q >= (1LL << 31)) return MMDYN_ERR_RANGE;
    a.src[g] = groups->src[g];
    a.out[g] = groups->out[g];
    a.plane[g] = plane;
    a.logits[g] = groups->logits[g];
    // 16-byte accesses: both pointers aligned and a sample / quantile stride that keeps the alignment
    a.vec[g] = (((uintptr_t)groups->src[g] | (uintptr_t)groups->out[g]) & 15) == 0 && plane % 4 == 0;
    work[g] = ceil_div64(plane, 4 * QUANTILE_CHUNK);                // in blocks of 256 threads, as the cap counts them
  }
  // the quantiles of a group are written while other blocks read the samples of EVERY group and write the other groups' quantiles
  Range outs[MMDYN_FEED_GROUPS], in[MMDYN_FEED_GROUPS];
  for (int g = 0; g < G; ++g) {
    outs[g] = {a.out[g], a.plane[g] * Q * 4};
    in[g] = {a.src[g], a.plane[g] * N * 4};
  }
  if (aliased(outs, G, in, G)) return MMDYN_ERR_SHAPE;
  int blocks = 4 * split_blocks(work, G, a.first_block);            // one wavefront per block: four for each counted block
  for (int g = 0; g <= MMDYN_FEED_GROUPS; ++g) a.first_block[g] *= 4;
  const int N4 = (N + 3) & ~3;
  const size_t lds = (size_t)(N4 > MMDYN_QUANTILES_MAX ? N4 : MMDYN_QUANTILES_MAX) * QUANTILE_CHUNK * sizeof(float);
  hipLaunchKernelGGL(ensemble_quantiles_kernel, dim3(blocks), dim3(QUANTILE_CHUNK), lds, ST, a, G, Q, N);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_plan_select_steps(double* bce_rows, double* mse_rows, const double* kl_rows, const uint8_t* tavail,
                                       const float* step_weight, const float* cand, const int64_t* cand_idx, int cd, float* cost,
                                       float* step_cost, int* best, float* best_cost, float* best_cond, int64_t* best_idx, int* top,
                                       float* top_cost, int K, int N, int B, int T, int Tg, float pose_multiplier, float kl_weight,
                                       const float* kl_weight_dev, void* stream) {
  if (!step_cost) return MMDYN_ERR_NULL;
  return launch_plan_select(bce_rows, mse_rows, kl_rows, tavail, step_weight, cand, cand_idx, cd, cost, step_cost, best, best_cost,
                            best_cond, best_idx, top, top_cost, K, N, B, T, Tg, pose_multiplier, kl_weight, kl_weight_dev, stream);
}

extern "C" int mmdyn_gather_best_steps(const mmdyn_gather_groups* groups, int G, const int* best, int N, int B, int T, void* stream) {
  return launch_gather_best(groups, G, best, N, B, T, stream);
}

extern "C" int mmdyn_plan_sample(const float* mean, const float* std, const float* eps, const float* keep, const float* lo,
                                 const float* hi, float* cand, int N, int B, int T, int cd, void* stream) {
  if (!mean || !std || !eps || !cand || (lo == nullptr) != (hi == nullptr)) return MMDYN_ERR_NULL;
  if (N < 1 || B < 1 || T < 1 || cd < 1) return MMDYN_ERR_SHAPE;
  const int64_t n = (int64_t)N * B * T * cd, row = (int64_t)B * T * cd;
  if (n >= (1LL << 31)) return MMDYN_ERR_RANGE;
  // the candidates are written while other threads read every input: no aliasing
  const Range out = {cand, n * 4};
  const Range in[6] = {{mean, row * 4}, {std, row * 4}, {eps, n * 4}, {keep, row * 4}, {lo, (int64_t)cd * 4}, {hi, (int64_t)cd * 4}};
  if (aliased(&out, 1, in, 6)) return MMDYN_ERR_SHAPE;
  const uintptr_t ptrs = (uintptr_t)mean | (uintptr_t)std | (uintptr_t)eps | (uintptr_t)keep | (uintptr_t)lo | (uintptr_t)hi |
                         (uintptr_t)cand;
  if ((ptrs & 15) == 0 && cd % 4 == 0)
    hipLaunchKernelGGL(plan_sample_kernel<4>, dim3(ew_grid(n / 4)), dim3(256), 0, ST, mean, std, eps, keep, lo, hi, cand, N, B, T, cd,
                       n / 4);
  else
    hipLaunchKernelGGL(plan_sample_kernel<1>, dim3(ew_grid(n)), dim3(256), 0, ST, mean, std, eps, keep, lo, hi, cand, N, B, T, cd, n);
  MMDYN_LAUNCH_CHECK();
}

extern "C" int mmdyn_plan_refit(const float* cost, const float* cand, const float* mean_in, const float* std_in, float* mean_out,
                                float* std_out, uint8_t* elite, int* count, int K, int N, int B, int T, int cd, float alpha,
                                float std_min, void* stream) {
  return launch_plan_refit(false, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, nullptr, nullptr, K, N, B, T, cd, 0.f,
                           alpha, std_min, stream);
}

extern "C" int mmdyn_plan_refit_weighted(const float* cost, const float* cand, const float* mean_in, const float* std_in,
                                         float* mean_out, float* std_out, uint8_t* elite, int* count, double* weight, float* ess,
                                         int K, int N, int B, int T, int cd, float temperature, float alpha, float std_min,
                                         void* stream) {
  return launch_plan_refit(true, cost, cand, mean_in, std_in, mean_out, std_out, elite, count, weight, ess, K, N, B, T, cd, temperature,
                           alpha, std_min, stream);
}

extern "C" int mmdyn_plan_shift(const float* prev_mean, const float* prev_std, const float* prev_keep, const float* init_mean,
                                const float* init_std, float* mean_out, float* std_out, float* keep_out, int B, int T, int cd,
                                int shift, float widen, void* stream) {
  if (!prev_mean || !prev_std || !init_mean || !init_std || !mean_out || !std_out || (prev_keep == nullptr) != (keep_out == nullptr))
    return MMDYN_ERR_NULL;
  if (B < 1 || T < 1 || cd < 1 || shift < 0 || shift > T || !(widen >= 0.f) || widen == INFINITY) return MMDYN_ERR_SHAPE;
  const int64_t n = (int64_t)B * T * cd;
  if (n >= (1LL << 31)) return MMDYN_ERR_RANGE;
  // every output is written while other threads read every input: no aliasing
  const Range in[5] = {{prev_mean, n * 4}, {prev_std, n * 4}, {prev_keep, n * 4}, {init_mean, n * 4}, {init_std, n * 4}};
  const Range outs[3] = {{mean_out, n * 4}, {std_out, n * 4}, {keep_out, n * 4}};
  if (aliased(outs, 3, in, 5)) return MMDYN_ERR_SHAPE;
  const uintptr_t ptrs = (uintptr_t)prev_mean | (uintptr_t)prev_std | (uintptr_t)prev_keep | (uintptr_t)init_mean |
                         (uintptr_t)init_std | (uintptr_t)mean_out | (uintptr_t)std_out | (uintptr_t)keep_out;
  if ((ptrs & 15) == 0 && cd % 4 == 0)
    hipLaunchKernelGGL(plan_shift_kernel<4>, dim3(ew_grid(n / 4)), dim3(256), 0, ST, prev_mean, prev_std, prev_keep, init_mean,
                       init_std, mean_out, std_out, keep_out, T, cd, shift, widen, n / 4);
  else
    hipLaunchKernelGGL(plan_shift_kernel<1>, dim3(ew_grid(n)), dim3(256), 0, ST, prev_mean, prev_std, prev_keep, init_mean, init_std,
                       mean_out, std_out, keep_out, T, cd, shift, widen, n);
  MMDYN_LAUNCH_CHECK();
}
