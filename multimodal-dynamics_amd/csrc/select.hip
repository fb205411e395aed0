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
// Memory-bound, no LDS, no atomics, no scratch.
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

bool overlap(const float* p, const float* q, int64_t n) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q, bytes = (uintptr_t)n * sizeof(float);
  return q != nullptr && a < b + bytes && b < a + bytes;
}

}  // namespace

#define ST ((hipStream_t)stream)

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
  int64_t work[MMDYN_FEED_GROUPS], total = 0;
  for (int g = 0; g < G; ++g) {
    if (!groups->recon[g] || !groups->out[g]) return MMDYN_ERR_NULL;
    if (groups->row_len[g] < 1 || groups->column[g] < 0 || groups->column[g] >= MMDYN_MAX_EXPERTS) return MMDYN_ERR_SHAPE;
    const int64_t n = (int64_t)B * groups->row_len[g];
    if (n >= (1LL << 31)) return MMDYN_ERR_RANGE;
    // the next state is written while the step's outputs and the observation are read by other threads: no aliasing
    if (overlap(groups->out[g], groups->recon[g], n) || overlap(groups->out[g], groups->obs[g], n)) return MMDYN_ERR_SHAPE;
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
    total += work[g];
  }
  // every group at least one block; past the element-wise cap the groups shrink in proportion to their work
  const int cap = ew_grid_cap();
  int blocks = 0;
  for (int g = 0; g < G; ++g) {
    int64_t nb = total > cap ? work[g] * cap / total : work[g];
    if (nb < 1) nb = 1;
    a.first_block[g] = blocks;
    blocks += (int)nb;
  }
  for (int g = G; g <= MMDYN_FEED_GROUPS; ++g) a.first_block[g] = blocks;
  hipLaunchKernelGGL(rollout_feed_kernel, dim3(blocks), dim3(256), 0, ST, a, reinterpret_cast<const uint32_t*>(obs_avail), G);
  MMDYN_LAUNCH_CHECK();
}
