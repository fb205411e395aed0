// Multi-step rollout of the one-step dynamics model (--problem-type dyn_modeling): the predictor applied to its own output T times.
// The reference has no such loop; a caller would write MVAE.forward (vae.py:126-165) + the sigmoid of the image logits
// (problems.py:616-626 takes them to image space) once per step, on the host.  Here the T steps sit in ONE captured graph and the
// only launch a step adds to the forward is the feed below: it turns the step's decoder outputs into the NEXT step's inputs,
//   out[g][b][i] = observed(g, b) ? obs[g][b][i] : (logits[g] ? sigmoid(recon[g][b][i]) : recon[g][b][i]),
//   observed(g, b) = obs[g] != null && (obs_avail == null || obs_avail[b][column[g]] != 0),
// for up to MMDYN_FEED_GROUPS tensors at once (visual image, tactile image, pose): one dependent launch per step where the
// completion path (complete_select_kernel, poe_avail.hip) takes one per modality.  out is the trajectory slot of the step, which
// the next step's encoders read in place.
//   - The element scheme is complete_select_kernel's: quads [0, n4) of the flat [B * row_len] array by 16-byte accesses (n4 = 0
//     when one of the group's pointers is not 16-byte aligned), the rest one by one; a quad inside one row loads only the side it
//     takes (the other may hold NaN / Inf), a quad that straddles rows (row_len % 4 != 0: the 7-DoF pose) loads both and selects
//     per element.  The arithmetic is sigmoid_f of poe_avail.hip, so a group's output has the bits of mmdyn_complete_select.
//   - A block belongs to ONE group (first_block[] is an exclusive scan of the groups' block counts, which follow their quad
//     counts: the pose group is 7 * B floats next to 12288 * B), so the group's pointers and flags are block-uniform and the
//     row's presence is wave-uniform wherever 256 consecutive floats lie in one row.
//   - Memory-bound, no LDS, no atomics, no scratch.
#include "common.h"

namespace {

struct FeedArgs {
  const float* recon[MMDYN_FEED_GROUPS];
  const float* obs[MMDYN_FEED_GROUPS];
  float* out[MMDYN_FEED_GROUPS];
  int64_t n[MMDYN_FEED_GROUPS], n4[MMDYN_FEED_GROUPS];
  int row_len[MMDYN_FEED_GROUPS], logits[MMDYN_FEED_GROUPS], column[MMDYN_FEED_GROUPS];
  int first_block[MMDYN_FEED_GROUPS + 1];
};

__device__ __forceinline__ bool has(uint32_t word, int m) { return ((word >> (8 * m)) & 0xffu) != 0u; }

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

__global__ __launch_bounds__(256) void rollout_feed_kernel(const FeedArgs a, const uint32_t* __restrict__ avail, int G) {
  int g = 0;
#pragma unroll
  for (int k = 1; k < MMDYN_FEED_GROUPS; ++k)
    if (k < G && (int)blockIdx.x >= a.first_block[k]) g = k;
  const float* __restrict__ recon = a.recon[g];
  const float* __restrict__ x = a.obs[g];
  float* __restrict__ out = a.out[g];
  const int64_t n = a.n[g], n4 = a.n4[g];
  const int row_len = a.row_len[g], logits = a.logits[g], column = a.column[g];
  const int64_t tid = (int64_t)((int)blockIdx.x - a.first_block[g]) * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)(a.first_block[g + 1] - a.first_block[g]) * blockDim.x;
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
        const bool present = x != nullptr && (!avail || has(avail[b], column));
        v[k] = present ? xv[k] : (logits ? sigmoid_f(r[k]) : r[k]);
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
      if (logits) v = sigmoid_f(v);
    }
    out[i] = v;
  }
}

bool overlap(const float* p, const float* q, int64_t n) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q, bytes = (uintptr_t)n * sizeof(float);
  return q != nullptr && a < b + bytes && b < a + bytes;
}

}  // namespace

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
  hipLaunchKernelGGL(rollout_feed_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a,
                     reinterpret_cast<const uint32_t*>(obs_avail), G);
  MMDYN_LAUNCH_CHECK();
}
