// k_returns.hip - discounted returns and GAE advantages of a rollout's [T, B] streams, one
// backward pass in one launch, aware of the episode ends INSIDE the rollout (the rollout kernels
// rebuild a finished environment on the spot, so a return must not leak across a `done`).
//
// The rule (include/campx_hip.h has it in full; tests/returns_reference.py restates it in numpy):
// for t = T-1 down to 0, per environment, every operation an f32 operation rounded on its own
//     r = isnan(reward) ? 0 : reward          c = gamma * discount     (gamma without a discount)
//     G = done ? r : r + c * G_next
//     delta = (done ? r : r + c * v_next) - v
//     A = done ? delta : delta + (c * lam) * A_next
//
// A lane per environment walks its column backwards (streams.hip.h: walk_back() and its Chunk,
// the head of the rule).  Like the update pass this is bound by latency, not bandwidth (13-21
// bytes per environment-frame, two dependent operations per frame and stream): what the chain of
// a frame needs from memory does not depend on the chain, so a chunk of eight frames issues ALL
// its loads - up to 32 per lane, coalesced along B - before its arithmetic starts, and everything
// that does not depend on the frame after (r, c, c * lam, delta) is computed off the chain.
// Stores are plain: the learner reads them next.

#include "streams.hip.h"

#include <cmath>

namespace campx_impl {

struct ReturnsParams {
  float gamma, lam;
  int32_t T;
  int64_t B;
  // elements from one frame's row to the next, per stream
  int64_t p_reward, p_done, p_discount, p_values, p_returns, p_adv;
};

template <bool kDiscount, bool kValues>
__global__ __launch_bounds__(kStreamThreads) void returns_kernel(
    ReturnsParams rp, const float* __restrict__ reward, const uint8_t* __restrict__ done,
    const float* __restrict__ discount, const float* __restrict__ values,
    const float* __restrict__ bootstrap, float* __restrict__ returns, float* __restrict__ adv) {
  const int64_t env = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
  if (env >= rp.B) return;
  const float boot = bootstrap ? bootstrap[env] : 0.0f;
  const float gamma = rp.gamma, lam = rp.lam;
  float G = boot, A = 0.0f, v_after = boot;     // of the frame after the one in hand
  walk_back(rp.T, [&](auto chunk) {
    float r[kStreamChunk], c[kStreamChunk], v[kStreamChunk];
    uint8_t d[kStreamChunk];
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      const int64_t t = chunk.load_t(j);
      r[j] = reward[t * rp.p_reward + env];
      d[j] = done[t * rp.p_done + env];
      c[j] = kDiscount ? discount[t * rp.p_discount + env] : 1.0f;
      v[j] = kValues ? values[t * rp.p_values + env] : 0.0f;
    }
    // off the chain: the reward that counts, the factor, and - with values - delta and c * lam
    float delta[kStreamChunk], cl[kStreamChunk];
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      r[j] = reward_that_counts(r[j]);
      c[j] = frame_factor<kDiscount>(gamma, c[j]);
      if (kValues) {
        delta[j] = __fsub_rn(CAMPX_UNLESS_DONE(d[j], r[j], c[j], j == 0 ? v_after : v[j - 1]), v[j]);
        cl[j] = __fmul_rn(c[j], lam);
      }
    }
    // the chain: a multiply and an add per frame and stream
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      if (chunk.has(j)) {
        G = CAMPX_UNLESS_DONE(d[j], r[j], c[j], G);
        returns[(int64_t)chunk.t(j) * rp.p_returns + env] = G;
        if (kValues) {
          A = CAMPX_UNLESS_DONE(d[j], delta[j], cl[j], A);
          adv[(int64_t)chunk.t(j) * rp.p_adv + env] = A;
          v_after = v[j];
        }
      }
    }
  });
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_returns_launch(const CampxReturns* r, int64_t B, int32_t T, void* stream) {
  if (!r || !r->reward || !r->done || !r->returns || !stream_shape_ok(B, T)) return CAMPX_EINVAL;
  if ((r->values == nullptr) != (r->advantages == nullptr)) return CAMPX_EINVAL;
  if (!std::isfinite(r->gamma) || !std::isfinite(r->lam)) return CAMPX_EINVAL;
  if (!all_aligned(4, {r->reward, r->discount, r->values, r->bootstrap, r->returns, r->advantages}))
    return CAMPX_EINVAL;
  if (!pitches_ok(B, T, {{r->reward, r->reward_pitch}, {r->done, r->done_pitch},
                         {r->discount, r->discount_pitch}, {r->values, r->values_pitch},
                         {r->returns, r->returns_pitch}, {r->advantages, r->advantages_pitch}}))
    return CAMPX_EINVAL;
  const ReturnsParams rp{r->gamma, r->lam, T, B, r->reward_pitch, r->done_pitch, r->discount_pitch,
                         r->values_pitch, r->returns_pitch, r->advantages_pitch};
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)stream_blocks(B));
#define CAMPX_RETURNS(DISCOUNT, VALUES)                                                         \
  hipLaunchKernelGGL((returns_kernel<DISCOUNT, VALUES>), grid, dim3(kStreamThreads), 0, hs, rp, \
                     r->reward, r->done, r->discount, r->values, r->bootstrap, r->returns,      \
                     r->advantages)
  if (r->discount && r->values) CAMPX_RETURNS(true, true);
  else if (r->discount) CAMPX_RETURNS(true, false);
  else if (r->values) CAMPX_RETURNS(false, true);
  else CAMPX_RETURNS(false, false);
#undef CAMPX_RETURNS
  return launch_status();
}

}  // extern "C"
