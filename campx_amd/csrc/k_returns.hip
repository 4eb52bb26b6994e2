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
// A lane per environment walks its column backwards.  Like the update pass this is bound by
// latency, not bandwidth (13-21 bytes per environment-frame, two dependent operations per frame
// and stream): what the chain of a frame needs from memory does not depend on the chain, so a
// chunk of eight frames issues ALL its loads - up to 32 per lane, coalesced along B - before its
// arithmetic starts, and everything that does not depend on the frame after (r, c, c * lam,
// delta) is computed off the chain.  Stores are plain: the learner reads them next.

#include "campx_common.hip.h"

#include <cmath>
#include <type_traits>

namespace campx_impl {

constexpr int kReturnsThreads = 256;
constexpr int kReturnsChunk = 8;

struct ReturnsParams {
  float gamma, lam;
  int32_t T;
  int64_t B;
  // elements from one frame's row to the next, per stream
  int64_t p_reward, p_done, p_discount, p_values, p_returns, p_adv;
};

template <bool kDiscount, bool kValues>
__global__ __launch_bounds__(kReturnsThreads) void returns_kernel(
    ReturnsParams rp, const float* __restrict__ reward, const uint8_t* __restrict__ done,
    const float* __restrict__ discount, const float* __restrict__ values,
    const float* __restrict__ bootstrap, float* __restrict__ returns, float* __restrict__ adv) {
  const int64_t env = (int64_t)blockIdx.x * kReturnsThreads + threadIdx.x;
  if (env >= rp.B) return;
  const float boot = bootstrap ? bootstrap[env] : 0.0f;
  const float gamma = rp.gamma, lam = rp.lam;
  float G = boot, A = 0.0f, v_after = boot;     // of the frame after the one in hand
  // One chunk: frames t1 - 1 down to t1 - 8.  kFull: all of them exist; else those below 0 are
  // loaded from frame 0 (no branch between the loads) and skipped.
  auto chunk = [&](auto full_tag, int t1) {
    constexpr bool kFull = decltype(full_tag)::value;
    float r[kReturnsChunk], c[kReturnsChunk], v[kReturnsChunk];
    uint8_t d[kReturnsChunk];
#pragma unroll
    for (int j = 0; j < kReturnsChunk; ++j) {
      int t = t1 - 1 - j;
      if (!kFull) t = t < 0 ? 0 : t;
      r[j] = reward[(int64_t)t * rp.p_reward + env];
      d[j] = done[(int64_t)t * rp.p_done + env];
      c[j] = kDiscount ? discount[(int64_t)t * rp.p_discount + env] : 1.0f;
      v[j] = kValues ? values[(int64_t)t * rp.p_values + env] : 0.0f;
    }
    // off the chain: the reward that counts, the factor, and - with values - delta and c * lam
    float delta[kReturnsChunk], cl[kReturnsChunk];
#pragma unroll
    for (int j = 0; j < kReturnsChunk; ++j) {
      r[j] = r[j] == r[j] ? r[j] : 0.0f;
      c[j] = kDiscount ? __fmul_rn(gamma, c[j]) : gamma;
      if (kValues) {
        const float v_next = j == 0 ? v_after : v[j - 1];
        const float q = d[j] ? r[j] : __fadd_rn(r[j], __fmul_rn(c[j], v_next));
        delta[j] = __fsub_rn(q, v[j]);
        cl[j] = __fmul_rn(c[j], lam);
      }
    }
    // the chain: a multiply and an add per frame and stream
#pragma unroll
    for (int j = 0; j < kReturnsChunk; ++j) {
      const int t = t1 - 1 - j;
      if (kFull || t >= 0) {
        G = d[j] ? r[j] : __fadd_rn(r[j], __fmul_rn(c[j], G));
        returns[(int64_t)t * rp.p_returns + env] = G;
        if (kValues) {
          A = d[j] ? delta[j] : __fadd_rn(delta[j], __fmul_rn(cl[j], A));
          adv[(int64_t)t * rp.p_adv + env] = A;
          v_after = v[j];
        }
      }
    }
  };
  int t1 = rp.T;
  for (; t1 >= kReturnsChunk; t1 -= kReturnsChunk) chunk(std::true_type{}, t1);
  if (t1 > 0) chunk(std::false_type{}, t1);
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_returns_launch(const CampxReturns* r, int64_t B, int32_t T, void* stream) {
  if (!r || !r->reward || !r->done || !r->returns || B <= 0 || B > (1ll << 31) ||
      T <= 0)
    return CAMPX_EINVAL;
  if ((r->values == nullptr) != (r->advantages == nullptr)) return CAMPX_EINVAL;
  if (!std::isfinite(r->gamma) || !std::isfinite(r->lam)) return CAMPX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(r->reward) | reinterpret_cast<uintptr_t>(r->discount) |
       reinterpret_cast<uintptr_t>(r->values) | reinterpret_cast<uintptr_t>(r->bootstrap) |
       reinterpret_cast<uintptr_t>(r->returns) | reinterpret_cast<uintptr_t>(r->advantages)) & 3)
    return CAMPX_EINVAL;
  // (a single frame never uses its pitch)
  const int64_t least = T > 1 ? B : 0, most = (1ll << 40) / T;
  auto pitch_ok = [&](const void* p, int64_t pitch) { return !p || (pitch >= least && pitch <= most); };
  if (!pitch_ok(r->reward, r->reward_pitch) || !pitch_ok(r->done, r->done_pitch) ||
      !pitch_ok(r->discount, r->discount_pitch) || !pitch_ok(r->values, r->values_pitch) ||
      !pitch_ok(r->returns, r->returns_pitch) || !pitch_ok(r->advantages, r->advantages_pitch))
    return CAMPX_EINVAL;
  ReturnsParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.gamma = r->gamma;
  rp.lam = r->lam;
  rp.T = T;
  rp.B = B;
  rp.p_reward = r->reward_pitch;
  rp.p_done = r->done_pitch;
  rp.p_discount = r->discount_pitch;
  rp.p_values = r->values_pitch;
  rp.p_returns = r->returns_pitch;
  rp.p_adv = r->advantages_pitch;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((B + kReturnsThreads - 1) / kReturnsThreads));
#define CAMPX_RETURNS(DISCOUNT, VALUES)                                                          \
  hipLaunchKernelGGL((returns_kernel<DISCOUNT, VALUES>), grid, dim3(kReturnsThreads), 0, hs, rp, \
                     r->reward, r->done, r->discount, r->values, r->bootstrap, r->returns,       \
                     r->advantages)
  if (r->discount && r->values) CAMPX_RETURNS(true, true);
  else if (r->discount) CAMPX_RETURNS(true, false);
  else if (r->values) CAMPX_RETURNS(false, true);
  else CAMPX_RETURNS(false, false);
#undef CAMPX_RETURNS
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CAMPX_OK : hip_failed(e);
}

}  // extern "C"
