// streams.hip.h - what the kernels that reduce a rollout's [T, B] streams (k_returns, k_vtrace,
// k_sums) and their launchers agree on, each said once: host side the shape, pitch and alignment
// tests of a launch and the rule that stages a float table in LDS; device side the walk over the
// frames in chunks of eight, the head of the returns rule, the (state, action) range test and bin,
// table staging and the per-workgroup counters.  Every device helper is __forceinline__, takes
// values and holds neither a barrier nor an early return: those stay visible in the kernels.
#ifndef CAMPX_STREAMS_HIP_H_
#define CAMPX_STREAMS_HIP_H_

#include "campx_common.hip.h"

#include <initializer_list>

namespace campx_impl {

constexpr int kStreamThreads = 256;      // a lane per environment
constexpr int kStreamChunk = 8;          // frames whose loads are all issued before any arithmetic
// dynamic LDS of a workgroup: below the 64 KiB a launch may have without an attribute (the
// counters are static LDS on top), and three workgroups of it still share a CU's 160 KiB
constexpr int64_t kStreamLdsBudget = CAMPX_SUMS_LDS_BUDGET;
typedef unsigned long long u64;

// ---------------------------------------------------------------------------- host side

inline bool stream_shape_ok(int64_t B, int32_t T) { return B >= 1 && B <= (1ll << 31) && T >= 1; }
inline int64_t stream_blocks(int64_t B) { return (B + kStreamThreads - 1) / kStreamThreads; }

inline bool all_aligned(uintptr_t n, std::initializer_list<const void*> pointers) {
  for (const void* p : pointers)
    if (!aligned_to(p, n)) return false;
  return true;
}

// The rows of a launch's streams: frame t's row is `pitch` elements after frame t - 1's, at least
// B and at most 2^40 / T - except that a single frame never uses its pitch.  A NULL stream passes.
struct StreamRows {
  const void* p;
  int64_t pitch;
};
inline bool pitches_ok(int64_t B, int32_t T, std::initializer_list<StreamRows> streams) {
  const int64_t least = T > 1 ? B : 0, most = (1ll << 40) / T;
  for (const StreamRows& s : streams)
    if (s.p && (s.pitch < least || s.pitch > most)) return false;
  return true;
}

// A float table of `entries` may be staged in LDS when its bytes fit the budget, and is when it
// also costs a workgroup no more loads than the `frames` frames each of its lanes looks up.
inline bool table_fits_lds(int64_t entries) { return entries * 4 <= kStreamLdsBudget; }
inline bool table_staged(int64_t entries, int64_t frames) {
  return table_fits_lds(entries) && entries <= (int64_t)kStreamThreads * frames;
}

// ---------------------------------------------------------------------------- device side

// One chunk of a walk: frames t0, t0 + kStep, ... t0 + 7 * kStep (kStep -1: backwards).  kFull:
// the walk has all of them; else those past `edge` - below it backwards, from it on forwards -
// are loaded from the walk's last frame (no branch between the loads) and left out.
template <bool kFull, int kStep>
struct Chunk {
  int32_t t0, edge;
  __device__ __forceinline__ int32_t t(int j) const { return t0 + kStep * j; }
  __device__ __forceinline__ bool has(int j) const {
    return kFull || (kStep > 0 ? t(j) < edge : t(j) >= edge);
  }
  __device__ __forceinline__ int64_t load_t(int j) const {
    return has(j) ? t(j) : (kStep > 0 ? edge - 1 : edge);
  }
};

// The two walks, `body` a generic lambda that takes the Chunk: frames T - 1 down to 0, and frames
// t_begin up to t_end - 1.
template <class Body>
__device__ __forceinline__ void walk_back(int32_t T, const Body& body) {
  int32_t t1 = T;
  for (; t1 >= kStreamChunk; t1 -= kStreamChunk) body(Chunk<true, -1>{t1 - 1, 0});
  if (t1 > 0) body(Chunk<false, -1>{t1 - 1, 0});
}
template <class Body>
__device__ __forceinline__ void walk_forward(int32_t t_begin, int32_t t_end, const Body& body) {
  int32_t t = t_begin;
  for (; t_end - t >= kStreamChunk; t += kStreamChunk) body(Chunk<true, 1>{t, t_end});
  if (t < t_end) body(Chunk<false, 1>{t, t_end});
}

// The head of the returns rule (include/campx_hip.h), every operation rounded on its own: the
// reward that counts, the frame's factor, and x + k * next unless the frame ends its episode - the
// one-step target, and each chain's step.  That one is a macro, not a function: as a function it
// reaches the chain as a select where the spelled-out choice is a branch that the frame's factor
// sinks into, and returns_kernel<true, false> goes from 37 VGPRs to 67 and loses a wave (NOTES.md).
__device__ __forceinline__ float reward_that_counts(float reward) { return reward == reward ? reward : 0.0f; }
template <bool kDiscount>
__device__ __forceinline__ float frame_factor(float gamma, float discount) {
  return kDiscount ? __fmul_rn(gamma, discount) : gamma;
}
#define CAMPX_UNLESS_DONE(done, x, k, next) ((done) ? (x) : __fadd_rn((x), __fmul_rn((k), (next))))

// A frame's ids against a table of S states and A actions (negative ids are large as unsigned;
// `&`: no load may hide behind a short circuit), and the bin they name, in 32 or 64 bits.
__device__ __forceinline__ bool ids_in_range(int32_t state, int8_t action, uint32_t S, uint32_t A) {
  return ((uint32_t)state < S) & ((uint32_t)(int32_t)action < A);
}
template <typename Index>
__device__ __forceinline__ Index bin_of(int32_t state, int8_t action, uint32_t A) {
  return (Index)(uint32_t)state * A + (uint32_t)(int32_t)action;
}

// `n` floats of `table` to `lds`, by the whole workgroup; the kernel's barrier follows.
__device__ __forceinline__ void stage_table(float* lds, const float* __restrict__ table, uint32_t n) {
  for (uint32_t i = threadIdx.x; i < n; i += kStreamThreads) lds[i] = table[i];
}

// The workgroup's two counters of frames it could not take, u64 block[2] in static LDS that the
// kernel zeroes before its first barrier: each lane's counts into them, and - after a barrier of
// the kernel's - thread 0 adds those that are not zero to the global ones (either may be NULL).
__device__ __forceinline__ void count_in_block(u64* block, u64 a, u64 b) {
  if (a) __hip_atomic_fetch_add(&block[0], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (b) __hip_atomic_fetch_add(&block[1], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void report_block_counts(const u64* block, u64* ga, u64* gb) {
  if (threadIdx.x == 0) {
    if (ga && block[0]) __hip_atomic_fetch_add(ga, block[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gb && block[1]) __hip_atomic_fetch_add(gb, block[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace campx_impl

#endif  // CAMPX_STREAMS_HIP_H_
