// k_policy.hip - closed-loop rollouts of the state-table tier: the update pass of k_wide.hip
// (a lane per environment walking (state, action) -> state) with every frame's action SAMPLED
// on the chain, from a policy given as a table over the game's states, weights[S][5].
//
// The sampling rule (include/campx_hip.h has it in full; tests/policy_reference.py restates it):
// one Philox4x32-10 block per environment and group of four frames, frame f takes word f & 3;
// u = (word >> 8) * 2^-24; thresholds c0 = w0, c1 = c0 + w1 ... c4 in f32, in that order;
// r = u * c4; action = (r >= c0) + (r >= c1) + (r >= c2) + (r >= c3).
//
// What a frame adds to wide_update_kernel's chain is one dependent read: the state's row of
// THRESHOLDS (the sums are taken once per state when the table is staged in LDS, not once per
// frame), then the entry of (state, action) as before.  The random words do not depend on the
// state: both blocks of a chunk of eight frames are computed before its chain starts.
//
// k_population.hip holds this kernel's twin for a population of policies - the same frame loop with
// two per-lane constants added.  A change to the sampling or to the chunk logic here is made there too.

#include "wide_table.hip.h"

#include <type_traits>

namespace campx_impl {

constexpr int kPolicyThreads = 256;
constexpr int kPolicyChunk = 8;     // frames per chunk: two Philox blocks

struct PolicyParams {
  int32_t n_states, n_planes;
  int32_t has_dcodes;          // some entry of the table carries a discount code
  uint32_t key0, key1;         // seed & 0xffffffff, seed >> 32
  float discounts[16];
  int64_t plane;               // entries from one plane of the trace to the next (T x row pitch)
  int64_t first_frame;         // absolute number of the launch's frame 0
};

// kLds: the state table AND the thresholds sit in LDS; else both are read through L1 / L2 (the
// thresholds are then summed from the weights at every frame).  kStates: the row each frame
// sampled from is written out.
template <bool kLds, bool kPerf, bool kStates>
__global__ __launch_bounds__(kPolicyThreads) void wide_policy_update_kernel(
    PolicyParams pp, const uint2* __restrict__ g_entries, const u32x4* __restrict__ g_cells,
    const int8_t* __restrict__ g_perf, const float* __restrict__ g_policy,
    int32_t* __restrict__ state, CampxState st, CampxOutputs out,
    int8_t* __restrict__ actions_out, int32_t* __restrict__ states_out, int64_t B, int32_t T,
    int32_t reset_first) {
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS, K = pp.n_planes;
  const uint2* entries = g_entries;
  const u32x4* cells = g_cells;
  const int8_t* perf_tab = g_perf;
  const float* thresholds = nullptr;
  if (kLds) {
    uint2* l_entries = lds_tables;
    u32x4* l_cells = reinterpret_cast<u32x4*>(l_entries + n_entries + (n_entries & 1));   // 16-byte aligned
    int8_t* l_perf = reinterpret_cast<int8_t*>(l_cells + S);
    float* l_thr = reinterpret_cast<float*>(l_perf + (kPerf ? (n_entries + 15) & ~15 : 0));
    for (int i = threadIdx.x; i < n_entries; i += kPolicyThreads) l_entries[i] = g_entries[i];
    for (int i = threadIdx.x; i < S; i += kPolicyThreads) l_cells[i] = g_cells[i];
    if (kPerf)
      for (int i = threadIdx.x; i < n_entries; i += kPolicyThreads) l_perf[i] = g_perf[i];
    for (int i = threadIdx.x; i < S; i += kPolicyThreads) {
      float c[5];
      policy_thresholds(g_policy + i * CAMPX_N_ACTIONS, c);
#pragma unroll
      for (int k = 0; k < 5; ++k) l_thr[i * CAMPX_N_ACTIONS + k] = c[k];
    }
    entries = l_entries;
    cells = l_cells;
    perf_tab = l_perf;
    thresholds = l_thr;
  }
  if (threadIdx.x < 16) discounts[threadIdx.x] = pp.discounts[threadIdx.x];
  __syncthreads();

  const int64_t env = (int64_t)blockIdx.x * kPolicyThreads + threadIdx.x;
  if (env >= B) return;
  uint32_t now = 0;
  int over = 0;
  float ret = 0.0f;
  if (!reset_first) {
    now = (uint32_t)state[env];
    now = now < (uint32_t)S ? now : 0u;      // (a state index from outside: start over)
    over = st.done[env];
    if (st.ret) ret = st.ret[env];
  }
  uint32_t from = over ? 0u : now;
  uint16_t* trace = reinterpret_cast<uint16_t*>(out.trace);
  const int64_t P = row_pitch(out, B), plane = pp.plane;
  int bad = 0;
  // Chunks start on a multiple of four ABSOLUTE frames, so that frame j of a chunk takes word
  // j & 3 of block j >> 2 whatever first_frame is: the first chunk begins up to three frames
  // before the launch's frame 0 (frames that are skipped).
  const int lead = (int)(pp.first_frame & 3);
  const uint64_t group0 = (uint64_t)(pp.first_frame - lead) >> 2;
  int64_t at = env - (int64_t)lead * P;            // element (frame, env) of the [T, P] streams
  // One chunk of frames.  `plain_tag` as in wide_update_kernel: 0 = the general chunk (any frame
  // may lie outside the launch, any stream may be missing, discount codes); k = 1 .. 8 = a whole
  // chunk of a game with k planes, no test inside.
  auto chunk = [&](auto plain_tag, int t0) {
    constexpr int kThings = decltype(plain_tag)::value;
    constexpr bool kPlain = kThings > 0;
    uint32_t x[kPolicyChunk];
    const uint64_t g = group0 + (uint64_t)((t0 + lead) >> 2);
    philox4x32_10((uint32_t)env, (uint32_t)g, (uint32_t)(g >> 32), 0u, pp.key0, pp.key1, x);
    philox4x32_10((uint32_t)env, (uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), 0u, pp.key0, pp.key1,
                  x + 4);
#pragma unroll
    for (int j = 0; j < kPolicyChunk; ++j) {
      if (kPlain || (t0 + j >= 0 && t0 + j < T)) {
        float c[5];
        if (kLds) {
#pragma unroll
          for (int k = 0; k < 5; ++k) c[k] = thresholds[from * CAMPX_N_ACTIONS + k];
        } else {
          policy_thresholds(g_policy + from * CAMPX_N_ACTIONS, c);
        }
        const float u = (float)(x[j] >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
        const float r = u * c[4];
        const uint32_t a = (uint32_t)(r >= c[0]) + (uint32_t)(r >= c[1]) + (uint32_t)(r >= c[2]) +
                           (uint32_t)(r >= c[3]);
        bad += c[4] == 0.0f;
        actions_out[at] = (int8_t)a;
        if (kStates) states_out[at] = (int32_t)from;
        const uint32_t idx = from * CAMPX_N_ACTIONS + a;
        const uint2 e = entries[idx];
        now = entry_next(e.y);
        const uint32_t done = entry_done(e.y), dcode = entry_dcode(e.y);
        from = done ? 0u : now;                      // the chain: state -> thresholds -> entry -> state
        const u32x4 cs = cells[now];                 // where things show in the state reached
        trace[at] = (uint16_t)cs.x;
        if (kPlain) {
          const uint32_t w[4] = {cs.x, cs.y, cs.z, cs.w};
#pragma unroll
          for (int d = 1; d < kThings; ++d)
            trace[at + d * plane] = (uint16_t)(w[d >> 1] >> (16 * (d & 1)));
        }
        if (!kPlain && K > 1) {
          uint16_t* tk = trace + at + plane;
          tk[0] = (uint16_t)(cs.x >> 16);
          if (K > 2) tk[plane] = (uint16_t)cs.y;
          if (K > 3) tk[2 * plane] = (uint16_t)(cs.y >> 16);
          if (K > 4) tk[3 * plane] = (uint16_t)cs.z;
          if (K > 5) tk[4 * plane] = (uint16_t)(cs.z >> 16);
          if (K > 6) tk[5 * plane] = (uint16_t)cs.w;
          if (K > 7) tk[6 * plane] = (uint16_t)(cs.w >> 16);
        }
        if (kPlain) {
          out.reward[at] = __uint_as_float(e.x);
          out.discount[at] = done ? 0.0f : 1.0f;
          out.done[at] = (uint8_t)done;
        } else {
          if (out.reward) out.reward[at] = __uint_as_float(e.x);
          if (out.discount) out.discount[at] = __uint_as_float(discount_bits(discounts, dcode, done));
          if (out.done) out.done[at] = (uint8_t)done;
        }
        if (kPerf && out.perf) out.perf[at] = perf_tab[idx];
        ret = (over ? 0.0f : ret) + real_reward(__uint_as_float(e.x));
        over = (int)done;
      }
      at += P;
    }
  };
  const bool plain = !pp.has_dcodes && out.reward && out.discount && out.done &&
                     (!kPerf || out.perf);
  for (int t0 = -lead; t0 < T; t0 += kPolicyChunk) {
    if (plain && t0 >= 0 && t0 + kPolicyChunk <= T) {
      switch (K) {      // (one uniform branch per chunk of eight frames)
        case 1: chunk(std::integral_constant<int, 1>{}, t0); break;
        case 2: chunk(std::integral_constant<int, 2>{}, t0); break;
        case 3: chunk(std::integral_constant<int, 3>{}, t0); break;
        case 4: chunk(std::integral_constant<int, 4>{}, t0); break;
        case 5: chunk(std::integral_constant<int, 5>{}, t0); break;
        case 6: chunk(std::integral_constant<int, 6>{}, t0); break;
        case 7: chunk(std::integral_constant<int, 7>{}, t0); break;
        default: chunk(std::integral_constant<int, 8>{}, t0); break;
      }
    } else {
      chunk(std::integral_constant<int, 0>{}, t0);
    }
  }
  state[env] = (int32_t)now;
  st.done[env] = (uint8_t)over;
  if (st.ret) st.ret[env] = ret;
  report_bad(out.bad_count, out.bad_flag, bad);      // (bad ROWS, on the rollout's counter)
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_policy_update_launch(const CampxWideSpec* s, const void* tables_dev,
                                        CampxState st, const float* policy, uint64_t seed,
                                        int64_t first_frame, CampxOutputs out, int8_t* actions_out,
                                        int32_t* states_out, int64_t B, int32_t T,
                                        int32_t reset_first, void* stream) {
  if (!s || !tables_dev || !st.pos || !st.done || !policy || !out.trace || !actions_out || B <= 0 ||
      T <= 0)
    return CAMPX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out.trace) & 1) || (reinterpret_cast<uintptr_t>(st.pos) & 3) ||
      (reinterpret_cast<uintptr_t>(policy) & 3) || (reinterpret_cast<uintptr_t>(states_out) & 3))
    return CAMPX_EINVAL;
  if (out.scalar_pitch && out.scalar_pitch < B) return CAMPX_EINVAL;
  // (the environment is one 32-bit word of the Philox counter; frames count up to 2^63 - 1)
  if (B > 0xffffffffll || first_frame < 0 || first_frame > INT64_MAX - T) return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  if (out.perf && !s->has_perf) return CAMPX_EINVAL;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const WideLayout w = wide_layout(*s);
  PolicyParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.n_states = s->n_states;
  pp.n_planes = w.n_planes;
  pp.discounts[0] = 1.0f;
  for (int i = 1; i < 16; ++i) pp.discounts[i] = s->discount_list[i];
  pp.has_dcodes = s->any_dcode;
  pp.key0 = (uint32_t)seed;
  pp.key1 = (uint32_t)(seed >> 32);
  pp.plane = (int64_t)T * row_pitch(out, B);
  pp.first_frame = first_frame;
  const char* blob = static_cast<const char*>(tables_dev);
  const uint2* entries = reinterpret_cast<const uint2*>(blob);
  const u32x4* cells = reinterpret_cast<const u32x4*>(blob + w.cells_off);
  const int8_t* perf = reinterpret_cast<const int8_t*>(blob + w.perf_off);
  int32_t* state = reinterpret_cast<int32_t*>(st.pos);
  // wide_update_kernel's size rule, with the thresholds (five floats per state) counted in
  const size_t want = (size_t)(w.cells_off) + (size_t)s->n_states * sizeof(u32x4) +
                      (out.perf ? (size_t)((w.n_entries + 15) & ~(int64_t)15) : 0) +
                      (size_t)w.n_entries * sizeof(float);
  const bool in_lds = want <= (size_t)knob(K_WIDE_LDS_MAX);
  const size_t lds = in_lds ? want : 0;
  const dim3 grid((unsigned)((B + kPolicyThreads - 1) / kPolicyThreads));
  out.obs = nullptr;
  out.board = nullptr;
#define CAMPX_POLICY_LAUNCH(LDS, PERF, STATES)                                                     \
  do {                                                                                             \
    CAMPX_ALLOW_LDS((wide_policy_update_kernel<LDS, PERF, STATES>), lds);                          \
    hipLaunchKernelGGL((wide_policy_update_kernel<LDS, PERF, STATES>), grid, dim3(kPolicyThreads), \
                       lds, hs, pp, entries, cells, perf, policy, state, st, out, actions_out,     \
                       states_out, B, T, reset_first);                                             \
  } while (0)
#define CAMPX_POLICY_LAUNCH2(LDS, PERF)                        \
  do {                                                         \
    if (states_out) CAMPX_POLICY_LAUNCH(LDS, PERF, true);      \
    else CAMPX_POLICY_LAUNCH(LDS, PERF, false);                \
  } while (0)
  if (in_lds && out.perf) CAMPX_POLICY_LAUNCH2(true, true);
  else if (in_lds) CAMPX_POLICY_LAUNCH2(true, false);
  else if (out.perf) CAMPX_POLICY_LAUNCH2(false, true);
  else CAMPX_POLICY_LAUNCH2(false, false);
#undef CAMPX_POLICY_LAUNCH2
#undef CAMPX_POLICY_LAUNCH
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CAMPX_OK : hip_failed(e);
}

}  // extern "C"
