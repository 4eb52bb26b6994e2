// k_policy.hip - closed-loop rollouts of the state-table tier: the update pass of k_wide.hip
// (a lane per environment walking (state, action) -> state) with every frame's action SAMPLED
// on the chain, from a policy given as a table over the game's states, weights[S][5] - or from a
// POPULATION of them, weights[P][S][5].
//
// The sampling rule (include/campx_hip.h has it in full; tests/policy_reference.py restates it):
// one Philox4x32-10 block per environment and group of four frames, frame f takes word f & 3;
// u = (word >> 8) * 2^-24; thresholds c0 = w0, c1 = c0 + w1 ... c4 in f32, in that order;
// r = u * c4; action = (r >= c0) + (r >= c1) + (r >= c2) + (r >= c3).
//
// The walk.  What a frame adds to wide_update_kernel's chain is one dependent read: the state's
// row of THRESHOLDS (the sums are taken once per row when the table is staged in LDS, not once
// per frame), then the entry of (state, action) as before.  The random words do not depend on the
// state: both blocks of a chunk of eight frames are computed before its chain starts.
//
// The member rule.  The B environments split into P equal contiguous blocks, block m sampling
// policy m: environment e reads row weights[e / n][state], n = B / P, under the same Philox counter
// (absolute environment, absolute frame >> 2).  A lane works its member out once, before the frame
// loop, which then knows of it through two per-lane constants only: where the member's rows start,
// and what is added to the state that goes to `states_out` (the flat row m * S + state).  On the
// LDS path a workgroup stages, beside the table, the thresholds of just the members its 256
// environments belong to (m_lo .. m_hi, rows [m - m_lo][state][5] - a contiguous piece of the
// policy tensor).  P = 1 takes instances of the kernel compiled without any of this (kMembers):
// no division, member 0, S rows staged, nothing added.

#include "wide_table.hip.h"

#include <type_traits>

namespace campx_impl {

constexpr int kPolicyThreads = 256;
constexpr int kPolicyChunk = 8;     // frames per chunk: two Philox blocks

struct PolicyParams {
  int32_t n_states, n_planes;
  int32_t has_dcodes;          // some entry of the table carries a discount code
  uint32_t key0, key1;         // seed & 0xffffffff, seed >> 32
  uint32_t envs_per_member;    // n = B / P
  float discounts[16];
  int64_t plane;               // entries from one plane of the trace to the next (T x row pitch)
  int64_t first_frame;         // absolute number of the launch's frame 0
};

// What a launch takes: campx_wide_population_plan()'s four words.
struct PopulationPlan {
  int32_t path;                // 1 table and thresholds in LDS, 2 through L1 / L2
  int64_t lds_bytes;
  int32_t threads;
  int64_t members_per_block;   // distinct members among one workgroup's environments, at most
};

// The largest number of members any workgroup of kPolicyThreads consecutive environments touches,
// exactly.  A workgroup that starts r environments into a member and holds L of them touches
// (r + L - 1) / n + 1.  n >= 256: at most two, and two exactly when a member boundary lies inside a
// workgroup - the first one, at n, does unless n is a multiple of 256 (then none does).  n < 256:
// r = 256 b mod n repeats after at most n workgroups, so the first 256 and the last, which may be
// short, are all there is to look at.
inline int64_t members_per_block(int64_t B, int64_t P) {
  const int64_t n = B / P;
  if (n >= kPolicyThreads) return (P > 1 && n % kPolicyThreads != 0) ? 2 : 1;
  const int64_t blocks = (B + kPolicyThreads - 1) / kPolicyThreads;
  int64_t most = 1;
  auto look = [&](int64_t b) {
    const int64_t a = b * kPolicyThreads, last = (a + kPolicyThreads < B ? a + kPolicyThreads : B) - 1;
    const int64_t count = last / n - a / n + 1;
    if (count > most) most = count;
  };
  for (int64_t b = 0; b < blocks && b < kPolicyThreads; ++b) look(b);
  look(blocks - 1);
  return most;
}

inline int32_t plan_population(int64_t S, int32_t has_perf, int64_t B, int64_t P, int64_t lds_max,
                               int32_t path, PopulationPlan* p, int64_t* plan_out) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || (has_perf & ~1) || B < 1 || B > 0xffffffffll || P < 1 ||
      B % P != 0 || P * S >= (1ll << 31) || lds_max < 0 || path < 0 || path > 2)
    return CAMPX_EINVAL;
  const int64_t n_entries = S * CAMPX_N_ACTIONS;
  p->members_per_block = members_per_block(B, P);
  // wide_update_kernel's table bytes - entries, the states' cells, the hidden performance - and
  // the thresholds of the staged members, five floats per state each
  const int64_t want = up16(n_entries * (int64_t)sizeof(uint2)) + S * (int64_t)sizeof(u32x4) +
                       (has_perf ? up16(n_entries) : 0) +
                       p->members_per_block * n_entries * (int64_t)sizeof(float);
  const bool fits = want <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  p->path = (path == 1 || (path == 0 && fits)) ? 1 : 2;
  p->lds_bytes = p->path == 1 ? want : 0;
  p->threads = kPolicyThreads;
  if (plan_out) {
    plan_out[0] = p->path;
    plan_out[1] = p->lds_bytes;
    plan_out[2] = p->threads;
    plan_out[3] = p->members_per_block;
  }
  return CAMPX_OK;
}

// kMembers: the member rule; else every lane is of member 0.  kLds: the state table AND the
// thresholds of the workgroup's members sit in LDS; else both are read through L1 / L2 (the
// thresholds are then summed from the weights at every frame).  kStates: the flat row each frame
// sampled from is written out.
template <bool kMembers, bool kLds, bool kPerf, bool kStates>
__global__ __launch_bounds__(kPolicyThreads) void wide_policy_update_kernel(
    PolicyParams pp, const uint2* __restrict__ g_entries, const u32x4* __restrict__ g_cells,
    const int8_t* __restrict__ g_perf, const float* __restrict__ g_policy,
    int32_t* __restrict__ state, CampxState st, CampxOutputs out,
    int8_t* __restrict__ actions_out, int32_t* __restrict__ states_out, int64_t B, int32_t T,
    int32_t reset_first) {
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS, K = pp.n_planes;
  const int64_t env_ = (int64_t)blockIdx.x * kPolicyThreads + threadIdx.x;
  // The lane's member: one division per lane.  (A lane past the batch stages with the others and
  // leaves below; it is given the last environment's member so that nothing it forms is out of
  // range.)
  const uint32_t n = pp.envs_per_member;
  const uint32_t m = kMembers ? (uint32_t)(env_ < B ? env_ : B - 1) / n : 0u;
  const uint2* entries = g_entries;
  const u32x4* cells = g_cells;
  const int8_t* perf_tab = g_perf;
  // the thresholds (LDS) or the weights (global) of the lane's member, row 0
  const float* rows = g_policy + (int64_t)m * n_entries;
  if (kLds) {
    uint2* l_entries = lds_tables;
    u32x4* l_cells = reinterpret_cast<u32x4*>(l_entries + n_entries + (n_entries & 1));   // 16-byte aligned
    int8_t* l_perf = reinterpret_cast<int8_t*>(l_cells + S);
    float* l_thr = reinterpret_cast<float*>(l_perf + (kPerf ? (n_entries + 15) & ~15 : 0));
    // the members of this workgroup's environments: uniform, one division each
    const int64_t env_lo = (int64_t)blockIdx.x * kPolicyThreads;
    const int64_t env_hi = (env_lo + kPolicyThreads < B ? env_lo + kPolicyThreads : B) - 1;
    const uint32_t m_lo = kMembers ? (uint32_t)env_lo / n : 0u;
    const uint32_t m_hi = kMembers ? (uint32_t)env_hi / n : 0u;
    const int staged = (int)(m_hi - m_lo + 1) * S;           // rows; the host sized the LDS for them
    const float* g_rows = g_policy + (int64_t)m_lo * n_entries;
    for (int i = threadIdx.x; i < n_entries; i += kPolicyThreads) l_entries[i] = g_entries[i];
    for (int i = threadIdx.x; i < S; i += kPolicyThreads) l_cells[i] = g_cells[i];
    if (kPerf)
      for (int i = threadIdx.x; i < n_entries; i += kPolicyThreads) l_perf[i] = g_perf[i];
    for (int i = threadIdx.x; i < staged; i += kPolicyThreads) {
      float c[5];
      policy_thresholds(g_rows + (int64_t)i * CAMPX_N_ACTIONS, c);
#pragma unroll
      for (int k = 0; k < 5; ++k) l_thr[i * CAMPX_N_ACTIONS + k] = c[k];
    }
    entries = l_entries;
    cells = l_cells;
    perf_tab = l_perf;
    rows = l_thr + (m - m_lo) * (uint32_t)n_entries;
  }
  if (threadIdx.x < 16) discounts[threadIdx.x] = pp.discounts[threadIdx.x];
  __syncthreads();

  // (spelled out again, not taken from env_: hipcc then numbers the scalar registers of the
  // kMembers = false loop as it did when the kernel had no members)
  const int64_t env = (int64_t)blockIdx.x * kPolicyThreads + threadIdx.x;
  if (env >= B) return;
  const int32_t row0 = (int32_t)(m * (uint32_t)S);     // flat row of the member's state 0: P * S < 2^31
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
  const int64_t pitch = row_pitch(out, B), plane = pp.plane;
  int bad = 0;
  // Chunks start on a multiple of four ABSOLUTE frames, so that frame j of a chunk takes word
  // j & 3 of block j >> 2 whatever first_frame is: the first chunk begins up to three frames
  // before the launch's frame 0 (frames that are skipped).
  const int lead = (int)(pp.first_frame & 3);
  const uint64_t group0 = (uint64_t)(pp.first_frame - lead) >> 2;
  int64_t at = env - (int64_t)lead * pitch;        // element (frame, env) of the [T, pitch] streams
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
          for (int k = 0; k < 5; ++k) c[k] = rows[from * CAMPX_N_ACTIONS + k];
        } else {
          policy_thresholds(rows + from * CAMPX_N_ACTIONS, c);
        }
        const float u = (float)(x[j] >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
        const float r = u * c[4];
        const uint32_t a = (uint32_t)(r >= c[0]) + (uint32_t)(r >= c[1]) + (uint32_t)(r >= c[2]) +
                           (uint32_t)(r >= c[3]);
        bad += c[4] == 0.0f;
        actions_out[at] = (int8_t)a;
        if (kStates) states_out[at] = row0 + (int32_t)from;
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
      at += pitch;
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

// The sixteen instances, at [kMembers][kLds][kPerf][kStates].
using PolicyKernel = decltype(&wide_policy_update_kernel<false, false, false, false>);
#define CAMPX_POLICY_KERNELS(M, L)                                                                \
  {{wide_policy_update_kernel<M, L, false, false>, wide_policy_update_kernel<M, L, false, true>}, \
   {wide_policy_update_kernel<M, L, true, false>, wide_policy_update_kernel<M, L, true, true>}}
static const PolicyKernel kPolicyKernels[2][2][2][2] = {
    {CAMPX_POLICY_KERNELS(false, false), CAMPX_POLICY_KERNELS(false, true)},
    {CAMPX_POLICY_KERNELS(true, false), CAMPX_POLICY_KERNELS(true, true)}};
#undef CAMPX_POLICY_KERNELS

// Both entry points: `n_members` policies, each over its block of the B environments.
static int32_t policy_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                             const float* policy, uint64_t seed, int64_t first_frame, CampxOutputs out,
                             int8_t* actions_out, int32_t* states_out, int64_t B, int32_t T,
                             int32_t reset_first, int64_t n_members, int32_t path, void* stream) {
  if (!s || !tables_dev || !st.pos || !st.done || !policy || !out.trace || !actions_out || B <= 0 ||
      T <= 0)
    return CAMPX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out.trace) & 1) || (reinterpret_cast<uintptr_t>(st.pos) & 3) ||
      (reinterpret_cast<uintptr_t>(policy) & 3) || (reinterpret_cast<uintptr_t>(states_out) & 3))
    return CAMPX_EINVAL;
  if (out.scalar_pitch && out.scalar_pitch < B) return CAMPX_EINVAL;
  // (the environment is one 32-bit word of the Philox counter; frames count up to 2^63 - 1)
  if (B > 0xffffffffll || first_frame < 0 || first_frame > INT64_MAX - T) return CAMPX_EINVAL;
  if (n_members < 1 || B % n_members != 0) return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  if (out.perf && !s->has_perf) return CAMPX_EINVAL;
  PopulationPlan plan;
  const int32_t planned = plan_population(s->n_states, out.perf ? 1 : 0, B, n_members,
                                          knob(K_WIDE_LDS_MAX), path, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const WideTables t = wide_tables(*s, tables_dev);
  PolicyParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.n_states = s->n_states;
  pp.n_planes = t.lay.n_planes;
  wide_discounts(*s, pp.discounts);
  pp.has_dcodes = s->any_dcode;
  pp.key0 = (uint32_t)seed;
  pp.key1 = (uint32_t)(seed >> 32);
  pp.envs_per_member = (uint32_t)(B / n_members);
  pp.plane = (int64_t)T * row_pitch(out, B);
  pp.first_frame = first_frame;
  out.obs = nullptr;
  out.board = nullptr;
  const PolicyKernel kernel =
      kPolicyKernels[n_members > 1][plan.path == 1][out.perf != nullptr][states_out != nullptr];
  CAMPX_ALLOW_LDS(kernel, (size_t)plan.lds_bytes);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kPolicyThreads - 1) / kPolicyThreads)),
                     dim3(kPolicyThreads), (size_t)plan.lds_bytes, static_cast<hipStream_t>(stream), pp,
                     t.entries, t.cells, t.perf, policy, reinterpret_cast<int32_t*>(st.pos), st, out,
                     actions_out, states_out, B, T, reset_first);
  return launch_status();
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_policy_update_launch(const CampxWideSpec* s, const void* tables_dev,
                                        CampxState st, const float* policy, uint64_t seed,
                                        int64_t first_frame, CampxOutputs out, int8_t* actions_out,
                                        int32_t* states_out, int64_t B, int32_t T,
                                        int32_t reset_first, void* stream) {
  return policy_launch(s, tables_dev, st, policy, seed, first_frame, out, actions_out, states_out, B, T,
                       reset_first, 1, 0, stream);
}

int32_t campx_wide_population_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t n_members,
                                   int64_t wide_lds_max, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  PopulationPlan plan;
  return plan_population(n_states, has_perf, B, n_members, wide_lds_max, path, &plan, plan_out);
}

int32_t campx_wide_policy_population_launch(const CampxWideSpec* s, const void* tables_dev,
                                            CampxState st, const float* policy, uint64_t seed,
                                            int64_t first_frame, CampxOutputs out,
                                            int8_t* actions_out, int32_t* states_out, int64_t B,
                                            int32_t T, int32_t reset_first, int64_t n_members,
                                            int32_t path, void* stream) {
  return policy_launch(s, tables_dev, st, policy, seed, first_frame, out, actions_out, states_out, B, T,
                       reset_first, n_members, path, stream);
}

}  // extern "C"
