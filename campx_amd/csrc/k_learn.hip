// k_learn.hip - online tabular learners of the state-table tier: Q-learning and expected SARSA,
// a whole run of T frames for B independent learners in ONE launch.  Environment e IS learner e:
// it owns the table q[e][S][5], acts epsilon-greedily on it, and updates q[e][s][a] after every
// single frame - the next frame's action is chosen from the updated table.  Nothing is shared
// between lanes: no atomics, and the run is reproducible bit for bit (include/campx_hip.h has the
// rule in full; tests/learner_reference.py restates it in numpy).
//
// The walk is k_policy.hip's - a lane per environment, chunks that start on a multiple of four
// ABSOLUTE frames - with the policy row replaced by the lane's own, writable, row of Q-values.  No
// trace and no per-frame stream is written: what leaves the kernel is q, three [W][B] rows per
// window of frames (reward, hidden performance, episodes that ended; environment innermost, hence
// coalesced) and the state at the end.
//
// The chain per frame is  row -> action -> entry -> next row -> one write.  The next frame's row is
// read BEFORE this frame's write, so it is also the bootstrap row (q[n] as it stands before the
// update); when the frame stays in its state the one element just written is patched in registers.
//
// Two paths (campx_wide_learn_plan()).  Path 1: the workgroup stages the entries, the hidden
// performance and its 256 learners' tables in LDS, the tables lane-innermost -
// (s * 5 + a) * 256 + lane - so that the five reads of a row, and the write, go to 32 consecutive
// banks per half wave: conflict-free.  They are copied in and out with 16-byte global accesses.
// Path 2: each lane reads and writes its own 20-byte rows of q through L1 / L2; the entries stay
// in LDS when they alone fit.

#include "wide_table.hip.h"

namespace campx_impl {

constexpr int kLearnThreads = 256;
constexpr int kLearnChunk = 4;      // frames per chunk: two Philox blocks, a pair of frames each

struct LearnParams {
  int32_t n_states;
  int32_t window;              // frames per window of the [W][B] sums
  uint32_t key0, key1;         // seed & 0xffffffff, seed >> 32
  float discounts[16];
  int64_t first_frame;         // absolute number of the launch's frame 0
};

// What a launch takes: campx_wide_learn_plan()'s four words.
struct LearnPlan {
  int32_t path;                // 1 tables and q in LDS, 2 q through L1 / L2
  int64_t lds_bytes;
  int32_t threads;
  int32_t table_in_lds;        // the entries (and the perf bytes) are staged: always on path 1
};

inline int32_t plan_learn(int64_t S, int32_t has_perf, int64_t B, int64_t lds_max, int32_t path,
                          LearnPlan* p, int64_t* plan_out) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || (has_perf & ~1) || B < 1 || B > 0xffffffffll ||
      B * S * CAMPX_N_ACTIONS >= (1ll << 31) || lds_max < 0 || path < 0 || path > 2)
    return CAMPX_EINVAL;
  const int64_t n_entries = S * CAMPX_N_ACTIONS;
  const int64_t table = up16(n_entries * (int64_t)sizeof(uint2)) + (has_perf ? up16(n_entries) : 0);
  const int64_t want = table + kLearnThreads * n_entries * (int64_t)sizeof(float);
  const bool fits = want <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  p->path = (path == 1 || (path == 0 && fits)) ? 1 : 2;
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? want : (p->table_in_lds ? table : 0);
  p->threads = kLearnThreads;
  if (plan_out) {
    plan_out[0] = p->path;
    plan_out[1] = p->lds_bytes;
    plan_out[2] = p->threads;
    plan_out[3] = p->table_in_lds;
  }
  return CAMPX_OK;
}

// The greedy reduction of a row: best = q0; for a = 1 .. 4: if (q[a] > best) ... - the lowest
// index wins ties, NaN never wins (k_plan.hip's, with the action kept).
__device__ __forceinline__ void greedy_of(const float (&r)[5], float& best, uint32_t& arg) {
  best = r[0];
  arg = 0;
#pragma unroll
  for (int a = 1; a < 5; ++a) {
    const bool better = r[a] > best;
    best = better ? r[a] : best;
    arg = better ? (uint32_t)a : arg;
  }
}

// kQLds: path 1.  kTableLds: the entries and perf bytes are staged (always with kQLds).
// kPerf: perf_sum is written.  kSarsa: the bootstrap is expected SARSA's, else the greedy maximum.
template <bool kQLds, bool kTableLds, bool kPerf, bool kSarsa>
__global__ __launch_bounds__(kLearnThreads) void wide_learn_kernel(
    LearnParams pp, const uint2* __restrict__ g_entries, const int8_t* __restrict__ g_perf,
    float* __restrict__ q, const float* __restrict__ alphas, const float* __restrict__ gammas,
    const float* __restrict__ epsilons, int32_t* __restrict__ state, CampxState st,
    float* __restrict__ reward_sum, int32_t* __restrict__ perf_sum, int32_t* __restrict__ episodes,
    int32_t* bad_count, int32_t* bad_flag, int64_t B, int32_t T, int32_t reset_first) {
  static_assert(kTableLds || !kQLds, "path 1 stages the table");
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS;
  const int lane = threadIdx.x;
  const int64_t env_lo = (int64_t)blockIdx.x * kLearnThreads;
  const int64_t env = env_lo + lane;
  const uint2* entries = g_entries;
  const int8_t* perf_tab = g_perf;
  float* l_q = nullptr;
  // this workgroup's learners and their piece of q: contiguous, 16-byte aligned (q is, and a
  // workgroup's piece starts a multiple of 256 * 20 bytes in)
  const int n_lanes = (int)(B - env_lo < kLearnThreads ? B - env_lo : kLearnThreads);
  const int n_q = n_lanes * n_entries;                 // floats: B * S * 5 < 2^31
  float* q_block = q + env_lo * n_entries;
  if (kTableLds) {
    uint2* l_entries = lds_tables;
    int8_t* l_perf = reinterpret_cast<int8_t*>(l_entries + n_entries + (n_entries & 1));   // 16-byte aligned
    for (int i = lane; i < n_entries; i += kLearnThreads) l_entries[i] = g_entries[i];
    if (kPerf)
      for (int i = lane; i < n_entries; i += kLearnThreads) l_perf[i] = g_perf[i];
    entries = l_entries;
    perf_tab = l_perf;
    if (kQLds) {
      l_q = reinterpret_cast<float*>(l_perf + (kPerf ? (n_entries + 15) & ~15 : 0));
      // element i of the piece is learner i / n_entries, entry i % n_entries: four at a time,
      // one division per group
      const int whole = n_q & ~3;
      for (int i = lane * 4; i < whole; i += kLearnThreads * 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(q_block + i);
        int who = i / n_entries, k = i - who * n_entries;
        const float w[4] = {__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                            __uint_as_float(v.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          l_q[k * kLearnThreads + who] = w[j];
          if (++k == n_entries) {
            k = 0;
            ++who;
          }
        }
      }
      for (int i = whole + lane; i < n_q; i += kLearnThreads)
        l_q[(i % n_entries) * kLearnThreads + i / n_entries] = q_block[i];
    }
  }
  if (lane < 16) discounts[lane] = pp.discounts[lane];
  __syncthreads();

  if (env < B) {
    const float alpha = alphas[env], gamma = gammas[env], epsilon = epsilons[env];
    // (x - x is 0 exactly for a finite x, NaN for an infinity or a NaN)
    const bool good = (alpha - alpha) == 0.0f && (gamma - gamma) == 0.0f && epsilon >= 0.0f &&
                      epsilon <= 1.0f;
    const float keep = 1.0f - epsilon;
    // the lane's table: row s is five floats at own[(s * 5 + a) * step]
    float* own = kQLds ? l_q + lane : q + env * n_entries;
    constexpr int step = kQLds ? kLearnThreads : 1;
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
    float row[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) row[a] = own[(from * CAMPX_N_ACTIONS + a) * step];
    float r_sum = 0.0f;
    int32_t p_sum = 0, n_done = 0;
    int in_window = 0;
    int64_t at = env;                          // element (window, env) of the [W][B] sums
    // Chunks start on a multiple of four ABSOLUTE frames, as in wide_policy_update_kernel: frame j
    // of a chunk takes words 2 * (j & 1), 2 * (j & 1) + 1 of block j >> 1 whatever first_frame is.
    const int lead = (int)(pp.first_frame & 3);
    const uint64_t pair0 = (uint64_t)(pp.first_frame - lead) >> 1;
    for (int t0 = -lead; t0 < T; t0 += kLearnChunk) {
      uint32_t x[2 * kLearnChunk];
      const uint64_t g = pair0 + (uint64_t)((t0 + lead) >> 1);
      philox4x32_10((uint32_t)env, (uint32_t)g, (uint32_t)(g >> 32), 1u, pp.key0, pp.key1, x);
      philox4x32_10((uint32_t)env, (uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), 1u, pp.key0, pp.key1,
                    x + 4);
#pragma unroll
      for (int j = 0; j < kLearnChunk; ++j) {
        if (t0 + j >= 0 && t0 + j < T) {
          float best;
          uint32_t arg;
          greedy_of(row, best, arg);
          const float u = (float)(x[2 * j] >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
          const uint32_t any = ((x[2 * j + 1] >> 8) * 5u) >> 24;                 // 0 .. 4
          uint32_t a = u < epsilon ? any : arg;
          a = good ? a : 4u;
          const uint32_t idx = from * CAMPX_N_ACTIONS + a;
          const uint2 e = entries[idx];
          now = entry_target(e.y, (uint32_t)S);
          const uint32_t done = entry_done(e.y);
          const float D = __uint_as_float(discount_bits(discounts, entry_dcode(e.y), done));
          const float r = real_reward(__uint_as_float(e.x));
          const uint32_t next = done ? 0u : now;
          // the next frame's row, as it stands BEFORE this frame's update: the bootstrap row too
          // (a frame that ends the episode bootstraps from nothing, its target is r)
          float nrow[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) nrow[k] = own[(next * CAMPX_N_ACTIONS + k) * step];
          float b;
          uint32_t unused;
          greedy_of(nrow, b, unused);
          if (kSarsa) {
            const float m = ((((nrow[0] + nrow[1]) + nrow[2]) + nrow[3]) + nrow[4]) * 0.2f;
            b = (keep * b) + (epsilon * m);
          }
          const float target = done ? r : r + (gamma * D) * b;
          float old = row[0];
#pragma unroll
          for (int k = 1; k < 5; ++k) old = a == (uint32_t)k ? row[k] : old;
          const float delta = target - old;
          const float fresh = old + alpha * delta;
          if (good) {
            own[idx * step] = fresh;
            if (next == from) {
#pragma unroll
              for (int k = 0; k < 5; ++k) nrow[k] = a == (uint32_t)k ? fresh : nrow[k];
            }
          }
#pragma unroll
          for (int k = 0; k < 5; ++k) row[k] = nrow[k];
          from = next;
          r_sum += r;
          if (kPerf) p_sum += perf_tab[idx];
          n_done += (int32_t)done;
          ret = (over ? 0.0f : ret) + r;
          over = (int)done;
          if (++in_window == pp.window) {      // (uniform: every lane is at the same frame)
            reward_sum[at] = r_sum;
            if (kPerf) perf_sum[at] = p_sum;
            episodes[at] = n_done;
            at += B;
            r_sum = 0.0f;
            p_sum = 0;
            n_done = 0;
            in_window = 0;
          }
        }
      }
    }
    if (in_window) {                           // the last window is short
      reward_sum[at] = r_sum;
      if (kPerf) perf_sum[at] = p_sum;
      episodes[at] = n_done;
    }
    state[env] = (int32_t)now;
    st.done[env] = (uint8_t)over;
    if (st.ret) st.ret[env] = ret;
    report_bad(bad_count, bad_flag, good ? 0 : 1);     // bad LEARNERS, once per launch
  }

  if (kQLds) {
    __syncthreads();
    const int whole = n_q & ~3;
    for (int i = lane * 4; i < whole; i += kLearnThreads * 4) {
      int who = i / n_entries, k = i - who * n_entries;
      float w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = l_q[k * kLearnThreads + who];
        if (++k == n_entries) {
          k = 0;
          ++who;
        }
      }
      *reinterpret_cast<u32x4*>(q_block + i) = u32x4{__float_as_uint(w[0]), __float_as_uint(w[1]),
                                                     __float_as_uint(w[2]), __float_as_uint(w[3])};
    }
    for (int i = whole + lane; i < n_q; i += kLearnThreads)
      q_block[i] = l_q[(i % n_entries) * kLearnThreads + i / n_entries];
  }
}

// The twelve instances, at [where q and the table are][kPerf][kSarsa]: 0 both read through the
// caches, 1 the table in LDS, 2 q and the table in LDS.  (q in LDS without the table does not exist.)
using LearnKernel = decltype(&wide_learn_kernel<false, false, false, false>);
static const LearnKernel kLearnKernels[3][2][2] = {
    {{wide_learn_kernel<false, false, false, false>, wide_learn_kernel<false, false, false, true>},
     {wide_learn_kernel<false, false, true, false>, wide_learn_kernel<false, false, true, true>}},
    {{wide_learn_kernel<false, true, false, false>, wide_learn_kernel<false, true, false, true>},
     {wide_learn_kernel<false, true, true, false>, wide_learn_kernel<false, true, true, true>}},
    {{wide_learn_kernel<true, true, false, false>, wide_learn_kernel<true, true, false, true>},
     {wide_learn_kernel<true, true, true, false>, wide_learn_kernel<true, true, true, true>}}};

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_learn_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                              int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  LearnPlan plan;
  return plan_learn(n_states, has_perf, B, wide_lds_max, path, &plan, plan_out);
}

int32_t campx_wide_learn_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                                const CampxLearner* l, int64_t B, int32_t T, void* stream) {
  if (!s || !tables_dev || !st.pos || !st.done || !l || B <= 0 || T <= 0) return CAMPX_EINVAL;
  if (!l->q || !l->alpha || !l->gamma || !l->epsilon || !l->reward_sum || !l->episodes)
    return CAMPX_EINVAL;
  if (!aligned_to(l->q, 16) || !aligned_to(st.pos, 4) || !aligned_to(st.ret, 4) ||
      !aligned_to(l->alpha, 4) || !aligned_to(l->gamma, 4) || !aligned_to(l->epsilon, 4) ||
      !aligned_to(l->reward_sum, 4) || !aligned_to(l->perf_sum, 4) || !aligned_to(l->episodes, 4) ||
      !aligned_to(l->bad_count, 4) || !aligned_to(l->bad_flag, 4))
    return CAMPX_EINVAL;
  // (the environment is one 32-bit word of the Philox counter; frames count up to 2^63 - 1)
  if (B > 0xffffffffll || l->first_frame < 0 || l->first_frame > INT64_MAX - T) return CAMPX_EINVAL;
  if (l->window < 1 || (l->rule != CAMPX_LEARN_Q && l->rule != CAMPX_LEARN_EXPECTED_SARSA) ||
      l->path < 0 || l->path > 2)
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  if (l->perf_sum && !s->has_perf) return CAMPX_EINVAL;
  LearnPlan plan;      // (refuses B * n_states * 5 >= 2^31, and path 1 for what does not fit)
  const int32_t planned = plan_learn(s->n_states, l->perf_sum ? 1 : 0, B, knob(K_WIDE_LDS_MAX),
                                     l->path, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const WideTables t = wide_tables(*s, tables_dev);
  LearnParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.n_states = s->n_states;
  pp.window = l->window;
  wide_discounts(*s, pp.discounts);
  pp.key0 = (uint32_t)l->seed;
  pp.key1 = (uint32_t)(l->seed >> 32);
  pp.first_frame = l->first_frame;
  const size_t lds = (size_t)plan.lds_bytes;
  const LearnKernel kernel = kLearnKernels[plan.path == 1 ? 2 : (plan.table_in_lds ? 1 : 0)]
                                          [l->perf_sum != nullptr][l->rule == CAMPX_LEARN_EXPECTED_SARSA];
  CAMPX_ALLOW_LDS(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kLearnThreads - 1) / kLearnThreads)),
                     dim3(kLearnThreads), lds, static_cast<hipStream_t>(stream), pp, t.entries, t.perf,
                     l->q, l->alpha, l->gamma, l->epsilon, reinterpret_cast<int32_t*>(st.pos), st,
                     l->reward_sum, l->perf_sum, l->episodes, l->bad_count, l->bad_flag, B, T,
                     l->reset_first);
  return launch_status();
}

}  // extern "C"
