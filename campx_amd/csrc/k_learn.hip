// k_learn.hip - online tabular learners of the state-table tier: Q-learning and expected SARSA,
// a whole run of T frames in ONE launch, reproducible bit for bit (include/campx_hip.h has the
// rules in full; tests/learner_reference.py and tests/shared_learner_reference.py restate them in
// numpy).  Three kernels, three schedules, each with its own account below: wide_learn_kernel, a
// table per environment, updated after every single frame, nothing shared between lanes;
// wide_learn_shared_kernel, n environments feeding one table, two barriers a frame; and
// wide_learn_traces_kernel, a table and an eligibility trace per environment, a team of lanes
// sweeping the whole table every frame (tests/trace_learner_reference.py).  A fourth,
// wide_learn_dyna_kernel, is the first's schedule with n planning updates of remembered pairs after
// every frame (Dyna-Q; tests/dyna_learner_reference.py).  A fifth, wide_learn_actor_kernel, is the
// first's schedule again with a softmax policy and a critic per learner in place of the Q-table
// (one-step actor-critic; tests/actor_critic_reference.py).  A sixth,
// wide_learn_actor_shared_kernel, is the second's schedule with the fifth's frame: n environments
// feeding one policy and one critic (tests/shared_actor_reference.py).
//
// What they have in common is written ONCE and called by all - a change of the rule is made
// there.  "The frame step": stage_table() (entries and perf bytes into LDS), Hyper (alpha, gamma,
// epsilon, `keep`, the `good` test), Carried (a lane's state / done / ret), Chunks (the Philox
// blocks of four ABSOLUTE frames), frame_action() (rule step 3), decode_entry() (step 4),
// td_error() (steps 5 - 7's delta), WindowSums (step 8).  "Launch set-up": plan_args_ok() and
// table_bytes() behind both plans; screen_learner(), learn_params() and pick_kernel() behind both
// launchers.  What a kernel does with delta, and when it reads the bootstrap row, is its own.
//
// The walk is k_policy.hip's - a lane per environment - with the policy row replaced by a writable
// row of Q-values.  No trace and no per-frame stream is written: what leaves a kernel is q, three
// [W][B] rows per window of frames (reward, hidden performance, episodes that ended; environment
// innermost, hence coalesced) and the state at the end.

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

// ---------------------------------------------------------------------------------------------
// The frame step: what wide_learn_kernel and wide_learn_shared_kernel share.  No helper holds a
// barrier, or a return that depends on the lane.

// The entries and the perf bytes as a kernel reads them, and the first free, 16-byte aligned LDS
// address after them: a kernel lays out its own q and accumulators there.  kTableLds: thread `tid`
// of `stride` copies its share to the dynamic LDS at `lds` (16-byte aligned), entries first, then -
// kPerf - the perf bytes from the next 16-byte boundary; the caller's barrier makes them visible.
struct StagedTable { const uint2* entries; const int8_t* perf_tab; unsigned char* free; };
template <bool kTableLds, bool kPerf>
__device__ __forceinline__ StagedTable stage_table(uint2* lds, const uint2* g_entries,
                                                   const int8_t* g_perf, int n_entries, int tid,
                                                   int stride) {
  if (!kTableLds) return {g_entries, g_perf, reinterpret_cast<unsigned char*>(lds)};
  int8_t* l_perf = reinterpret_cast<int8_t*>(lds + n_entries + (n_entries & 1));
  for (int i = tid; i < n_entries; i += stride) lds[i] = g_entries[i];
  if (kPerf)
    for (int i = tid; i < n_entries; i += stride) l_perf[i] = g_perf[i];
  return {lds, l_perf, reinterpret_cast<unsigned char*>(l_perf + (kPerf ? (n_entries + 15) & ~15 : 0))};
}

// A learner's hyper-parameters.  As constructed: those of a lane that has none (it is not `good`).
struct Hyper {
  float alpha = 0.0f, gamma = 0.0f, epsilon = 0.0f, keep = 0.0f;
  bool good = false;
  __device__ __forceinline__ void load(const float* alphas, const float* gammas, const float* epsilons,
                                       int64_t learner) {
    alpha = alphas[learner];
    gamma = gammas[learner];
    epsilon = epsilons[learner];
    // (x - x is 0 exactly for a finite x, NaN for an infinity or a NaN)
    good = (alpha - alpha) == 0.0f && (gamma - gamma) == 0.0f && epsilon >= 0.0f && epsilon <= 1.0f;
    keep = 1.0f - epsilon;
  }
};

// One table entry, decoded: the state it leads to, the state the next frame starts from (0 after
// `done`), the frame's discount and its reward, None counted as 0.
struct Entry { uint32_t now, next, done; float D, r; };
__device__ __forceinline__ Entry decode_entry(uint2 e, int S, const float* discounts) {
  const uint32_t now = entry_target(e.y, (uint32_t)S), done = entry_done(e.y);
  return {now, done ? 0u : now, done, __uint_as_float(discount_bits(discounts, entry_dcode(e.y), done)),
          real_reward(__uint_as_float(e.x))};
}

// What a lane carries from frame to frame, and from launch to launch in state / done / ret.  As
// constructed: a new episode (`reset_first`, and a lane without an environment).
struct Carried {
  uint32_t now = 0, from = 0;  // the state as stored; the state the frame starts from
  int over = 0;
  float ret = 0.0f;
  __device__ __forceinline__ void load(const int32_t* state, const CampxState& st, int64_t env, int S,
                                       int32_t reset_first) {
    if (!reset_first) {
      now = (uint32_t)state[env];
      now = now < (uint32_t)S ? now : 0u;      // (a state index from outside: start over)
      over = st.done[env];
      if (st.ret) ret = st.ret[env];
    }
    from = over ? 0u : now;
  }
  __device__ __forceinline__ void advance(const Entry& e) {
    now = e.now;
    from = e.next;
    ret = (over ? 0.0f : ret) + e.r;
    over = (int)e.done;
  }
  __device__ __forceinline__ void store(int32_t* state, const CampxState& st, int64_t env) const {
    state[env] = (int32_t)now;
    st.done[env] = (uint8_t)over;
    if (st.ret) st.ret[env] = ret;
  }
};

// Chunks start on a multiple of four ABSOLUTE frames, as in wide_policy_update_kernel: t0 runs from
// -lead in steps of kLearnChunk, and frame j of a chunk takes words 2 * (j & 1), 2 * (j & 1) + 1 of
// block j >> 1 - x[2 * j] and x[2 * j + 1] of words() - whatever first_frame is.
struct Chunks {
  int lead;                    // frames of the first chunk that lie before the launch's frame 0
  uint64_t pair0;              // the first chunk's first pair of frames
  __device__ __forceinline__ explicit Chunks(int64_t first_frame)
      : lead((int)(first_frame & 3)), pair0((uint64_t)(first_frame - lead) >> 1) {}
  __device__ __forceinline__ void words(const LearnParams& pp, int64_t env, int t0,
                                        uint32_t (&x)[2 * kLearnChunk]) const {
    const uint64_t g = pair0 + (uint64_t)((t0 + lead) >> 1);
    philox4x32_10((uint32_t)env, (uint32_t)g, (uint32_t)(g >> 32), 1u, pp.key0, pp.key1, x);
    philox4x32_10((uint32_t)env, (uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), 1u, pp.key0, pp.key1,
                  x + 4);
  }
};

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

// A frame's action: the row's greedy one, or - the frame's first word below epsilon - the one its
// second word draws; action 4 for a learner that is not good.
__device__ __forceinline__ uint32_t frame_action(const float (&row)[5], uint32_t x0, uint32_t x1,
                                                 float epsilon, bool good) {
  float best;
  uint32_t arg;
  greedy_of(row, best, arg);
  const float u = (float)(x0 >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
  const uint32_t any = ((x1 >> 8) * 5u) >> 24;                     // 0 .. 4
  const uint32_t a = u < epsilon ? any : arg;
  return good ? a : 4u;
}

// The TD error of a frame that met entry `e`; `old` is the element of its row that the action it
// took picks and the kernel goes on to update, `nrow` the bootstrap row (a frame that ends the
// episode bootstraps from nothing, its target is r).  (`old` is picked in the kernel: the same
// selection in a helper, on a row passed by reference, becomes an indexed load before it is inlined,
// and the row then lives in scratch.  The entry is read before the choice: a select, no branch.)
template <bool kSarsa>
__device__ __forceinline__ float td_error(float old, const float (&nrow)[5], const Entry& e,
                                          float gamma, float keep, float epsilon) {
  float b;
  uint32_t unused;
  greedy_of(nrow, b, unused);
  if (kSarsa) {
    const float m = ((((nrow[0] + nrow[1]) + nrow[2]) + nrow[3]) + nrow[4]) * 0.2f;
    b = (keep * b) + (epsilon * m);
  }
  const float r = e.r, discounted = (gamma * e.D) * b;
  const float target = e.done ? r : r + discounted;
  return target - old;
}

// The sums of the window of frames a lane is in, and where they go: element `at` = (window, env)
// of the three [W][B] rows of pitch B (perf_sum, and add()'s `perf`, only when kPerf).  Every lane
// is at the same frame: the flush is uniform.  flush_short(): the last window may be short.
template <bool kPerf>
struct WindowSums {
  float* reward_sum;
  int32_t *perf_sum, *episodes;
  int64_t at;
  float r_sum = 0.0f;
  int32_t p_sum = 0, n_done = 0;
  int in_window = 0;
  __device__ __forceinline__ void write() const {
    reward_sum[at] = r_sum;
    if (kPerf) perf_sum[at] = p_sum;
    episodes[at] = n_done;
  }
  __device__ __forceinline__ void add(const LearnParams& pp, float r, int32_t perf, uint32_t done,
                                      int64_t B) {
    r_sum += r;
    if (kPerf) p_sum += perf;
    n_done += (int32_t)done;
    if (++in_window == pp.window) {
      write();
      at += B;
      r_sum = 0.0f, p_sum = n_done = in_window = 0;
    }
  }
  __device__ __forceinline__ void flush_short() const { if (in_window) write(); }
};

// ---------------------------------------------------------------------------------------------
// Launch set-up: what the two plans and the two launchers share.

// The LDS bytes of the staged entries and perf bytes.
inline int64_t table_bytes(int64_t S, int32_t has_perf) {
  const int64_t n_entries = S * CAMPX_N_ACTIONS;
  return up16(n_entries * (int64_t)sizeof(uint2)) + (has_perf ? up16(n_entries) : 0);
}

// A plan's arguments; the `tables` <= B Q-tables of S x 5 floats are indexed with 32 bits.
inline bool plan_args_ok(int64_t S, int32_t has_perf, int64_t B, int64_t tables, int64_t lds_max,
                         int32_t path) {
  return !(S < 1 || S > CAMPX_WIDE_MAX_STATES || (has_perf & ~1) || B < 1 || B > 0xffffffffll ||
           tables * S * CAMPX_N_ACTIONS >= (1ll << 31) || lds_max < 0 || path < 0 || path > 2);
}

// What a launcher refuses before anything touches a device, for CampxLearner and CampxSharedLearner
// alike (their common fields carry the same names); `own_ok`: the caller's checks of its own fields.
template <typename Learner>
int32_t screen_learner(const CampxWideSpec* s, const void* tables_dev, const CampxState& st,
                       const Learner* l, int64_t B, int32_t T, bool own_ok) {
  if (!s || !tables_dev || !st.pos || !st.done || !l || B <= 0 || T <= 0 || !own_ok || !l->q ||
      !l->alpha || !l->gamma || !l->epsilon || !l->reward_sum || !l->episodes)
    return CAMPX_EINVAL;
  if (!aligned_to(l->q, 16) || !aligned_to(st.pos, 4) || !aligned_to(st.ret, 4) ||
      !aligned_to(l->alpha, 4) || !aligned_to(l->gamma, 4) || !aligned_to(l->epsilon, 4) ||
      !aligned_to(l->reward_sum, 4) || !aligned_to(l->perf_sum, 4) || !aligned_to(l->episodes, 4) ||
      !aligned_to(l->bad_count, 4) || !aligned_to(l->bad_flag, 4))
    return CAMPX_EINVAL;
  // (the environment is one 32-bit word of the Philox counter; frames count up to 2^63 - 1)
  if (B > 0xffffffffll || l->first_frame < 0 || l->first_frame > INT64_MAX - T || l->window < 1 ||
      (l->rule != CAMPX_LEARN_Q && l->rule != CAMPX_LEARN_EXPECTED_SARSA) || l->path < 0 || l->path > 2)
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  if (l->perf_sum && !s->has_perf) return CAMPX_EINVAL;
  return CAMPX_OK;
}

template <typename Learner>
LearnParams learn_params(const CampxWideSpec& s, const Learner& l) {
  LearnParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.n_states = s.n_states;
  pp.window = l.window;
  wide_discounts(s, pp.discounts);
  pp.key0 = (uint32_t)l.seed;
  pp.key1 = (uint32_t)(l.seed >> 32);
  pp.first_frame = l.first_frame;
  return pp;
}

// The twelve instances of a kernel template <kQLds, kTableLds, kPerf, kSarsa>, at
// [where q and the table are][kPerf][kSarsa]: 0 both read through the caches, 1 the table in LDS,
// 2 q and the table in LDS.  (q in LDS without the table does not exist.)
#define CAMPX_LEARN_INSTANCES(K)                                                  \
  {{{K<0, 0, 0, 0>, K<0, 0, 0, 1>}, {K<0, 0, 1, 0>, K<0, 0, 1, 1>}},              \
   {{K<0, 1, 0, 0>, K<0, 1, 0, 1>}, {K<0, 1, 1, 0>, K<0, 1, 1, 1>}},              \
   {{K<1, 1, 0, 0>, K<1, 1, 0, 1>}, {K<1, 1, 1, 0>, K<1, 1, 1, 1>}}}

template <typename Kernel, typename Plan, typename Learner>
Kernel pick_kernel(const Kernel (&instances)[3][2][2], const Plan& plan, const Learner& l) {
  return instances[plan.path == 1 ? 2 : (plan.table_in_lds ? 1 : 0)][l.perf_sum != nullptr]
                  [l.rule == CAMPX_LEARN_EXPECTED_SARSA];
}

// ---------------------------------------------------------------------------------------------
// A table per environment.  The chain per frame is  row -> action -> entry -> next row -> one
// write.  The next frame's row is read BEFORE this frame's write, so it is also the bootstrap row
// (q[n] as it stands before the update); when the frame stays in its state the one element just
// written is patched in registers.
//
// Two paths (campx_wide_learn_plan()).  Path 1: the workgroup stages the entries, the hidden
// performance and its 256 learners' tables in LDS, the tables lane-innermost -
// (s * 5 + a) * 256 + lane - so that the five reads of a row, and the write, go to 32 consecutive
// banks per half wave: conflict-free.  They are copied in and out with 16-byte global accesses.
// Path 2: each lane reads and writes its own 20-byte rows of q through L1 / L2; the entries stay
// in LDS when they alone fit.

// campx_wide_learn_plan()'s four words, in their order.  path: 1 tables and q in LDS, 2 q through
// L1 / L2; table_in_lds: the entries (and the perf bytes) are staged, always on path 1.
struct LearnPlan { int64_t path, lds_bytes, threads, table_in_lds; };

inline int32_t plan_learn(int64_t S, int32_t has_perf, int64_t B, int64_t lds_max, int32_t path,
                          LearnPlan* p, int64_t* plan_out) {
  if (!plan_args_ok(S, has_perf, B, B, lds_max, path)) return CAMPX_EINVAL;
  const int64_t table = table_bytes(S, has_perf);
  const int64_t want = table + kLearnThreads * S * CAMPX_N_ACTIONS * (int64_t)sizeof(float);
  const bool fits = want <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  p->path = (path == 1 || (path == 0 && fits)) ? 1 : 2;
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? want : (p->table_in_lds ? table : 0);
  p->threads = kLearnThreads;
  if (plan_out) memcpy(plan_out, p, sizeof(*p));
  return CAMPX_OK;
}

// Path 1's tables between q - element i of the workgroup's piece is learner i / n_entries, entry
// i % n_entries - and LDS (kIn: into it, else back out): four elements and one 16-byte global access
// at a time, one division per group.
template <bool kIn>
__device__ __forceinline__ void move_q(float* l_q, float* q_block, int n_q, int n_entries, int lane) {
  const int whole = n_q & ~3;
  for (int i = lane * 4; i < whole; i += kLearnThreads * 4) {
    u32x4* piece = reinterpret_cast<u32x4*>(q_block + i);
    u32x4 v = kIn ? *piece : u32x4{};
    int who = i / n_entries, k = i - who * n_entries;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float& cell = l_q[k * kLearnThreads + who];
      if (kIn) cell = __uint_as_float(v[j]);
      else v[j] = __float_as_uint(cell);
      if (++k == n_entries) {
        k = 0;
        ++who;
      }
    }
    if (!kIn) *piece = v;
  }
  for (int i = whole + lane; i < n_q; i += kLearnThreads) {
    float& cell = l_q[(i % n_entries) * kLearnThreads + i / n_entries];
    if (kIn) cell = q_block[i];
    else q_block[i] = cell;
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
  // this workgroup's learners and their piece of q: contiguous, 16-byte aligned (q is, and a
  // workgroup's piece starts a multiple of 256 * 20 bytes in)
  const int n_lanes = (int)(B - env_lo < kLearnThreads ? B - env_lo : kLearnThreads);
  const int n_q = n_lanes * n_entries;                 // floats: B * S * 5 < 2^31
  float* q_block = q + env_lo * n_entries;
  const StagedTable tab =
      stage_table<kTableLds, kPerf>(lds_tables, g_entries, g_perf, n_entries, lane, kLearnThreads);
  float* l_q = reinterpret_cast<float*>(tab.free);
  if (kQLds) move_q<true>(l_q, q_block, n_q, n_entries, lane);
  if (lane < 16) discounts[lane] = pp.discounts[lane];
  __syncthreads();

  if (env < B) {
    Hyper h;
    h.load(alphas, gammas, epsilons, env);
    // the lane's table: row s is five floats at own[(s * 5 + a) * step]
    float* own = kQLds ? l_q + lane : q + env * n_entries;
    constexpr int step = kQLds ? kLearnThreads : 1;
    Carried c;
    c.load(state, st, env, S, reset_first);
    float row[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) row[a] = own[(c.from * CAMPX_N_ACTIONS + a) * step];
    WindowSums<kPerf> sums{reward_sum, perf_sum, episodes, env};
    const Chunks chunks(pp.first_frame);
    for (int t0 = -chunks.lead; t0 < T; t0 += kLearnChunk) {
      uint32_t x[2 * kLearnChunk];
      chunks.words(pp, env, t0, x);
#pragma unroll
      for (int j = 0; j < kLearnChunk; ++j) {
        if (t0 + j >= 0 && t0 + j < T) {
          const uint32_t a = frame_action(row, x[2 * j], x[2 * j + 1], h.epsilon, h.good);
          const uint32_t idx = c.from * CAMPX_N_ACTIONS + a;
          const Entry e = decode_entry(tab.entries[idx], S, discounts);
          // the next frame's row, as it stands BEFORE this frame's update: the bootstrap row too.
          // It is read for a bad learner as well: it is the row its next frame acts from.
          float nrow[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) nrow[k] = own[(e.next * CAMPX_N_ACTIONS + k) * step];
          float old = row[0];
#pragma unroll
          for (int k = 1; k < 5; ++k) old = a == (uint32_t)k ? row[k] : old;
          const float delta = td_error<kSarsa>(old, nrow, e, h.gamma, h.keep, h.epsilon);
          const float fresh = old + h.alpha * delta;
          if (h.good) {
            own[idx * step] = fresh;
            if (e.next == c.from) {
#pragma unroll
              for (int k = 0; k < 5; ++k) nrow[k] = a == (uint32_t)k ? fresh : nrow[k];
            }
          }
#pragma unroll
          for (int k = 0; k < 5; ++k) row[k] = nrow[k];
          c.advance(e);
          sums.add(pp, e.r, kPerf ? tab.perf_tab[idx] : 0, e.done, B);
        }
      }
    }
    sums.flush_short();
    c.store(state, st, env);
    report_bad(bad_count, bad_flag, h.good ? 0 : 1);     // bad LEARNERS, once per launch
  }

  if (kQLds) {
    __syncthreads();
    move_q<false>(l_q, q_block, n_q, n_entries, lane);
  }
}

using LearnKernel = decltype(&wide_learn_kernel<false, false, false, false>);
static const LearnKernel kLearnKernels[3][2][2] = CAMPX_LEARN_INSTANCES(wide_learn_kernel);

// ---------------------------------------------------------------------------------------------
// Shared learners: P tables, each fed by the n = B / P consecutive environments of its block
// (include/campx_hip.h, "Shared online learners", has the rule; tests/shared_learner_reference.py
// restates it in numpy).  Within a frame every environment of a learner reads the table as the
// frame found it; the TD errors - td_error(), the per-environment learners' - are quantised to
// 64-bit fixed point and added per (state, action) as INTEGERS, and the table moves once per
// visited bin: no order of arrival changes a bit.
//
// A workgroup holds G whole learners, G * n threads, thread tid being environment
// blockIdx.x * G * n + tid.  A frame is
//   (A) row, action, entry, bootstrap row, delta; count += 1 and sum += z on the bin's accumulators
//       (workgroup-scope atomics) - the lane whose count-add returned 0 owns the bin;
//   barrier;
//   (B) the owner exchanges both accumulators for 0 and writes q[m][s][a];
//   barrier.
// EVERY lane of the workgroup reaches both barriers of every frame: the loop bounds depend on the
// kernel's arguments alone, and what an absent lane (past B in the last workgroup) or the lane of
// a bad learner skips lies BETWEEN the barriers, never around one.
//
// Path 1: the entries, the perf bytes, the G tables (as they lie in q: a straight copy in and out)
// and the accumulators in LDS.  Path 2: q and the accumulators - `scratch`, zero on entry and left
// zero by the exchanges of (B) - in global memory, through the L2 the workgroup's waves share; the
// entries in LDS when they alone fit.

constexpr int kSharedMaxThreads = 1024;      // the largest workgroup: actors per learner, at most
constexpr int kSharedPack = 256;             // threads a workgroup of several learners has, at most
constexpr int64_t kSharedBytesPerEntry = 16; // path 1, per (learner, state, action): sum 8, q 4, count 4
constexpr double kSharedScale = 4294967296.0;          // 2^32
constexpr double kSharedLimit = 4503599627370496.0;    // 2^52
constexpr long long kSharedLimitQ = 1ll << 52;

// campx_wide_shared_plan()'s six words, in their order.  path: 1 tables, q and accumulators in LDS,
// 2 q and accumulators global; learners: G, whole learners of a workgroup; threads: G * n; copies:
// accumulators per bin - 1, the adds are not privatised.
struct SharedPlan { int64_t path, learners, threads, lds_bytes, table_in_lds, copies; };

// The plan rule of both shared kernels; `per_state`: path 1's LDS bytes per state and learner.
inline int32_t plan_shared_rule(int64_t S, int32_t has_perf, int64_t B, int64_t P, int64_t lds_max,
                                int32_t path, int64_t per_state, SharedPlan* p, int64_t* plan_out) {
  if (P < 1 || P > B || !plan_args_ok(S, has_perf, B, P, lds_max, path) || B % P != 0 ||
      B / P > kSharedMaxThreads)
    return CAMPX_EINVAL;
  const int64_t n = B / P;
  const int64_t table = table_bytes(S, has_perf);
  const int64_t per = S * per_state;
  int64_t most = n <= kSharedPack ? kSharedPack / n : 1;       // what a workgroup would hold
  if (most > P) most = P;
  const int64_t room = lds_max >= table ? (lds_max - table) / per : 0;
  const int64_t held = room < most ? room : most;              // ... and what of it path 1 can
  if (path == 1 && held < 1) return CAMPX_EINVAL;
  // Unforced, path 1 must still fill a wave (or hold all it would anyway): a workgroup cut down to
  // a few lanes by its LDS leaves most of a wave idle at every frame.
  const bool pays = held >= 1 && (held == most || held * n >= 64);
  p->path = (path == 1 || (path == 0 && pays)) ? 1 : 2;
  p->learners = p->path == 1 ? held : most;
  p->threads = p->learners * n;
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? table + p->learners * per : (p->table_in_lds ? table : 0);
  p->copies = 1;
  if (plan_out) memcpy(plan_out, p, sizeof(*p));
  return CAMPX_OK;
}

inline int32_t plan_shared(int64_t S, int32_t has_perf, int64_t B, int64_t P, int64_t lds_max,
                           int32_t path, SharedPlan* p, int64_t* plan_out) {
  return plan_shared_rule(S, has_perf, B, P, lds_max, path, CAMPX_N_ACTIONS * kSharedBytesPerEntry, p,
                          plan_out);
}

// kQLds: path 1.  kTableLds, kPerf, kSarsa: as in wide_learn_kernel.  `n`: environments per
// learner; `G`: learners per workgroup, blockDim.x == G * n.  `acc_sum` / `acc_count`: path 2's
// accumulators, [P][S][5] each.
template <bool kQLds, bool kTableLds, bool kPerf, bool kSarsa>
__global__ __launch_bounds__(kSharedMaxThreads) void wide_learn_shared_kernel(
    LearnParams pp, const uint2* __restrict__ g_entries, const int8_t* __restrict__ g_perf, float* q,
    const float* __restrict__ alphas, const float* __restrict__ gammas,
    const float* __restrict__ epsilons, int32_t* __restrict__ state, CampxState st,
    float* __restrict__ reward_sum, int32_t* __restrict__ perf_sum, int32_t* __restrict__ episodes,
    long long* __restrict__ clamped, long long* acc_sum, uint32_t* acc_count, int32_t* bad_count,
    int32_t* bad_flag, int64_t B, int64_t P, int32_t n, int32_t G, int32_t T, int32_t reset_first) {
  static_assert(kTableLds || !kQLds, "path 1 stages the table");
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  __shared__ unsigned long long l_clamped[kSharedPack];      // per learner of the workgroup
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS;
  const int tid = threadIdx.x, threads = blockDim.x;
  const int64_t first_learner = (int64_t)blockIdx.x * G;
  const int n_here = (int)(P - first_learner < G ? P - first_learner : G);   // learners present
  const int64_t env = first_learner * n + tid;
  const int who = tid / n;                                   // learner of the workgroup
  const bool active = who < n_here;                          // (an absent lane: last workgroup only)
  const int64_t m = first_learner + who;
  const int n_q = n_here * n_entries;                        // floats: P * S * 5 < 2^31
  float* q_block = q + first_learner * n_entries;
  float* tables = q_block;                                   // [learner][s][a], wherever they are
  long long* sums = kQLds ? nullptr : acc_sum + first_learner * n_entries;
  uint32_t* counts = kQLds ? nullptr : acc_count + first_learner * n_entries;
  const StagedTable tab =
      stage_table<kTableLds, kPerf>(lds_tables, g_entries, g_perf, n_entries, tid, threads);
  if (kQLds) {
    // [sums G x entries x 8][tables G x entries x 4][counts G x entries x 4], 16-byte aligned
    sums = reinterpret_cast<long long*>(tab.free);
    float* l_q = reinterpret_cast<float*>(sums + (int64_t)G * n_entries);
    counts = reinterpret_cast<uint32_t*>(l_q + (int64_t)G * n_entries);
    for (int i = tid; i < n_q; i += threads) {
      l_q[i] = q_block[i];
      sums[i] = 0;
      counts[i] = 0u;
    }
    tables = l_q;
  }
  if (tid < 16) discounts[tid] = pp.discounts[tid];
  if (tid < kSharedPack) l_clamped[tid] = 0ull;
  __syncthreads();

  // What stays in registers for the run.  An absent lane keeps these values - no learner, a new
  // episode, empty sums - and does nothing between the barriers below.
  Hyper h;
  Carried c;
  WindowSums<kPerf> win{reward_sum, perf_sum, episodes, env};
  unsigned long long n_clamped = 0ull;
  const int own = who * n_entries;             // the learner's table, sums and counts start here
  if (active) {
    h.load(alphas, gammas, epsilons, m);
    c.load(state, st, env, S, reset_first);
  }
  const Chunks chunks(pp.first_frame);
  for (int t0 = -chunks.lead; t0 < T; t0 += kLearnChunk) {
    uint32_t x[2 * kLearnChunk];
    if (active) chunks.words(pp, env, t0, x);
#pragma unroll
    for (int j = 0; j < kLearnChunk; ++j) {
      if (t0 + j < 0 || t0 + j >= T) continue;               // (uniform: kernel arguments alone)
      int bin = 0;                                           // own + s * 5 + a
      bool owner = false;
      if (active) {                                          // ---- (A)
        float row[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) row[k] = tables[own + c.from * CAMPX_N_ACTIONS + k];
        const uint32_t a = frame_action(row, x[2 * j], x[2 * j + 1], h.epsilon, h.good);
        const uint32_t idx = c.from * CAMPX_N_ACTIONS + a;
        const Entry e = decode_entry(tab.entries[idx], S, discounts);
        if (h.good) {
          // the bootstrap row: the table as the frame found it, for every lane of the learner
          float nrow[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) nrow[k] = tables[own + e.next * CAMPX_N_ACTIONS + k];
          float old = row[0];
#pragma unroll
          for (int k = 1; k < 5; ++k) old = a == (uint32_t)k ? row[k] : old;
          const float delta = td_error<kSarsa>(old, nrow, e, h.gamma, h.keep, h.epsilon);
          const double d = (double)delta * kSharedScale;
          long long z;
          if (!(fabs(d) <= kSharedLimit)) {                  // NaN, +-Inf, past the limit
            ++n_clamped;
            z = d != d ? 0ll : (d > 0.0 ? kSharedLimitQ : -kSharedLimitQ);
          } else {
            z = __double2ll_rn(d);
          }
          bin = own + (int)idx;
          owner = __hip_atomic_fetch_add(&counts[bin], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_WORKGROUP) == 0u;
          __hip_atomic_fetch_add(&sums[bin], z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        c.advance(e);
        win.add(pp, e.r, kPerf ? tab.perf_tab[idx] : 0, e.done, B);
      }
      __syncthreads();
      if (owner) {                                           // ---- (B)
        const long long Z = __hip_atomic_exchange(&sums[bin], 0ll, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t visits = __hip_atomic_exchange(&counts[bin], 0u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
        const double g = (double)Z / (double)visits;
        const float mean = (float)(g * (1.0 / kSharedScale));
        const float step = h.alpha * mean;
        tables[bin] = tables[bin] + step;
      }
      __syncthreads();
    }
  }
  if (active) {
    win.flush_short();
    c.store(state, st, env);
    if (n_clamped)
      __hip_atomic_fetch_add(&l_clamped[who], n_clamped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tid == who * n) report_bad(bad_count, bad_flag, h.good ? 0 : 1);     // bad LEARNERS, once
  }
  __syncthreads();
  if (active && tid == who * n) clamped[m] = (long long)l_clamped[who];
  if (kQLds)
    for (int i = tid; i < n_q; i += threads) q_block[i] = tables[i];
}

using SharedKernel = decltype(&wide_learn_shared_kernel<false, false, false, false>);
static const SharedKernel kSharedKernels[3][2][2] = CAMPX_LEARN_INSTANCES(wide_learn_shared_kernel);

// ---------------------------------------------------------------------------------------------
// Eligibility traces: Q(lambda) and expected SARSA(lambda), a table AND a trace per (state, action)
// per environment (include/campx_hip.h, "Online learners with eligibility traces", has the frame;
// tests/trace_learner_reference.py restates it in numpy).  The one learner whose frame touches the
// whole table: a learner is a TEAM of L lanes (a power of two), a workgroup 256 threads holding
// G = 256 / L learners, thread tid being lane tid % L of learner blockIdx.x * G + tid / L.  A frame is
//   (A) EVERY lane of the team computes the scalar part - row, action, entry, bootstrap row, delta,
//       step, c - from the same words: broadcast reads, no communication;
//   barrier (L > 1): all lanes have read row / nrow / old;
//   (B) lane l's pass over the entries i = l (mod L): cut, bump, sweep and decay fused - one read of
//       z, one read-modify-write of q where z != 0, one write of z;
//   barrier (L > 1): the table is whole again before the next frame's rows are read.
// EVERY lane of the workgroup reaches both barriers of every frame: the loop bounds depend on the
// kernel's arguments alone (L is one), and what an absent lane (a team past B in the last workgroup)
// or the lanes of a bad learner skip lies BETWEEN the barriers, never around one - the discipline of
// wide_learn_shared_kernel.  L = 1 has no barrier: a lane reads what it wrote itself.
// Two barriers, not one: (B) of frame t writes what (A) of frame t reads and (A) of frame t + 1
// reads what (B) of frame t wrote, so both orders need a barrier unless (B) writes another copy than
// (A) reads - 16 bytes of LDS per entry where the plan counts 8.  Not taken; DESIGN.md says so.
//
// Path 1: the entries, the perf bytes, the workgroup's q and its z in LDS.  L = 1: lane-innermost,
// i * 256 + learner, as in wide_learn_kernel (conflict-free).  L > 1: entry-innermost,
// learner * n_entries + i, so that a team's lanes hit consecutive banks.  Path 2: q and z as they
// lie in global memory, through the L1 / L2 the workgroup's waves share; the entries in LDS when
// they alone fit.  Either way entry i of learner `who` is cell who * sw + i * si of Q and of Z.

constexpr int kTraceMaxTeam = kLearnThreads;

// campx_wide_traces_plan()'s five words, in their order.
struct TracePlan { int64_t path, team, lds_bytes, threads, table_in_lds; };

inline int32_t plan_traces(int64_t S, int32_t has_perf, int64_t B, int64_t lds_max, int32_t path,
                           int32_t team, TracePlan* p, int64_t* plan_out) {
  if (!plan_args_ok(S, has_perf, B, B, lds_max, path) || team < 0 || team > kTraceMaxTeam ||
      (team & (team - 1)))
    return CAMPX_EINVAL;
  const int64_t table = table_bytes(S, has_perf);
  const int64_t per = S * CAMPX_N_ACTIONS * 2 * (int64_t)sizeof(float);      // q and z of a learner
  // the smallest team whose learners fit beside the table (a forced team: that one or none)
  int64_t L = team ? team : 1;
  while (table + (kLearnThreads / L) * per > lds_max && !team && L < kTraceMaxTeam) L *= 2;
  const bool fits = table + (kLearnThreads / L) * per <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  p->path = (path == 1 || (path == 0 && fits)) ? 1 : 2;
  p->team = (p->path == 1 || team) ? L : kTraceMaxTeam;
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? table + (kLearnThreads / L) * per : (p->table_in_lds ? table : 0);
  p->threads = kLearnThreads;
  if (plan_out) memcpy(plan_out, p, sizeof(*p));
  return CAMPX_OK;
}

// Path 1's q or z between global memory - element i of the workgroup's piece `g` is learner
// i / n_entries, entry i % n_entries - and its cells in LDS (kIn: into it, else back out).  `g + head`
// is 16-byte aligned: the elements from there go four at a time, one 16-byte global access and one
// division per group (move_q()'s walk), the at most three before and three after one by one.
template <bool kIn>
__device__ __forceinline__ void move_cells(float* cells, float* g, int n, int n_entries, int si, int sw,
                                           int head, int tid) {
  head = head < n ? head : n;
  const int whole = (n - head) & ~3;
  for (int i = head + tid * 4; i < head + whole; i += kLearnThreads * 4) {
    u32x4* piece = reinterpret_cast<u32x4*>(g + i);
    u32x4 v = kIn ? *piece : u32x4{};
    int who = i / n_entries, k = i - who * n_entries;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float& cell = cells[who * sw + k * si];
      if (kIn) cell = __uint_as_float(v[j]);
      else v[j] = __float_as_uint(cell);
      if (++k == n_entries) {
        k = 0;
        ++who;
      }
    }
    if (!kIn) *piece = v;
  }
  for (int j = tid; j < n - whole; j += kLearnThreads) {
    const int i = j < head ? j : j + whole;
    float& cell = cells[(i / n_entries) * sw + (i % n_entries) * si];
    if (kIn) cell = g[i];
    else g[i] = cell;
  }
}

// kQLds: path 1.  kTableLds, kPerf, kSarsa: as in wide_learn_kernel.  `L`: lanes of a team, a power
// of two, blockDim.x == 256 == G * L.  `replacing`: the trace kind.
template <bool kQLds, bool kTableLds, bool kPerf, bool kSarsa>
__global__ __launch_bounds__(kLearnThreads) void wide_learn_traces_kernel(
    LearnParams pp, const uint2* __restrict__ g_entries, const int8_t* __restrict__ g_perf, float* q,
    float* traces, const float* __restrict__ alphas, const float* __restrict__ gammas,
    const float* __restrict__ epsilons, const float* __restrict__ lams, int32_t* __restrict__ state,
    CampxState st, float* __restrict__ reward_sum, int32_t* __restrict__ perf_sum,
    int32_t* __restrict__ episodes, int32_t* bad_count, int32_t* bad_flag, int64_t B, int32_t T,
    int32_t reset_first, int32_t L, int32_t replacing) {
  static_assert(kTableLds || !kQLds, "path 1 stages the table");
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS;
  const int tid = threadIdx.x;
  const int G = kLearnThreads / L;
  const int who = tid / L, part = tid - who * L;             // learner of the workgroup, lane of the team
  const int64_t first_learner = (int64_t)blockIdx.x * G;
  const int n_here = (int)(B - first_learner < G ? B - first_learner : G);   // learners present
  const bool active = who < n_here;                          // (an absent team: last workgroup only)
  const int64_t learner = first_learner + who;
  const int n_own = n_here * n_entries;                      // floats: B * S * 5 < 2^31
  float* q_block = q + first_learner * n_entries;
  float* z_block = traces + first_learner * n_entries;
  const int head = (int)((0 - first_learner * n_entries) & 3);     // floats up to 16 bytes (q, traces are)
  const StagedTable tab =
      stage_table<kTableLds, kPerf>(lds_tables, g_entries, g_perf, n_entries, tid, kLearnThreads);
  float* l_q = reinterpret_cast<float*>(tab.free);
  float* Q = kQLds ? l_q : q_block;
  float* Z = kQLds ? l_q + G * n_entries : z_block;
  const int si = (kQLds && L == 1) ? kLearnThreads : 1;      // entry i of learner `who`:
  const int sw = (kQLds && L == 1) ? 1 : n_entries;          //   cell who * sw + i * si
  if (kQLds) {
    move_cells<true>(Q, q_block, n_own, n_entries, si, sw, head, tid);
    move_cells<true>(Z, z_block, n_own, n_entries, si, sw, head, tid);
  }
  if (tid < 16) discounts[tid] = pp.discounts[tid];
  __syncthreads();

  // What stays in registers for the run.  An absent lane keeps these values - no learner, a new
  // episode - and does nothing between the barriers below.
  Hyper h;
  float lam = 0.0f;
  Carried c;
  WindowSums<kPerf> win{reward_sum, perf_sum, episodes, learner};
  if (active) {
    h.load(alphas, gammas, epsilons, learner);
    lam = lams[learner];
    h.good = h.good && lam >= 0.0f && lam <= 1.0f;           // (a NaN is in no interval)
    c.load(state, st, learner, S, reset_first);
  }
  const bool lead = part == 0;                               // writes the sums and the final state
  float* own_q = Q + who * sw;
  float* own_z = Z + who * sw;
  const Chunks chunks(pp.first_frame);
  for (int t0 = -chunks.lead; t0 < T; t0 += kLearnChunk) {
    uint32_t x[2 * kLearnChunk];
    if (active) chunks.words(pp, learner, t0, x);
#pragma unroll
    for (int j = 0; j < kLearnChunk; ++j) {
      if (t0 + j < 0 || t0 + j >= T) continue;               // (uniform: kernel arguments alone)
      bool sweep = false, cut = false, ends = false;
      int idx = 0;
      float step = 0.0f, decay = 0.0f;
      if (active) {                                          // ---- (A)
        float row[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) row[k] = own_q[(c.from * CAMPX_N_ACTIONS + k) * si];
        const uint32_t a = frame_action(row, x[2 * j], x[2 * j + 1], h.epsilon, h.good);
        idx = (int)(c.from * CAMPX_N_ACTIONS + a);
        const Entry e = decode_entry(tab.entries[idx], S, discounts);
        if (h.good) {
          float nrow[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) nrow[k] = own_q[(e.next * CAMPX_N_ACTIONS + k) * si];
          float old = row[0], best;
#pragma unroll
          for (int k = 1; k < 5; ++k) old = a == (uint32_t)k ? row[k] : old;
          uint32_t unused;
          greedy_of(row, best, unused);
          const float delta = td_error<kSarsa>(old, nrow, e, h.gamma, h.keep, h.epsilon);
          step = h.alpha * delta;
          decay = (h.gamma * e.D) * lam;
          cut = (!kSarsa && !(old == best)) || (reset_first && t0 + j == 0);
          ends = e.done != 0u;
          sweep = true;
        }
        c.advance(e);
        if (lead) win.add(pp, e.r, kPerf ? tab.perf_tab[idx] : 0, e.done, B);
      }
      if (L > 1) __syncthreads();
      if (sweep) {                                           // ---- (B)
        for (int i = part; i < n_entries; i += L) {
          float z = own_z[i * si];
          z = cut ? 0.0f : z;
          if (i == idx) z = replacing ? 1.0f : z + 1.0f;
          if (z != 0.0f) own_q[i * si] = own_q[i * si] + step * z;
          own_z[i * si] = ends ? 0.0f : decay * z;
        }
      }
      if (L > 1) __syncthreads();
    }
  }
  if (active && lead) {
    win.flush_short();
    c.store(state, st, learner);
    report_bad(bad_count, bad_flag, h.good ? 0 : 1);         // bad LEARNERS, once per launch
  }
  if (kQLds) {
    __syncthreads();
    move_cells<false>(Q, q_block, n_own, n_entries, si, sw, head, tid);
    move_cells<false>(Z, z_block, n_own, n_entries, si, sw, head, tid);
  }
}

using TraceKernel = decltype(&wide_learn_traces_kernel<false, false, false, false>);
static const TraceKernel kTraceKernels[3][2][2] = CAMPX_LEARN_INSTANCES(wide_learn_traces_kernel);

// ---------------------------------------------------------------------------------------------
// Dyna-Q: wide_learn_kernel's frame, then `planning[e]` updates of remembered pairs (include/
// campx_hip.h, "Dyna-Q online learners", has the frame; tests/dyna_learner_reference.py restates it
// in numpy).  The game is deterministic and its table is what the workgroup already holds, so a
// learner's model is the LIST of the flat entries it has met - `seen`, in order of first visit -
// and a membership bitmap that answers "is this pair new" in one read.  A lane per learner, 256 to
// a workgroup, nothing shared between lanes: no barrier inside the frame loop.  The chain per frame
// is  row -> action -> entry -> bootstrap row -> write -> (bit test, append) -> n x (word -> list
// element -> entry -> bootstrap row -> write) -> the next row, RE-READ: planning may have written
// any element of it, so the register patch of wide_learn_kernel does not carry over - except for a
// learner with planning[e] = 0, which keeps the patch and the one-step learner's chain.
//
// Path 1: entries, perf bytes, q (move_q(), lane-innermost) and, after them, the lists as 16-bit
// elements [5S][256] and the bitmap [W][256] in LDS.  A 16-bit list that were simply lane-innermost
// would put lanes 2j and 2j + 1 in one dword - one bank, two addresses whenever their indices
// differ: a two-way conflict on every planning read.  dyna_slot() keeps the bytes and moves the
// lanes: the 32 lanes of a half wave (the group a 16- or 32-bit LDS access is served in) take 32
// different dwords, and the half waves 2h and 2h + 1 share them as low and high halves.
// Path 2: q, seen (int32, as it lies) and the bitmap `marks` through L1 / L2.

// campx_wide_dyna_plan()'s five words, in their order.
struct DynaPlan { int64_t path, lds_bytes, threads, table_in_lds, words; };

inline int32_t plan_dyna(int64_t S, int32_t has_perf, int64_t B, int64_t lds_max, int32_t path,
                         DynaPlan* p, int64_t* plan_out) {
  if (!plan_args_ok(S, has_perf, B, B, lds_max, path)) return CAMPX_EINVAL;
  const int64_t n_entries = S * CAMPX_N_ACTIONS, words = (n_entries + 31) / 32;
  const int64_t table = table_bytes(S, has_perf);
  const int64_t want = table + kLearnThreads * (n_entries * (int64_t)(sizeof(float) + sizeof(uint16_t)) +
                                                words * (int64_t)sizeof(uint32_t));
  const bool fits = want <= lds_max && n_entries <= 65536;       // (a list element is 16 bits there)
  if (path == 1 && !fits) return CAMPX_EINVAL;
  p->path = (path == 1 || (path == 0 && fits)) ? 1 : 2;
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? want : (p->table_in_lds ? table : 0);
  p->threads = kLearnThreads;
  p->words = words;
  if (plan_out) memcpy(plan_out, p, sizeof(*p));
  return CAMPX_OK;
}

// Where lane `t` sits in a row of 256 16-bit elements: dword (t & 31) + 32 * (t >> 6), half (t >> 5) & 1.
__device__ __forceinline__ int dyna_slot(int t) {
  return ((((t & 31) | ((t >> 6) << 5)) << 1) | ((t >> 5) & 1));
}

// One planning update of entry `i` of the lane's table: td_error() on the entry the game's table
// has for it, the bootstrap row read before the write.
template <bool kSarsa, int step>
__device__ __forceinline__ void plan_update(float* own, uint32_t i, const uint2* entries, int S,
                                            const float* discounts, const Hyper& h) {
  const Entry e = decode_entry(entries[i], S, discounts);
  float nrow[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) nrow[k] = own[(e.next * CAMPX_N_ACTIONS + k) * step];
  const float old = own[i * step];
  const float delta = td_error<kSarsa>(old, nrow, e, h.gamma, h.keep, h.epsilon);
  own[i * step] = old + h.alpha * delta;
}

// kQLds: path 1.  kTableLds, kPerf, kSarsa: as in wide_learn_kernel.  `words`: bitmap words of a
// learner, ceil(n_states * 5 / 32).  `marks`: path 2's bitmap, unused on path 1.
template <bool kQLds, bool kTableLds, bool kPerf, bool kSarsa>
__global__ __launch_bounds__(kLearnThreads) void wide_learn_dyna_kernel(
    LearnParams pp, const uint2* __restrict__ g_entries, const int8_t* __restrict__ g_perf,
    float* __restrict__ q, const float* __restrict__ alphas, const float* __restrict__ gammas,
    const float* __restrict__ epsilons, int32_t* __restrict__ seen, int32_t* __restrict__ n_seen,
    const int32_t* __restrict__ planning, uint32_t* __restrict__ marks, int32_t* __restrict__ state,
    CampxState st, float* __restrict__ reward_sum, int32_t* __restrict__ perf_sum,
    int32_t* __restrict__ episodes, int32_t* bad_count, int32_t* bad_flag, int64_t B, int32_t T,
    int32_t reset_first, int32_t words) {
  static_assert(kTableLds || !kQLds, "path 1 stages the table");
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS;
  const int lane = threadIdx.x;
  const int64_t env_lo = (int64_t)blockIdx.x * kLearnThreads;
  const int64_t env = env_lo + lane;
  const int n_lanes = (int)(B - env_lo < kLearnThreads ? B - env_lo : kLearnThreads);
  const int n_q = n_lanes * n_entries;                 // floats: B * S * 5 < 2^31
  float* q_block = q + env_lo * n_entries;
  const StagedTable tab =
      stage_table<kTableLds, kPerf>(lds_tables, g_entries, g_perf, n_entries, lane, kLearnThreads);
  float* l_q = reinterpret_cast<float*>(tab.free);
  if (kQLds) move_q<true>(l_q, q_block, n_q, n_entries, lane);
  if (lane < 16) discounts[lane] = pp.discounts[lane];
  __syncthreads();

  if (env < B) {
    Hyper h;
    h.load(alphas, gammas, epsilons, env);
    float* own = kQLds ? l_q + lane : q + env * n_entries;
    constexpr int step = kQLds ? kLearnThreads : 1;
    // the lane's list and bitmap: element k at list16[k * 256] (path 1) or list32[k] (path 2), word
    // w at bits[w * bstep].  Nobody else touches them.
    uint16_t* list16 = reinterpret_cast<uint16_t*>(l_q + n_entries * kLearnThreads) + dyna_slot(lane);
    int32_t* list32 = seen + env * n_entries;
    uint32_t* bits = kQLds ? reinterpret_cast<uint32_t*>(l_q) + n_entries * (kLearnThreads * 3 / 2) + lane
                           : marks + env * words;
    constexpr int bstep = kQLds ? kLearnThreads : 1;
    // screen the list and rebuild the bitmap from it; a list that fails makes the learner bad
    const int n_plan = planning[env];
    const int n_old = n_seen[env];
    bool list_ok = n_old >= 0 && n_old <= n_entries;
    for (int w = 0; w < words; ++w) bits[w * bstep] = 0u;
    for (int k = 0; k < (list_ok ? n_old : 0); ++k) {
      const uint32_t i = (uint32_t)list32[k];
      if (i < (uint32_t)n_entries) {
        bits[(i >> 5) * bstep] |= 1u << (i & 31);
        if (kQLds) list16[k * kLearnThreads] = (uint16_t)i;
      } else {
        list_ok = false;
      }
    }
    h.good = h.good && list_ok && n_plan >= 0 && n_plan <= CAMPX_DYNA_MAX_PLANNING;
    int n = n_old;                                     // (only a good learner's n is used)

    Carried c;
    c.load(state, st, env, S, reset_first);
    float row[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) row[a] = own[(c.from * CAMPX_N_ACTIONS + a) * step];
    WindowSums<kPerf> sums{reward_sum, perf_sum, episodes, env};
    const Chunks chunks(pp.first_frame);
    for (int t0 = -chunks.lead; t0 < T; t0 += kLearnChunk) {
      uint32_t x[2 * kLearnChunk];
      chunks.words(pp, env, t0, x);
#pragma unroll
      for (int j = 0; j < kLearnChunk; ++j) {
        if (t0 + j >= 0 && t0 + j < T) {
          const uint32_t a = frame_action(row, x[2 * j], x[2 * j + 1], h.epsilon, h.good);
          const uint32_t idx = c.from * CAMPX_N_ACTIONS + a;
          const Entry e = decode_entry(tab.entries[idx], S, discounts);
          // the next frame's row before this frame's write: the bootstrap row, as in wide_learn_kernel
          float nrow[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) nrow[k] = own[(e.next * CAMPX_N_ACTIONS + k) * step];
          if (h.good) {
            float old = row[0];
#pragma unroll
            for (int k = 1; k < 5; ++k) old = a == (uint32_t)k ? row[k] : old;
            const float delta = td_error<kSarsa>(old, nrow, e, h.gamma, h.keep, h.epsilon);
            const float fresh = old + h.alpha * delta;
            own[idx * step] = fresh;
            if (e.next == c.from) {
#pragma unroll
              for (int k = 0; k < 5; ++k) nrow[k] = a == (uint32_t)k ? fresh : nrow[k];
            }
            // record: n < n_entries whenever the pair is new - the bitmap holds every listed pair,
            // so a list of n_entries elements without a repeat has no new pair left, and one WITH
            // repeats is checked here
            const uint32_t word = bits[(idx >> 5) * bstep], bit = 1u << (idx & 31);
            if (!(word & bit) && n < n_entries) {
              bits[(idx >> 5) * bstep] = word | bit;
              if (kQLds) list16[n * kLearnThreads] = (uint16_t)idx;
              else list32[n] = (int32_t)idx;
              ++n;
            }
            // plan: n >= 1 here, the pair just met is listed
            const uint64_t f = (uint64_t)(pp.first_frame + t0 + j);
            for (int k0 = 0; k0 < n_plan; k0 += 4) {
              uint32_t y[4];
              philox4x32_10((uint32_t)env, (uint32_t)f, (uint32_t)(f >> 32), 2u + (uint32_t)(k0 >> 2),
                            pp.key0, pp.key1, y);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                if (k0 + k < n_plan) {
                  const uint32_t at = __umulhi(y[k], (uint32_t)n);
                  const uint32_t i = kQLds ? (uint32_t)list16[at * kLearnThreads] : (uint32_t)list32[at];
                  plan_update<kSarsa, step>(own, i, tab.entries, S, discounts, h);
                }
              }
            }
            // the next frame's row as planning left the table: any step may have written it, so it
            // is read again; without planning wide_learn_kernel's patch above is the whole change
            if (n_plan > 0) {
#pragma unroll
              for (int k = 0; k < 5; ++k) nrow[k] = own[(e.next * CAMPX_N_ACTIONS + k) * step];
            }
          }
#pragma unroll
          for (int k = 0; k < 5; ++k) row[k] = nrow[k];
          c.advance(e);
          sums.add(pp, e.r, kPerf ? tab.perf_tab[idx] : 0, e.done, B);
        }
      }
    }
    sums.flush_short();
    c.store(state, st, env);
    if (h.good) {
      // the elements the launch appended, and the count; nothing before n_old, nothing from n on
      if (kQLds)
        for (int k = n_old; k < n; ++k) list32[k] = (int32_t)list16[k * kLearnThreads];
      n_seen[env] = n;
    }
    report_bad(bad_count, bad_flag, h.good ? 0 : 1);     // bad LEARNERS, once per launch
  }

  if (kQLds) {
    __syncthreads();
    move_q<false>(l_q, q_block, n_q, n_entries, lane);
  }
}

using DynaKernel = decltype(&wide_learn_dyna_kernel<false, false, false, false>);
static const DynaKernel kDynaKernels[3][2][2] = CAMPX_LEARN_INSTANCES(wide_learn_dyna_kernel);

// ---------------------------------------------------------------------------------------------
// Actor-critic: one-step actor-critic with a softmax policy per learner (include/campx_hip.h,
// "Actor-critic online learners", has the frame; tests/actor_critic_reference.py restates it in
// numpy).  wide_learn_kernel's schedule - a lane per learner, 256 to a workgroup, nothing shared
// between lanes, no barrier inside the frame loop - with two tables per learner, the preferences
// `prefs[e]` [S][5] and the critic's `values[e]` [S], and k_policy.hip's sampler in place of the
// epsilon-greedy choice: the weights are softmax_weights() of the state's row (wide_table.hip.h: a
// stated f32 rule, not expf()), the thresholds policy_thresholds(), the random word that of
// rollout_policy() - word f & 3 of the block with counter (e, f >> 2, 0) - so a learner whose step
// sizes are 0 walks exactly as rollout_population() walks its weights.  The chain per frame is
// row -> five weights -> thresholds -> action -> entry -> values[s], values[n] -> delta -> one write
// of values, five of prefs -> the next row, RE-READ (the frame wrote all five elements of row s,
// and n may be s).  No epsilon and no rule: Hyper, frame_action() and td_error() are not used.
//
// Path 1: the entries, the perf bytes, prefs (move_q(), lane-innermost, (s * 5 + a) * 256 + lane)
// and, after them, values (move_q() with rows of one element, s * 256 + lane) in LDS: 24 bytes a
// state and learner.  Path 2: prefs and values through L1 / L2, the entries in LDS when they fit.

// campx_wide_actor_plan()'s four words, in their order (LearnPlan's).
inline int32_t plan_actor(int64_t S, int32_t has_perf, int64_t B, int64_t lds_max, int32_t path,
                          LearnPlan* p, int64_t* plan_out) {
  if (!plan_args_ok(S, has_perf, B, B, lds_max, path)) return CAMPX_EINVAL;
  const int64_t table = table_bytes(S, has_perf);
  const int64_t want = table + kLearnThreads * S * (CAMPX_N_ACTIONS + 1) * (int64_t)sizeof(float);
  const bool fits = want <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  p->path = (path == 1 || (path == 0 && fits)) ? 1 : 2;
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? want : (p->table_in_lds ? table : 0);
  p->threads = kLearnThreads;
  if (plan_out) memcpy(plan_out, p, sizeof(*p));
  return CAMPX_OK;
}

// kQLds: path 1.  kTableLds, kPerf: as in wide_learn_kernel.  `bad_rows`: environment-frames of
// good learners that met a row that is not good; `bad_count`: bad learners, once per launch.
template <bool kQLds, bool kTableLds, bool kPerf>
__global__ __launch_bounds__(kLearnThreads) void wide_learn_actor_kernel(
    LearnParams pp, const uint2* __restrict__ g_entries, const int8_t* __restrict__ g_perf,
    float* __restrict__ prefs, float* __restrict__ values, const float* __restrict__ alpha_actors,
    const float* __restrict__ alpha_critics, const float* __restrict__ gammas,
    int32_t* __restrict__ state, CampxState st, float* __restrict__ reward_sum,
    int32_t* __restrict__ perf_sum, int32_t* __restrict__ episodes, int32_t* bad_count,
    int32_t* bad_rows, int32_t* bad_flag, int64_t B, int32_t T, int32_t reset_first) {
  static_assert(kTableLds || !kQLds, "path 1 stages the table");
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS;
  const int lane = threadIdx.x;
  const int64_t env_lo = (int64_t)blockIdx.x * kLearnThreads;
  const int64_t env = env_lo + lane;
  // this workgroup's learners and their pieces of prefs and values: contiguous, 16-byte aligned
  // (both tensors are, and a piece starts a multiple of 256 * 4 bytes in)
  const int n_lanes = (int)(B - env_lo < kLearnThreads ? B - env_lo : kLearnThreads);
  float* h_block = prefs + env_lo * n_entries;         // floats: B * S * 5 < 2^31
  float* v_block = values + env_lo * S;
  const StagedTable tab =
      stage_table<kTableLds, kPerf>(lds_tables, g_entries, g_perf, n_entries, lane, kLearnThreads);
  float* l_h = reinterpret_cast<float*>(tab.free);
  float* l_v = l_h + n_entries * kLearnThreads;
  if (kQLds) {
    move_q<true>(l_h, h_block, n_lanes * n_entries, n_entries, lane);
    move_q<true>(l_v, v_block, n_lanes * S, S, lane);
  }
  if (lane < 16) discounts[lane] = pp.discounts[lane];
  __syncthreads();

  if (env < B) {
    const float alpha_actor = alpha_actors[env], alpha_critic = alpha_critics[env], gamma = gammas[env];
    // (x - x is 0 exactly for a finite x, NaN for an infinity or a NaN)
    const bool good = (alpha_actor - alpha_actor) == 0.0f && (alpha_critic - alpha_critic) == 0.0f &&
                      (gamma - gamma) == 0.0f;
    // the lane's tables: element (s, a) of prefs at own_h[(s * 5 + a) * step], values[s] at own_v[s * step]
    float* own_h = kQLds ? l_h + lane : prefs + env * n_entries;
    float* own_v = kQLds ? l_v + lane : values + env * S;
    constexpr int step = kQLds ? kLearnThreads : 1;
    Carried c;
    c.load(state, st, env, S, reset_first);
    WindowSums<kPerf> sums{reward_sum, perf_sum, episodes, env};
    const Chunks chunks(pp.first_frame);
    int n_bad_rows = 0;
    for (int t0 = -chunks.lead; t0 < T; t0 += kLearnChunk) {
      // rollout_policy()'s block of the chunk's four absolute frames: fourth counter word 0
      uint32_t x[kLearnChunk];
      const uint64_t g = (chunks.pair0 >> 1) + (uint64_t)((t0 + chunks.lead) >> 2);
      philox4x32_10((uint32_t)env, (uint32_t)g, (uint32_t)(g >> 32), 0u, pp.key0, pp.key1, x);
#pragma unroll
      for (int j = 0; j < kLearnChunk; ++j) {
        if (t0 + j >= 0 && t0 + j < T) {
          const uint32_t base = c.from * CAMPX_N_ACTIONS;
          float h[5], w[5], thr[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) h[k] = own_h[(base + k) * step];
          const bool row_good = softmax_weights(h, w) && good;
          if (!row_good) {
#pragma unroll
            for (int k = 0; k < 5; ++k) w[k] = 0.0f;   // (a bad learner: action 4 throughout)
          }
          policy_thresholds(w, thr);
          const float u = (float)(x[j] >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
          const float r = u * thr[4];
          const uint32_t a = (uint32_t)(r >= thr[0]) + (uint32_t)(r >= thr[1]) +
                             (uint32_t)(r >= thr[2]) + (uint32_t)(r >= thr[3]);
          n_bad_rows += good && !row_good;
          const uint32_t idx = base + a;
          const Entry e = decode_entry(tab.entries[idx], S, discounts);
          if (row_good) {
            // both values as the frame found them
            const float v_s = own_v[c.from * step], v_n = own_v[e.next * step];
            const float discounted = (gamma * e.D) * v_n;
            const float target = e.done ? e.r : e.r + discounted;
            const float delta = target - v_s;
            own_v[c.from * step] = v_s + alpha_critic * delta;
            const float push = alpha_actor * delta;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
              const float pi = w[k] / thr[4];
              const float grad = (a == (uint32_t)k ? 1.0f : 0.0f) - pi;
              own_h[(base + k) * step] = h[k] + push * grad;
            }
          }
          c.advance(e);
          sums.add(pp, e.r, kPerf ? tab.perf_tab[idx] : 0, e.done, B);
        }
      }
    }
    sums.flush_short();
    c.store(state, st, env);
    report_bad(bad_count, bad_flag, good ? 0 : 1);       // bad LEARNERS, once per launch
    // bad ROWS, per environment-frame.  (The count is added here and not handed to report_bad():
    // every other call of this file passes it 0 or 1, which the compiler knows and uses in the
    // older kernels - an arbitrary count from here would change their instructions.)
    if (n_bad_rows) {
      if (bad_rows) atomicAdd(bad_rows, n_bad_rows);
      report_bad(nullptr, bad_flag, 1);
    }
  }

  if (kQLds) {
    __syncthreads();
    move_q<false>(l_h, h_block, n_lanes * n_entries, n_entries, lane);
    move_q<false>(l_v, v_block, n_lanes * S, S, lane);
  }
}

// At [where the tables are][kPerf], the first index as in CAMPX_LEARN_INSTANCES.
using ActorKernel = decltype(&wide_learn_actor_kernel<false, false, false>);
static const ActorKernel kActorKernels[3][2] = {
    {wide_learn_actor_kernel<0, 0, 0>, wide_learn_actor_kernel<0, 0, 1>},
    {wide_learn_actor_kernel<0, 1, 0>, wide_learn_actor_kernel<0, 1, 1>},
    {wide_learn_actor_kernel<1, 1, 0>, wide_learn_actor_kernel<1, 1, 1>}};

// ---------------------------------------------------------------------------------------------
// Shared actor-critic: P softmax policies and critics, each fed by the n = B / P consecutive
// environments of its block - synchronous advantage actor-critic (include/campx_hip.h, "Shared
// actor-critic learners", has the frame; tests/shared_actor_reference.py restates it in numpy).
// wide_learn_shared_kernel's schedule and arithmetic - G whole learners per workgroup, two barriers
// a frame, the errors quantised to 64-bit fixed point and added as INTEGERS, the owner by the first
// add - with wide_learn_actor_kernel's frame: softmax_weights(), policy_thresholds(),
// rollout_policy()'s sampler and stream, the bad-row rule.  A frame is
//   (A) row, weights, action, entry, values[s] and values[n] as the frame found them, delta;
//       sum[s][a] += z and visitors[s] += 1 (workgroup-scope atomics) - the lane whose visitor-add
//       returned 0 owns STATE s;
//   barrier;
//   (B) the owner exchanges the state's five sums and its visitor count for 0 and writes values[s]
//       and the five preferences of row s, from the row, the weights and the value it still holds
//       in registers (it is in s itself);
//   barrier.
// EVERY lane of the workgroup reaches both barriers of every frame: the loop bounds depend on the
// kernel's arguments alone, and what an absent lane, a lane of a bad learner or a lane on a bad row
// skips lies BETWEEN the barriers, never around one.
//
// Path 1: the entries, the perf bytes and per learner the sums, prefs, values and visitor counts in
// LDS - 40 + 20 + 4 + 4 = 68 bytes a state; prefs and values are copied straight in and out.
// Path 2: prefs, values and the accumulators - `scratch`, zero on entry and left zero by the
// exchanges of (B) - in global memory; the entries in LDS when they alone fit.

constexpr int64_t kSharedActorBytesPerState = 68;    // path 1, per (learner, state)
constexpr int64_t kSharedActorScratchPerState = 44;  // path 2, per (learner, state): sums 40, visitors 4

// campx_wide_actor_shared_plan()'s six words: SharedPlan's, by plan_shared()'s rule.
inline int32_t plan_actor_shared(int64_t S, int32_t has_perf, int64_t B, int64_t P, int64_t lds_max,
                                 int32_t path, SharedPlan* p, int64_t* plan_out) {
  return plan_shared_rule(S, has_perf, B, P, lds_max, path, kSharedActorBytesPerState, p, plan_out);
}

// double(Z) / double(N) * 2^-32 as a float: the mean of N quantised errors that sum to Z.
__device__ __forceinline__ float shared_mean(long long Z, double visitors) {
  return (float)(((double)Z / visitors) * (1.0 / kSharedScale));
}

// kQLds: path 1.  kTableLds, kPerf: as in wide_learn_kernel.  `n`: environments per learner; `G`:
// learners per workgroup, blockDim.x == G * n.  `acc_sum` [P][S][5] / `acc_visits` [P][S]: path 2's
// accumulators.  `bad_rows`, `bad_count`: as in wide_learn_actor_kernel, the latter per LEARNER.
template <bool kQLds, bool kTableLds, bool kPerf>
__global__ __launch_bounds__(kSharedMaxThreads) void wide_learn_actor_shared_kernel(
    LearnParams pp, const uint2* __restrict__ g_entries, const int8_t* __restrict__ g_perf,
    float* prefs, float* values, const float* __restrict__ alpha_actors,
    const float* __restrict__ alpha_critics, const float* __restrict__ gammas,
    int32_t* __restrict__ state, CampxState st, float* __restrict__ reward_sum,
    int32_t* __restrict__ perf_sum, int32_t* __restrict__ episodes, long long* __restrict__ clamped,
    long long* acc_sum, uint32_t* acc_visits, int32_t* bad_count, int32_t* bad_rows, int32_t* bad_flag,
    int64_t B, int64_t P, int32_t n, int32_t G, int32_t T, int32_t reset_first) {
  static_assert(kTableLds || !kQLds, "path 1 stages the table");
  extern __shared__ __attribute__((aligned(16))) uint2 lds_tables[];
  __shared__ float discounts[16];
  __shared__ unsigned long long l_clamped[kSharedPack];      // per learner of the workgroup
  const int S = pp.n_states, n_entries = S * CAMPX_N_ACTIONS;
  const int tid = threadIdx.x, threads = blockDim.x;
  const int64_t first_learner = (int64_t)blockIdx.x * G;
  const int n_here = (int)(P - first_learner < G ? P - first_learner : G);   // learners present
  const int64_t env = first_learner * n + tid;
  const int who = tid / n;                                   // learner of the workgroup
  const bool active = who < n_here;                          // (an absent lane: last workgroup only)
  const int64_t m = first_learner + who;
  float* h_block = prefs + first_learner * n_entries;        // floats: P * S * 5 < 2^31
  float* v_block = values + first_learner * S;
  float *h_tab = h_block, *v_tab = v_block;                  // [learner][s][a], [learner][s], wherever they are
  long long* sums = kQLds ? nullptr : acc_sum + first_learner * n_entries;
  uint32_t* visits = kQLds ? nullptr : acc_visits + first_learner * S;
  const StagedTable tab =
      stage_table<kTableLds, kPerf>(lds_tables, g_entries, g_perf, n_entries, tid, threads);
  if (kQLds) {
    // [sums G x S x 5 x 8][prefs G x S x 5 x 4][values G x S x 4][visitors G x S x 4], 16-byte aligned
    sums = reinterpret_cast<long long*>(tab.free);
    h_tab = reinterpret_cast<float*>(sums + (int64_t)G * n_entries);
    v_tab = h_tab + (int64_t)G * n_entries;
    visits = reinterpret_cast<uint32_t*>(v_tab + (int64_t)G * S);
    for (int i = tid; i < n_here * n_entries; i += threads) {
      h_tab[i] = h_block[i];
      sums[i] = 0;
    }
    for (int i = tid; i < n_here * S; i += threads) {
      v_tab[i] = v_block[i];
      visits[i] = 0u;
    }
  }
  // (strided: a workgroup of G * n threads may have fewer than 16, down to one)
  for (int i = tid; i < 16; i += threads) discounts[i] = pp.discounts[i];
  for (int i = tid; i < kSharedPack; i += threads) l_clamped[i] = 0ull;
  __syncthreads();

  // What stays in registers for the run.  An absent lane keeps these values - no learner, a new
  // episode, empty sums - and does nothing between the barriers below.
  float alpha_actor = 0.0f, alpha_critic = 0.0f, gamma = 0.0f;
  bool good = false;
  Carried c;
  WindowSums<kPerf> win{reward_sum, perf_sum, episodes, env};
  unsigned long long n_clamped = 0ull;
  int n_bad_rows = 0;
  const int own_h = who * n_entries, own_v = who * S;        // the learner's rows start here
  if (active) {
    alpha_actor = alpha_actors[m], alpha_critic = alpha_critics[m], gamma = gammas[m];
    // (x - x is 0 exactly for a finite x, NaN for an infinity or a NaN)
    good = (alpha_actor - alpha_actor) == 0.0f && (alpha_critic - alpha_critic) == 0.0f &&
           (gamma - gamma) == 0.0f;
    c.load(state, st, env, S, reset_first);
  }
  const Chunks chunks(pp.first_frame);
  for (int t0 = -chunks.lead; t0 < T; t0 += kLearnChunk) {
    // rollout_policy()'s block of the chunk's four absolute frames: fourth counter word 0
    uint32_t x[kLearnChunk] = {0u, 0u, 0u, 0u};
    if (active) {
      const uint64_t g = (chunks.pair0 >> 1) + (uint64_t)((t0 + chunks.lead) >> 2);
      philox4x32_10((uint32_t)env, (uint32_t)g, (uint32_t)(g >> 32), 0u, pp.key0, pp.key1, x);
    }
#pragma unroll
    for (int j = 0; j < kLearnChunk; ++j) {
      if (t0 + j < 0 || t0 + j >= T) continue;               // (uniform: kernel arguments alone)
      bool owner = false;
      int row_at = 0, cell = 0;                              // own_h + s * 5, own_v + s
      float h[5], w[5], total = 0.0f, v_s = 0.0f;
#pragma unroll
      for (int k = 0; k < 5; ++k) h[k] = w[k] = 0.0f;
      if (active) {                                          // ---- (A)
        const uint32_t base = c.from * CAMPX_N_ACTIONS;
        row_at = own_h + (int)base;
        cell = own_v + (int)c.from;
        float thr[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) h[k] = h_tab[row_at + k];
        const bool row_good = softmax_weights(h, w) && good;
        if (!row_good) {
#pragma unroll
          for (int k = 0; k < 5; ++k) w[k] = 0.0f;           // (a bad learner: action 4 throughout)
        }
        policy_thresholds(w, thr);
        total = thr[4];
        const float u = (float)(x[j] >> 8) * 5.9604644775390625e-8f;     // 2^-24: exact
        const float r = u * thr[4];
        const uint32_t a = (uint32_t)(r >= thr[0]) + (uint32_t)(r >= thr[1]) +
                           (uint32_t)(r >= thr[2]) + (uint32_t)(r >= thr[3]);
        n_bad_rows += good && !row_good;
        const uint32_t idx = base + a;
        const Entry e = decode_entry(tab.entries[idx], S, discounts);
        if (row_good) {
          // both values as the frame found them, for every lane of the learner
          v_s = v_tab[cell];
          const float v_n = v_tab[own_v + (int)e.next];
          const float discounted = (gamma * e.D) * v_n;
          const float target = e.done ? e.r : e.r + discounted;
          const float delta = target - v_s;
          const double d = (double)delta * kSharedScale;
          long long z;
          if (!(fabs(d) <= kSharedLimit)) {                  // NaN, +-Inf, past the limit
            ++n_clamped;
            z = d != d ? 0ll : (d > 0.0 ? kSharedLimitQ : -kSharedLimitQ);
          } else {
            z = __double2ll_rn(d);
          }
          owner = __hip_atomic_fetch_add(&visits[cell], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_WORKGROUP) == 0u;
          __hip_atomic_fetch_add(&sums[own_h + (int)idx], z, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        c.advance(e);
        win.add(pp, e.r, kPerf ? tab.perf_tab[idx] : 0, e.done, B);
      }
      __syncthreads();
      if (owner) {                                           // ---- (B)
        long long Z[5], Zall = 0ll;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          Z[k] = __hip_atomic_exchange(&sums[row_at + k], 0ll, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
          Zall += Z[k];                                      // (1 024 values of at most 2^52: no overflow)
        }
        const double visitors = (double)__hip_atomic_exchange(&visits[cell], 0u, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_WORKGROUP);
        const float mean_all = shared_mean(Zall, visitors);
        v_tab[cell] = v_s + alpha_critic * mean_all;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const float pi = w[k] / total;
          const float grad = shared_mean(Z[k], visitors) - pi * mean_all;
          h_tab[row_at + k] = h[k] + alpha_actor * grad;
        }
      }
      __syncthreads();
    }
  }
  if (active) {
    win.flush_short();
    c.store(state, st, env);
    if (n_clamped)
      __hip_atomic_fetch_add(&l_clamped[who], n_clamped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tid == who * n) report_bad(bad_count, bad_flag, good ? 0 : 1);       // bad LEARNERS, once
    // bad ROWS, per environment-frame (added here, as in wide_learn_actor_kernel)
    if (n_bad_rows) {
      if (bad_rows) atomicAdd(bad_rows, n_bad_rows);
      report_bad(nullptr, bad_flag, 1);
    }
  }
  __syncthreads();
  if (active && tid == who * n) clamped[m] = (long long)l_clamped[who];
  if (kQLds) {
    for (int i = tid; i < n_here * n_entries; i += threads) h_block[i] = h_tab[i];
    for (int i = tid; i < n_here * S; i += threads) v_block[i] = v_tab[i];
  }
}

// At [where the tables are][kPerf], the first index as in CAMPX_LEARN_INSTANCES.
using SharedActorKernel = decltype(&wide_learn_actor_shared_kernel<false, false, false>);
static const SharedActorKernel kSharedActorKernels[3][2] = {
    {wide_learn_actor_shared_kernel<0, 0, 0>, wide_learn_actor_shared_kernel<0, 0, 1>},
    {wide_learn_actor_shared_kernel<0, 1, 0>, wide_learn_actor_shared_kernel<0, 1, 1>},
    {wide_learn_actor_shared_kernel<1, 1, 0>, wide_learn_actor_shared_kernel<1, 1, 1>}};

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
  const int32_t screened = screen_learner(s, tables_dev, st, l, B, T, true);
  if (screened != CAMPX_OK) return screened;
  LearnPlan plan;      // (refuses B * n_states * 5 >= 2^31, and path 1 for what does not fit)
  const int32_t planned = plan_learn(s->n_states, l->perf_sum ? 1 : 0, B, knob(K_WIDE_LDS_MAX),
                                     l->path, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const WideTables t = wide_tables(*s, tables_dev);
  const size_t lds = (size_t)plan.lds_bytes;
  const LearnKernel kernel = pick_kernel(kLearnKernels, plan, *l);
  CAMPX_ALLOW_LDS(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kLearnThreads - 1) / kLearnThreads)),
                     dim3(kLearnThreads), lds, static_cast<hipStream_t>(stream), learn_params(*s, *l),
                     t.entries, t.perf, l->q, l->alpha, l->gamma, l->epsilon,
                     reinterpret_cast<int32_t*>(st.pos), st, l->reward_sum, l->perf_sum, l->episodes,
                     l->bad_count, l->bad_flag, B, T, l->reset_first);
  return launch_status();
}

int32_t campx_wide_shared_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t P,
                               int64_t wide_lds_max, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SharedPlan plan;
  return plan_shared(n_states, has_perf, B, P, wide_lds_max, path, &plan, plan_out);
}

int64_t campx_wide_shared_scratch_bytes(int64_t n_states, int64_t P) {
  if (n_states < 1 || n_states > CAMPX_WIDE_MAX_STATES || P < 1 || P > 0xffffffffll ||
      P * n_states * CAMPX_N_ACTIONS >= (1ll << 31))
    return 0;
  return P * n_states * CAMPX_N_ACTIONS * 12;
}

int32_t campx_wide_shared_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                                 const CampxSharedLearner* l, int64_t B, int32_t T, void* stream) {
  const bool own_ok = l && l->clamped && aligned_to(l->clamped, 8) && aligned_to(l->scratch, 8) &&
                      l->n_learners >= 1 && l->scratch_bytes >= 0;
  const int32_t screened = screen_learner(s, tables_dev, st, l, B, T, own_ok);
  if (screened != CAMPX_OK) return screened;
  const int64_t P = l->n_learners;
  SharedPlan plan;     // (refuses a P that does not divide B, n > 1024, P * n_states * 5 >= 2^31)
  const int32_t planned = plan_shared(s->n_states, l->perf_sum ? 1 : 0, B, P, knob(K_WIDE_LDS_MAX),
                                      l->path, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const int64_t n_bins = P * s->n_states * CAMPX_N_ACTIONS;
  if (plan.path == 2 && (!l->scratch || l->scratch_bytes < n_bins * 12)) return CAMPX_EINVAL;
  const WideTables t = wide_tables(*s, tables_dev);
  const size_t lds = (size_t)plan.lds_bytes;
  const SharedKernel kernel = pick_kernel(kSharedKernels, plan, *l);
  CAMPX_ALLOW_LDS(kernel, lds);
  // path 2's accumulators: [sums int64 x bins][counts uint32 x bins]
  long long* acc_sum = plan.path == 2 ? static_cast<long long*>(l->scratch) : nullptr;
  uint32_t* acc_count = plan.path == 2 ? reinterpret_cast<uint32_t*>(acc_sum + n_bins) : nullptr;
  const int64_t G = plan.learners;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((P + G - 1) / G)), dim3((unsigned)plan.threads), lds,
                     static_cast<hipStream_t>(stream), learn_params(*s, *l), t.entries, t.perf, l->q,
                     l->alpha, l->gamma, l->epsilon, reinterpret_cast<int32_t*>(st.pos), st,
                     l->reward_sum, l->perf_sum, l->episodes, reinterpret_cast<long long*>(l->clamped),
                     acc_sum, acc_count, l->bad_count, l->bad_flag, B, P, (int32_t)(B / P), (int32_t)G,
                     T, l->reset_first);
  return launch_status();
}

int32_t campx_wide_traces_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                               int32_t path, int32_t team, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  TracePlan plan;
  return plan_traces(n_states, has_perf, B, wide_lds_max, path, team, &plan, plan_out);
}

int32_t campx_wide_traces_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                                 const CampxTraceLearner* l, int64_t B, int32_t T, void* stream) {
  const bool own_ok = l && l->traces && l->lam && aligned_to(l->traces, 16) && aligned_to(l->lam, 4) &&
                      (l->trace == CAMPX_TRACE_ACCUMULATING || l->trace == CAMPX_TRACE_REPLACING);
  const int32_t screened = screen_learner(s, tables_dev, st, l, B, T, own_ok);
  if (screened != CAMPX_OK) return screened;
  TracePlan plan;      // (refuses B * n_states * 5 >= 2^31, a bad team, a forced shape that does not fit)
  const int32_t planned = plan_traces(s->n_states, l->perf_sum ? 1 : 0, B, knob(K_WIDE_LDS_MAX),
                                      l->path, l->team, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const WideTables t = wide_tables(*s, tables_dev);
  const size_t lds = (size_t)plan.lds_bytes;
  const TraceKernel kernel = pick_kernel(kTraceKernels, plan, *l);
  CAMPX_ALLOW_LDS(kernel, lds);
  const int64_t G = kLearnThreads / plan.team;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + G - 1) / G)), dim3(kLearnThreads), lds,
                     static_cast<hipStream_t>(stream), learn_params(*s, *l), t.entries, t.perf, l->q,
                     l->traces, l->alpha, l->gamma, l->epsilon, l->lam,
                     reinterpret_cast<int32_t*>(st.pos), st, l->reward_sum, l->perf_sum, l->episodes,
                     l->bad_count, l->bad_flag, B, T, l->reset_first, (int32_t)plan.team, l->trace);
  return launch_status();
}

int32_t campx_wide_dyna_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                             int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  DynaPlan plan;
  return plan_dyna(n_states, has_perf, B, wide_lds_max, path, &plan, plan_out);
}

int32_t campx_wide_dyna_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                               const CampxDynaLearner* l, int64_t B, int32_t T, void* stream) {
  const bool own_ok = l && l->seen && l->n_seen && l->planning && aligned_to(l->seen, 16) &&
                      aligned_to(l->n_seen, 4) && aligned_to(l->planning, 4) && aligned_to(l->marks, 4);
  const int32_t screened = screen_learner(s, tables_dev, st, l, B, T, own_ok);
  if (screened != CAMPX_OK) return screened;
  DynaPlan plan;       // (refuses B * n_states * 5 >= 2^31, and path 1 for what does not fit)
  const int32_t planned = plan_dyna(s->n_states, l->perf_sum ? 1 : 0, B, knob(K_WIDE_LDS_MAX), l->path,
                                    &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  if (plan.path == 2 && !l->marks) return CAMPX_EINVAL;
  const WideTables t = wide_tables(*s, tables_dev);
  const size_t lds = (size_t)plan.lds_bytes;
  const DynaKernel kernel = pick_kernel(kDynaKernels, plan, *l);
  CAMPX_ALLOW_LDS(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kLearnThreads - 1) / kLearnThreads)),
                     dim3(kLearnThreads), lds, static_cast<hipStream_t>(stream), learn_params(*s, *l),
                     t.entries, t.perf, l->q, l->alpha, l->gamma, l->epsilon, l->seen, l->n_seen,
                     l->planning, l->marks, reinterpret_cast<int32_t*>(st.pos), st, l->reward_sum,
                     l->perf_sum, l->episodes, l->bad_count, l->bad_flag, B, T, l->reset_first,
                     (int32_t)plan.words);
  return launch_status();
}

int32_t campx_wide_actor_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                              int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  LearnPlan plan;
  return plan_actor(n_states, has_perf, B, wide_lds_max, path, &plan, plan_out);
}

int32_t campx_wide_actor_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                                const CampxActorLearner* l, int64_t B, int32_t T, void* stream) {
  // the one-step learners' screening, on the fields the actor-critic shares with them: prefs stands
  // where q does, the two step sizes where alpha and epsilon do; it has no rule
  CampxLearner as{};
  if (l) {
    as.q = l->prefs, as.alpha = l->alpha_actor, as.gamma = l->gamma, as.epsilon = l->alpha_critic;
    as.reward_sum = l->reward_sum, as.perf_sum = l->perf_sum, as.episodes = l->episodes;
    as.bad_count = l->bad_count, as.bad_flag = l->bad_flag, as.seed = l->seed;
    as.first_frame = l->first_frame, as.window = l->window, as.rule = CAMPX_LEARN_Q;
    as.path = l->path, as.reset_first = l->reset_first;
  }
  const bool own_ok = l && l->values && aligned_to(l->values, 16) && aligned_to(l->bad_rows, 4);
  const int32_t screened = screen_learner(s, tables_dev, st, &as, B, T, own_ok);
  if (screened != CAMPX_OK) return screened;
  LearnPlan plan;      // (refuses B * n_states * 5 >= 2^31, and path 1 for what does not fit)
  const int32_t planned = plan_actor(s->n_states, l->perf_sum ? 1 : 0, B, knob(K_WIDE_LDS_MAX), l->path,
                                     &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const WideTables t = wide_tables(*s, tables_dev);
  const size_t lds = (size_t)plan.lds_bytes;
  const ActorKernel kernel =
      kActorKernels[plan.path == 1 ? 2 : (plan.table_in_lds ? 1 : 0)][l->perf_sum != nullptr];
  CAMPX_ALLOW_LDS(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kLearnThreads - 1) / kLearnThreads)),
                     dim3(kLearnThreads), lds, static_cast<hipStream_t>(stream), learn_params(*s, as),
                     t.entries, t.perf, l->prefs, l->values, l->alpha_actor, l->alpha_critic, l->gamma,
                     reinterpret_cast<int32_t*>(st.pos), st, l->reward_sum, l->perf_sum, l->episodes,
                     l->bad_count, l->bad_rows, l->bad_flag, B, T, l->reset_first);
  return launch_status();
}

int32_t campx_wide_actor_shared_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t P,
                                     int64_t wide_lds_max, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SharedPlan plan;
  return plan_actor_shared(n_states, has_perf, B, P, wide_lds_max, path, &plan, plan_out);
}

int64_t campx_wide_actor_shared_scratch_bytes(int64_t n_states, int64_t P) {
  if (n_states < 1 || n_states > CAMPX_WIDE_MAX_STATES || P < 1 || P > 0xffffffffll ||
      P * n_states * CAMPX_N_ACTIONS >= (1ll << 31))
    return 0;
  return P * n_states * kSharedActorScratchPerState;
}

int32_t campx_wide_actor_shared_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                                       const CampxSharedActorLearner* l, int64_t B, int32_t T,
                                       void* stream) {
  // screened as campx_wide_actor_launch() screens: prefs stands where q does, the two step sizes
  // where alpha and epsilon do; there is no rule
  CampxLearner as{};
  if (l) {
    as.q = l->prefs, as.alpha = l->alpha_actor, as.gamma = l->gamma, as.epsilon = l->alpha_critic;
    as.reward_sum = l->reward_sum, as.perf_sum = l->perf_sum, as.episodes = l->episodes;
    as.bad_count = l->bad_count, as.bad_flag = l->bad_flag, as.seed = l->seed;
    as.first_frame = l->first_frame, as.window = l->window, as.rule = CAMPX_LEARN_Q;
    as.path = l->path, as.reset_first = l->reset_first;
  }
  const bool own_ok = l && l->values && aligned_to(l->values, 16) && aligned_to(l->bad_rows, 4) &&
                      l->clamped && aligned_to(l->clamped, 8) && aligned_to(l->scratch, 8) &&
                      l->n_learners >= 1 && l->scratch_bytes >= 0;
  const int32_t screened = screen_learner(s, tables_dev, st, &as, B, T, own_ok);
  if (screened != CAMPX_OK) return screened;
  const int64_t P = l->n_learners;
  SharedPlan plan;     // (refuses a P that does not divide B, n > 1024, P * n_states * 5 >= 2^31)
  const int32_t planned = plan_actor_shared(s->n_states, l->perf_sum ? 1 : 0, B, P,
                                            knob(K_WIDE_LDS_MAX), l->path, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const int64_t n_bins = P * s->n_states * CAMPX_N_ACTIONS;
  if (plan.path == 2 &&
      (!l->scratch || l->scratch_bytes < P * s->n_states * kSharedActorScratchPerState))
    return CAMPX_EINVAL;
  const WideTables t = wide_tables(*s, tables_dev);
  const size_t lds = (size_t)plan.lds_bytes;
  const SharedActorKernel kernel =
      kSharedActorKernels[plan.path == 1 ? 2 : (plan.table_in_lds ? 1 : 0)][l->perf_sum != nullptr];
  CAMPX_ALLOW_LDS(kernel, lds);
  // path 2's accumulators: [sums int64 x P x S x 5][visitors uint32 x P x S]
  long long* acc_sum = plan.path == 2 ? static_cast<long long*>(l->scratch) : nullptr;
  uint32_t* acc_visits = plan.path == 2 ? reinterpret_cast<uint32_t*>(acc_sum + n_bins) : nullptr;
  const int64_t G = plan.learners;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((P + G - 1) / G)), dim3((unsigned)plan.threads), lds,
                     static_cast<hipStream_t>(stream), learn_params(*s, as), t.entries, t.perf,
                     l->prefs, l->values, l->alpha_actor, l->alpha_critic, l->gamma,
                     reinterpret_cast<int32_t*>(st.pos), st, l->reward_sum, l->perf_sum, l->episodes,
                     reinterpret_cast<long long*>(l->clamped), acc_sum, acc_visits, l->bad_count,
                     l->bad_rows, l->bad_flag, B, P, (int32_t)(B / P), (int32_t)G, T, l->reset_first);
  return launch_status();
}

}  // extern "C"
