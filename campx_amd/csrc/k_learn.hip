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
//
// Below it, the SHARED learners: n environments feed one table (wide_learn_shared_kernel has its
// own account).

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

// ---------------------------------------------------------------------------------------------
// Shared learners: P tables, each fed by the n = B / P consecutive environments of its block
// (include/campx_hip.h, "Shared online learners", has the rule; tests/shared_learner_reference.py
// restates it in numpy).  Within a frame every environment of a learner reads the table as the
// frame found it; the TD errors are quantised to 64-bit fixed point and added per (state, action)
// as INTEGERS, and the table moves once per visited bin: no order of arrival changes a bit.
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

struct SharedPlan {
  int32_t path;                // 1 tables, q and accumulators in LDS, 2 q and accumulators global
  int32_t learners;            // G: whole learners of a workgroup
  int32_t threads;             // G * n
  int64_t lds_bytes;
  int32_t table_in_lds;
  int32_t copies;              // accumulators per bin: 1, the adds are not privatised
};

inline int32_t plan_shared(int64_t S, int32_t has_perf, int64_t B, int64_t P, int64_t lds_max,
                           int32_t path, SharedPlan* p, int64_t* plan_out) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || (has_perf & ~1) || B < 1 || B > 0xffffffffll || P < 1 ||
      P > B || B % P != 0 || B / P > kSharedMaxThreads || P * S * CAMPX_N_ACTIONS >= (1ll << 31) ||
      lds_max < 0 || path < 0 || path > 2)
    return CAMPX_EINVAL;
  const int64_t n = B / P, n_entries = S * CAMPX_N_ACTIONS;
  const int64_t table = up16(n_entries * (int64_t)sizeof(uint2)) + (has_perf ? up16(n_entries) : 0);
  const int64_t per = n_entries * kSharedBytesPerEntry;
  int64_t most = n <= kSharedPack ? kSharedPack / n : 1;       // what a workgroup would hold
  if (most > P) most = P;
  const int64_t room = lds_max >= table ? (lds_max - table) / per : 0;
  const int64_t held = room < most ? room : most;              // ... and what of it path 1 can
  if (path == 1 && held < 1) return CAMPX_EINVAL;
  // Unforced, path 1 must still fill a wave (or hold all it would anyway): a workgroup cut down to
  // a few lanes by its LDS leaves most of a wave idle at every frame.
  const bool pays = held >= 1 && (held == most || held * n >= 64);
  p->path = (path == 1 || (path == 0 && pays)) ? 1 : 2;
  p->learners = (int32_t)(p->path == 1 ? held : most);
  p->threads = (int32_t)(p->learners * n);
  p->table_in_lds = (p->path == 1 || table <= lds_max) ? 1 : 0;
  p->lds_bytes = p->path == 1 ? table + p->learners * per : (p->table_in_lds ? table : 0);
  p->copies = 1;
  if (plan_out) {
    plan_out[0] = p->path;
    plan_out[1] = p->learners;
    plan_out[2] = p->threads;
    plan_out[3] = p->lds_bytes;
    plan_out[4] = p->table_in_lds;
    plan_out[5] = p->copies;
  }
  return CAMPX_OK;
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
  const uint2* entries = g_entries;
  const int8_t* perf_tab = g_perf;
  const int n_q = n_here * n_entries;                        // floats: P * S * 5 < 2^31
  float* q_block = q + first_learner * n_entries;
  float* tables = q_block;                                   // [learner][s][a], wherever they are
  long long* sums = kQLds ? nullptr : acc_sum + first_learner * n_entries;
  uint32_t* counts = kQLds ? nullptr : acc_count + first_learner * n_entries;
  if (kTableLds) {
    uint2* l_entries = lds_tables;
    int8_t* l_perf = reinterpret_cast<int8_t*>(l_entries + n_entries + (n_entries & 1));   // 16-byte aligned
    for (int i = tid; i < n_entries; i += threads) l_entries[i] = g_entries[i];
    if (kPerf)
      for (int i = tid; i < n_entries; i += threads) l_perf[i] = g_perf[i];
    entries = l_entries;
    perf_tab = l_perf;
    if (kQLds) {
      // [sums G x entries x 8][tables G x entries x 4][counts G x entries x 4], 16-byte aligned
      sums = reinterpret_cast<long long*>(l_perf + (kPerf ? (n_entries + 15) & ~15 : 0));
      float* l_q = reinterpret_cast<float*>(sums + (int64_t)G * n_entries);
      counts = reinterpret_cast<uint32_t*>(l_q + (int64_t)G * n_entries);
      for (int i = tid; i < n_q; i += threads) {
        l_q[i] = q_block[i];
        sums[i] = 0;
        counts[i] = 0u;
      }
      tables = l_q;
    }
  }
  if (tid < 16) discounts[tid] = pp.discounts[tid];
  if (tid < kSharedPack) l_clamped[tid] = 0ull;
  __syncthreads();

  // What stays in registers for the run.  An absent lane keeps these values and does nothing
  // between the barriers below.
  float alpha = 0.0f, gamma = 0.0f, epsilon = 0.0f, keep = 0.0f;
  bool good = false;
  uint32_t now = 0, from = 0;
  int over = 0;
  float ret = 0.0f, r_sum = 0.0f;
  int32_t p_sum = 0, n_done = 0;
  int in_window = 0;
  int64_t at = env;                            // element (window, env) of the [W][B] sums
  unsigned long long n_clamped = 0ull;
  const int own = who * n_entries;             // the learner's table, sums and counts start here
  if (active) {
    alpha = alphas[m];
    gamma = gammas[m];
    epsilon = epsilons[m];
    // (x - x is 0 exactly for a finite x, NaN for an infinity or a NaN)
    good = (alpha - alpha) == 0.0f && (gamma - gamma) == 0.0f && epsilon >= 0.0f && epsilon <= 1.0f;
    keep = 1.0f - epsilon;
    if (!reset_first) {
      now = (uint32_t)state[env];
      now = now < (uint32_t)S ? now : 0u;      // (a state index from outside: start over)
      over = st.done[env];
      if (st.ret) ret = st.ret[env];
    }
    from = over ? 0u : now;
  }
  // Chunks start on a multiple of four ABSOLUTE frames, as in wide_learn_kernel.  t0, lead and T
  // are the same in every lane of the grid.
  const int lead = (int)(pp.first_frame & 3);
  const uint64_t pair0 = (uint64_t)(pp.first_frame - lead) >> 1;
  for (int t0 = -lead; t0 < T; t0 += kLearnChunk) {
    uint32_t x[2 * kLearnChunk];
    if (active) {
      const uint64_t g = pair0 + (uint64_t)((t0 + lead) >> 1);
      philox4x32_10((uint32_t)env, (uint32_t)g, (uint32_t)(g >> 32), 1u, pp.key0, pp.key1, x);
      philox4x32_10((uint32_t)env, (uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), 1u, pp.key0, pp.key1,
                    x + 4);
    }
#pragma unroll
    for (int j = 0; j < kLearnChunk; ++j) {
      if (t0 + j < 0 || t0 + j >= T) continue;               // (uniform: kernel arguments alone)
      int bin = 0;                                           // own + s * 5 + a
      bool owner = false;
      if (active) {                                          // ---- (A)
        float row[5], nrow[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) row[k] = tables[own + from * CAMPX_N_ACTIONS + k];
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
        if (good) {
          // the bootstrap row: the table as the frame found it, for every lane of the learner
#pragma unroll
          for (int k = 0; k < 5; ++k) nrow[k] = tables[own + next * CAMPX_N_ACTIONS + k];
          float b;
          uint32_t unused;
          greedy_of(nrow, b, unused);
          if (kSarsa) {
            const float mean = ((((nrow[0] + nrow[1]) + nrow[2]) + nrow[3]) + nrow[4]) * 0.2f;
            b = (keep * b) + (epsilon * mean);
          }
          const float target = done ? r : r + (gamma * D) * b;
          float old = row[0];
#pragma unroll
          for (int k = 1; k < 5; ++k) old = a == (uint32_t)k ? row[k] : old;
          const float delta = target - old;
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
        from = next;
        r_sum += r;
        if (kPerf) p_sum += perf_tab[idx];
        n_done += (int32_t)done;
        ret = (over ? 0.0f : ret) + r;
        over = (int)done;
        if (++in_window == pp.window) {
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
      __syncthreads();
      if (owner) {                                           // ---- (B)
        const long long Z = __hip_atomic_exchange(&sums[bin], 0ll, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t c = __hip_atomic_exchange(&counts[bin], 0u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        const double g = (double)Z / (double)c;
        const float mean = (float)(g * (1.0 / kSharedScale));
        const float step = alpha * mean;
        tables[bin] = tables[bin] + step;
      }
      __syncthreads();
    }
  }
  if (active) {
    if (in_window) {                           // the last window is short
      reward_sum[at] = r_sum;
      if (kPerf) perf_sum[at] = p_sum;
      episodes[at] = n_done;
    }
    state[env] = (int32_t)now;
    st.done[env] = (uint8_t)over;
    if (st.ret) st.ret[env] = ret;
    if (n_clamped)
      __hip_atomic_fetch_add(&l_clamped[who], n_clamped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tid == who * n) report_bad(bad_count, bad_flag, good ? 0 : 1);     // bad LEARNERS, once
  }
  __syncthreads();
  if (active && tid == who * n) clamped[m] = (long long)l_clamped[who];
  if (kQLds)
    for (int i = tid; i < n_q; i += threads) q_block[i] = tables[i];
}

using SharedKernel = decltype(&wide_learn_shared_kernel<false, false, false, false>);
static const SharedKernel kSharedKernels[3][2][2] = {
    {{wide_learn_shared_kernel<false, false, false, false>, wide_learn_shared_kernel<false, false, false, true>},
     {wide_learn_shared_kernel<false, false, true, false>, wide_learn_shared_kernel<false, false, true, true>}},
    {{wide_learn_shared_kernel<false, true, false, false>, wide_learn_shared_kernel<false, true, false, true>},
     {wide_learn_shared_kernel<false, true, true, false>, wide_learn_shared_kernel<false, true, true, true>}},
    {{wide_learn_shared_kernel<true, true, false, false>, wide_learn_shared_kernel<true, true, false, true>},
     {wide_learn_shared_kernel<true, true, true, false>, wide_learn_shared_kernel<true, true, true, true>}}};

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

int32_t campx_wide_shared_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t P,
                               int64_t wide_lds_max, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SharedPlan plan;
  return plan_shared(n_states, has_perf, B, P, wide_lds_max, path, &plan, plan_out);
}

int64_t campx_wide_shared_scratch_bytes(int64_t n_states, int64_t P) {
  if (n_states < 1 || n_states > CAMPX_WIDE_MAX_STATES || P < 1 ||
      P * n_states * CAMPX_N_ACTIONS >= (1ll << 31))
    return 0;
  return P * n_states * CAMPX_N_ACTIONS * 12;
}

int32_t campx_wide_shared_launch(const CampxWideSpec* s, const void* tables_dev, CampxState st,
                                 const CampxSharedLearner* l, int64_t B, int32_t T, void* stream) {
  if (!s || !tables_dev || !st.pos || !st.done || !l || B <= 0 || T <= 0) return CAMPX_EINVAL;
  if (!l->q || !l->alpha || !l->gamma || !l->epsilon || !l->reward_sum || !l->episodes || !l->clamped)
    return CAMPX_EINVAL;
  if (!aligned_to(l->q, 16) || !aligned_to(st.pos, 4) || !aligned_to(st.ret, 4) ||
      !aligned_to(l->alpha, 4) || !aligned_to(l->gamma, 4) || !aligned_to(l->epsilon, 4) ||
      !aligned_to(l->reward_sum, 4) || !aligned_to(l->perf_sum, 4) || !aligned_to(l->episodes, 4) ||
      !aligned_to(l->clamped, 8) || !aligned_to(l->scratch, 8) || !aligned_to(l->bad_count, 4) ||
      !aligned_to(l->bad_flag, 4))
    return CAMPX_EINVAL;
  if (B > 0xffffffffll || l->first_frame < 0 || l->first_frame > INT64_MAX - T) return CAMPX_EINVAL;
  if (l->window < 1 || (l->rule != CAMPX_LEARN_Q && l->rule != CAMPX_LEARN_EXPECTED_SARSA) ||
      l->path < 0 || l->path > 2 || l->n_learners < 1 || l->scratch_bytes < 0)
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  if (l->perf_sum && !s->has_perf) return CAMPX_EINVAL;
  const int64_t P = l->n_learners;
  SharedPlan plan;     // (refuses a P that does not divide B, n > 1024, P * n_states * 5 >= 2^31)
  const int32_t planned = plan_shared(s->n_states, l->perf_sum ? 1 : 0, B, P, knob(K_WIDE_LDS_MAX),
                                      l->path, &plan, nullptr);
  if (planned != CAMPX_OK) return planned;
  const int64_t n_bins = P * s->n_states * CAMPX_N_ACTIONS;
  if (plan.path == 2 && (!l->scratch || l->scratch_bytes < n_bins * 12)) return CAMPX_EINVAL;
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
  const SharedKernel kernel = kSharedKernels[plan.path == 1 ? 2 : (plan.table_in_lds ? 1 : 0)]
                                            [l->perf_sum != nullptr][l->rule == CAMPX_LEARN_EXPECTED_SARSA];
  CAMPX_ALLOW_LDS(kernel, lds);
  // path 2's accumulators: [sums int64 x bins][counts uint32 x bins]
  long long* acc_sum = plan.path == 2 ? static_cast<long long*>(l->scratch) : nullptr;
  uint32_t* acc_count = plan.path == 2 ? reinterpret_cast<uint32_t*>(acc_sum + n_bins) : nullptr;
  const int64_t G = plan.learners;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((P + G - 1) / G)), dim3((unsigned)plan.threads), lds,
                     static_cast<hipStream_t>(stream), pp, t.entries, t.perf, l->q, l->alpha, l->gamma,
                     l->epsilon, reinterpret_cast<int32_t*>(st.pos), st, l->reward_sum, l->perf_sum,
                     l->episodes, reinterpret_cast<long long*>(l->clamped), acc_sum, acc_count,
                     l->bad_count, l->bad_flag, B, P, (int32_t)(B / P), (int32_t)G, T, l->reset_first);
  return launch_status();
}

}  // extern "C"
