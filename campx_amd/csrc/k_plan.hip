// k_plan.hip - exact policy evaluation and value iteration on a game's state table: Jacobi sweeps
// of the Bellman backup over the blob that wide_policy_update_kernel walks, which is the game's
// complete deterministic MDP, (state, action) -> next state, reward, done, discount code.
//
// The rule (include/campx_hip.h has it in full; tests/planning_reference.py restates it in numpy
// float32): for entry (s, a) with next state n, reward r (NaN counts as 0), done d and the frame's
// discount D as a rollout reports it,
//     c = gamma * D        q[s, a] = d ? r : r + c * v[n]
//     policy   v'[s] = (((((w0*q0) + w1*q1) + w2*q2) + w3*q3) + w4*q4) / c4     (a bad row: q4)
//     greedy   v'[s] = max_a q[s, a], the lowest a attaining it
// every operation an f32 operation rounded on its own, the division IEEE-rounded.  A sweep reads
// v_{k-1} only and writes v_k only (Jacobi), so its result does not depend on which lane takes
// which state, and residual[k-1] - the largest bit pattern of |v_k[s] - v_{k-1}[s]| - is a maximum
// of integers: both paths below give the same bits.
//
// A population: member m of P is the policy reduction above with policies[m] and gamma[m], and
// nothing else.  Members share the table and nothing they write, so the only questions are where a
// member's vectors live and which lane takes which (member, state) pair - and by the rule neither
// can change a bit.  The kernels are compiled with the members (kMembers) and without: one member,
// gamma from the params, no division by S, no slot per member.
//
// A population of rewards (campx_wide_population_solve_launch()): member m may also have a reward
// table of its own, rewards[m] in place of the table's rewards or of the one override, and the
// greedy reduction has members too - value iteration under P rewards or P gammas, `greedy_out`
// [P][S].  These are further instances of the same two kernels: kRewards is compiled into them
// alone, so that the instances behind the two older launches keep their loads and branches.
//
// wide_sweeps_lds_kernel   a workgroup holds the entries (reward already resolved: NaN -> 0, the
//     override taken) and the vectors of G consecutive members in LDS and runs ALL n sweeps of the
//     call, one __syncthreads() per sweep.  Everything per (state, action) is laid out
//     [action][state], so that the lanes of a wave read consecutive addresses.  A member's vectors
//     are FLAT over the pairs i = g * S + s: two value vectors [G * S] and, for a policy, the
//     weights [5][G * S] and their totals [G * S] - pair i is lane i's in every one of them,
//     whether a wave sits inside a member, across two, or holds several.  With members, G residual
//     slots per sweep parity and the members' gammas lie behind the entries; without, the two
//     residual slots are in the header and the one workgroup is the whole launch.  With kRewards
//     the members' rewards are staged [5][G * S] floats, flat over the pairs like the weights and
//     NaN already resolved; the staged entries keep the shared next / done / discount-code word
//     and their reward word goes unused.  That is 20 bytes per (member, state) on top of a greedy
//     member's 8 and a policy member's 32.
// wide_sweep_kernel        one launch per sweep, a lane per pair, a workgroup per 256 states of
//     ONE member (the blocks of all members flattened into grid.x): five 8-byte entries (40
//     contiguous bytes), five gathers from v, between two value buffers; the residual goes through
//     the workgroup and then one atomicMax per workgroup.  The n launches follow each other on the
//     stream: a sweep boundary is a kernel boundary, there is no barrier across workgroups.
// Either grid stops at kPlanMaxGrid workgroups; a workgroup takes the groups (or blocks) that are
// a whole grid apart, one after the other.
// plan_sweeps() chooses; campx_wide_sweeps_plan(), campx_wide_population_sweeps_plan() and
// campx_wide_population_solve_plan() show the choice to a test without a GPU.  The members to a
// workgroup of the new forms are members_per_workgroup()'s rule TAKEN OVER as it stands (pack =
// 256, ceil(P / CUs), the new LDS bytes in rule (a)): it was measured on the policy form with shared
// rewards and is not tuned for a greedy member or for staged rewards.

#include "wide_table.hip.h"

namespace campx_impl {

constexpr int kPlanThreads = 256;          // global path
constexpr int64_t kPlanLdsHeader = 128;    // discount list, the two residual slots of one member
constexpr int32_t kPlanMaxSweeps = 1 << 20;
constexpr int64_t kPlanMaxGrid = 1 << 20;
constexpr int64_t kPlanMaxElements = 0x7fffffff;     // P * S * 5, the elements of `policies`
constexpr int64_t kPlanPackThreads = 256;

struct SweepsPlan {
  int32_t path, threads, G;
  int64_t grid, lds_bytes, groups;           // groups: of G members (path 1) / blocks of 256 states (path 2)
  int32_t off_red, off_gamma, off_v0, off_v1, off_w, off_c4, off_r;   // byte offsets into the dynamic LDS
};

// The LDS G members of S states take, and where its parts start: header, entries [5][S] x 8 bytes,
// with `slots` two residual slots and a gamma per member, two value vectors, and for a policy the
// weights and the totals.  An override costs nothing: the staged entry holds the reward the sweeps
// use, wherever it came from.  `rewards`: a reward table per member, [5][G * S] floats at the end.
inline int64_t sweeps_lds(int64_t S, int64_t G, bool policy, bool slots, bool rewards, SweepsPlan* p) {
  int64_t at = kPlanLdsHeader + up16(S * CAMPX_N_ACTIONS * (int64_t)sizeof(uint2));
  int64_t part[7] = {0, 0, 0, 0, 0, 0, 0};   // red, gamma, v0, v1, w, c4, r
  if (slots) {
    part[0] = at;
    at += up16(2 * G * 4);
    part[1] = at;
    at += up16(G * 4);
  }
  part[2] = at;
  at += up16(G * S * 4);
  part[3] = at;
  at += up16(G * S * 4);
  if (policy) {
    part[4] = at;
    at += up16(G * S * CAMPX_N_ACTIONS * 4);
    part[5] = at;
    at += up16(G * S * 4);
  }
  if (rewards) {
    part[6] = at;
    at += up16(G * S * CAMPX_N_ACTIONS * 4);
  }
  if (p && at <= 0x7fffffff) {
    p->off_red = (int32_t)part[0];
    p->off_gamma = (int32_t)part[1];
    p->off_v0 = (int32_t)part[2];
    p->off_v1 = (int32_t)part[3];
    p->off_w = (int32_t)part[4];
    p->off_c4 = (int32_t)part[5];
    p->off_r = (int32_t)part[6];
  }
  return at;
}

// The plan of P members; `slots`: the LDS layout of a population (a single policy or value
// iteration is P = 1 on one compute unit without them).  Path 1 whenever one member fits; how
// many members a workgroup of it takes is members_per_workgroup()'s rule (wide_table.hip.h, with
// the measurement behind it, which was made on these kernels' policy instances with shared
// rewards; `rewards` - a reward table per member - and a greedy population take it over untuned).
inline int32_t plan_sweeps(int64_t S, int64_t P, int32_t policy, bool slots, int32_t has_override,
                           int32_t rewards, int64_t lds_max, int64_t n_cus, int32_t path,
                           SweepsPlan* p) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || P < 1 || (policy & ~1) || (has_override & ~1) ||
      (rewards & ~1) || n_cus < 1 || lds_max < 0 || path < 0 || path > 2)
    return CAMPX_EINVAL;
  if (P > kPlanMaxElements / (S * CAMPX_N_ACTIONS)) return CAMPX_EINVAL;
  memset(p, 0, sizeof(*p));
  const bool fits = sweeps_lds(S, 1, policy, slots, rewards, nullptr) <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  if (path == 1 || (path == 0 && fits)) {
    const int64_t G = members_per_workgroup(S, P, n_cus, lds_max, kPlanPackThreads, [&](int64_t g) {
      return sweeps_lds(S, g, policy, slots, rewards, nullptr);
    });
    p->path = 1;
    p->G = (int32_t)G;
    p->lds_bytes = sweeps_lds(S, G, policy, slots, rewards, p);
    const int64_t t = (G * S + 63) / 64 * 64;
    p->threads = (int32_t)(t > kTableLdsThreads ? kTableLdsThreads : t);
    p->groups = (P + G - 1) / G;
  } else {
    p->path = 2;
    p->G = 1;                                  // a workgroup serves one member
    p->threads = kPlanThreads;
    p->groups = (S + kPlanThreads - 1) / kPlanThreads * P;
  }
  p->grid = p->groups > kPlanMaxGrid ? kPlanMaxGrid : p->groups;
  return CAMPX_OK;
}

// The words both _plan() entry points show: path, LDS bytes, threads, grid.
inline void plan_words(const SweepsPlan& p, int64_t* plan_out) {
  plan_out[0] = p.path;
  plan_out[1] = p.lds_bytes;
  plan_out[2] = p.threads;
  plan_out[3] = p.grid;
}

struct SweepParams {
  int32_t S, n_sweeps, G;
  float gamma;                               // of every member, where there is no gamma per member
  int64_t P, groups;
  float discounts[16];
  int32_t off_red, off_gamma, off_v0, off_v1, off_w, off_c4, off_r;
};

// q of one entry - its second word - and the reward to use beside it, given v[next].
__device__ __forceinline__ float backup(float r, uint32_t word, float gamma, const float* discounts,
                                        float vn) {
  const uint32_t done = entry_done(word), dcode = entry_dcode(word);
  const float c = gamma * __uint_as_float(discount_bits(discounts, dcode, done));
  return done ? r : r + c * vn;
}

// v' of a state from its five q; `arg` is the greedy action (4 for a bad policy row).
template <bool kPolicy>
__device__ __forceinline__ float reduce_q(const float (&q)[5], const float (&w)[5], float c4, int& arg) {
  if (kPolicy) {
    float num = w[0] * q[0];
    num = num + w[1] * q[1];
    num = num + w[2] * q[2];
    num = num + w[3] * q[3];
    num = num + w[4] * q[4];
    arg = 4;
    return c4 == 0.0f ? q[4] : __fdiv_rn(num, c4);
  }
  float best = q[0];
  arg = 0;
#pragma unroll
  for (int a = 1; a < 5; ++a) {
    if (q[a] > best) {
      best = q[a];
      arg = a;
    }
  }
  return best;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t m) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)m, o);
    m = other > m ? other : m;
  }
  return m;
}

// `residual` is [n_sweeps][P].  The grid never exceeds sp.groups, so a workgroup's first group is
// its own index; without members there is one group, the launch's one workgroup's.  `g_reward` is
// the one override [S][5] or NULL - with kRewards the members' rewards [P][S][5], never NULL;
// `greedy_out` is [P][S].
template <bool kPolicy, bool kMembers, bool kRewards>
__global__ __launch_bounds__(kTableLdsThreads) void wide_sweeps_lds_kernel(
    SweepParams sp, const uint2* __restrict__ g_entries, const float* __restrict__ g_policy,
    const float* __restrict__ g_reward, const float* __restrict__ g_gammas, const float* v_in,
    float* v_out, float* __restrict__ q_out, int8_t* __restrict__ greedy_out,
    uint32_t* __restrict__ residual, int32_t* __restrict__ bad_rows, int32_t* __restrict__ bad_flag) {
  // (the two older launches take <policy, solo>, <policy, members> and <greedy, solo> without
  // kRewards; a greedy population and every kRewards instance are campx_wide_population_solve's)
  static_assert(kMembers || !kRewards, "rewards per member come with the members' layout");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_plan[];
  float* discounts = reinterpret_cast<float*>(lds_plan);                 // [16]
  uint2* ent = reinterpret_cast<uint2*>(lds_plan + kPlanLdsHeader);      // [5][S]
  uint32_t* red =                                                        // [2][G]: sweep k uses k & 1
      reinterpret_cast<uint32_t*>(lds_plan + (kMembers ? sp.off_red : 64));
  float* gam = reinterpret_cast<float*>(lds_plan + sp.off_gamma);        // [G] (kMembers)
  float* v0 = reinterpret_cast<float*>(lds_plan + sp.off_v0);            // [G * S]
  float* v1 = reinterpret_cast<float*>(lds_plan + sp.off_v1);
  float* wts = reinterpret_cast<float*>(lds_plan + sp.off_w);            // [5][G * S]
  float* tot = reinterpret_cast<float*>(lds_plan + sp.off_c4);           // [G * S]
  float* rew = reinterpret_cast<float*>(lds_plan + sp.off_r);            // [5][G * S] (kRewards)
  const int S = sp.S, G = kMembers ? sp.G : 1, GS = G * S, nt = (int)blockDim.x, tid = (int)threadIdx.x;
  const int64_t P = kMembers ? sp.P : 1;
  for (int i = tid; i < S * CAMPX_N_ACTIONS; i += nt) {
    const uint2 e = g_entries[i];
    const float r = real_reward(!kRewards && g_reward ? g_reward[i] : __uint_as_float(e.x));
    const int s = i / CAMPX_N_ACTIONS, a = i - s * CAMPX_N_ACTIONS;
    ent[a * S + s] = make_uint2(__float_as_uint(r), e.y);
  }
  if (tid < 16) discounts[tid] = sp.discounts[tid];

  int bad = 0;
  int64_t group = kMembers ? blockIdx.x : 0;
  do {
    const int64_t m0 = group * G;                                        // the group's first member
    const int members = (int)(P - m0 < G ? P - m0 : G);                  // (the last group may be short)
    const int n = members * S;                                           // its pairs
    const int64_t row0 = m0 * S;                                         // pair 0 among all P * S
    float *vi = v0, *vo = v1;
    for (int i = tid; i < n; i += nt) {
      vi[i] = v_in[row0 + i];
      if (kPolicy) {
        float w[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) w[a] = g_policy[(row0 + i) * CAMPX_N_ACTIONS + a];
#pragma unroll
        for (int a = 0; a < 5; ++a) wts[a * GS + i] = w[a];
        tot[i] = policy_row_total(w);
      }
      if (kRewards) {
        float r[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) r[a] = g_reward[(row0 + i) * CAMPX_N_ACTIONS + a];
#pragma unroll
        for (int a = 0; a < 5; ++a) rew[a * GS + i] = real_reward(r[a]);
      }
    }
    for (int g = tid; g < members; g += nt) {
      if (kMembers) gam[g] = g_gammas ? g_gammas[m0 + g] : sp.gamma;
      red[g] = 0;
      red[G + g] = 0;
    }
    __syncthreads();

    for (int k = 0; k < sp.n_sweeps; ++k) {
      const bool last = k == sp.n_sweeps - 1;
      uint32_t* redk = red + (k & 1) * G;
      // pair i, state s of the member whose v_{k-1} is vg: v_k, the outputs of the last sweep, and
      // the bits of |v_k - v_{k-1}|
      const auto pair = [&](int i, int s, const float* vg, float gamma) {
        float q[5], vn[5], r[5], w[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, c4 = 0.0f;
        uint2 e[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) e[a] = ent[a * S + s];
#pragma unroll
        for (int a = 0; a < 5; ++a) vn[a] = vg[entry_target(e[a].y, (uint32_t)S)];   // five in flight
#pragma unroll
        for (int a = 0; a < 5; ++a) r[a] = kRewards ? rew[a * GS + i] : __uint_as_float(e[a].x);
#pragma unroll
        for (int a = 0; a < 5; ++a) q[a] = backup(r[a], e[a].y, gamma, discounts, vn[a]);
        if (kPolicy) {
#pragma unroll
          for (int a = 0; a < 5; ++a) w[a] = wts[a * GS + i];
          c4 = tot[i];
        }
        int arg;
        const float v = reduce_q<kPolicy>(q, w, c4, arg);
        vo[i] = v;
        const uint32_t diff = __float_as_uint(fabsf(v - vi[i]));
        if (last) {
          if (q_out) {
#pragma unroll
            for (int a = 0; a < 5; ++a) q_out[(row0 + i) * CAMPX_N_ACTIONS + a] = q[a];
          }
          if ((!kMembers || !kPolicy) && greedy_out) greedy_out[row0 + i] = (int8_t)arg;
          bad += kPolicy && c4 == 0.0f;
        }
        return diff;
      };
      if (kMembers) {
        for (int base = 0; base < n; base += nt) {          // every thread of the workgroup goes round
          const int i = base + tid;
          const bool live = i < n;
          int g = -1;
          uint32_t m = 0;
          if (live) {
            g = G == 1 ? 0 : i / S;
            m = pair(i, i - g * S, vi + g * S, gam[g]);
          }
          // a wave inside one member reduces first; one that straddles members goes lane by lane
          // (lane 0 holds the wave's lowest pair: where it is idle, so is the wave, and m is 0)
          const int g0 = __shfl(g, 0);
          if (__all(!live || g == g0)) {
            m = wave_max(m);
            if ((tid & 63) == 0 && m) atomicMax(&redk[g0], m);
          } else if (m) {
            atomicMax(&redk[g], m);
          }
        }
      } else {
        uint32_t m = 0;
        for (int s = tid; s < S; s += nt) {
          const uint32_t diff = pair(s, s, vi, sp.gamma);
          m = diff > m ? diff : m;
        }
        m = wave_max(m);
        if ((tid & 63) == 0 && m) atomicMax(redk, m);
      }
      __syncthreads();             // v_k and its residuals are complete; v_{k-1} is free
      for (int g = tid; g < members; g += nt) {
        residual[(int64_t)k * P + m0 + g] = redk[g];
        redk[g] = 0;               // (used again by sweep k + 2, past the next barrier)
      }
      float* t = vi;
      vi = vo;
      vo = t;
    }
    for (int i = tid; i < n; i += nt) v_out[row0 + i] = vi[i];
    if (kMembers) __syncthreads();   // the next group of this workgroup stages over these vectors
  } while (kMembers && (group += gridDim.x) < sp.groups);
  report_bad(bad_rows, bad_flag, bad);
}

// What the global path starts with: the `n` residual slots to zero (the sweeps raise them with
// atomicMax) and - v_in == v_out with an odd number of sweeps - a copy of the `n_values` values to
// start from.
__global__ __launch_bounds__(kPlanThreads) void sweeps_prepare_kernel(
    uint32_t* __restrict__ residual, int64_t n, const float* __restrict__ src,
    float* __restrict__ dst, int64_t n_values) {
  const int64_t first = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kPlanThreads;
  for (int64_t i = first; i < n; i += step) residual[i] = 0;
  if (dst)
    for (int64_t i = first; i < n_values; i += step) dst[i] = src[i];
}

// `residual` is the row of the sweep: [P].  The grid never exceeds sp.groups; without members it
// is the blocks of the one member, each its workgroup's only one.  `reward`, `greedy_out`: as above.
template <bool kPolicy, bool kMembers, bool kRewards>
__global__ __launch_bounds__(kPlanThreads) void wide_sweep_kernel(
    SweepParams sp, const uint2* __restrict__ entries, const float* __restrict__ policy,
    const float* __restrict__ reward, const float* __restrict__ gammas,
    const float* __restrict__ v_src, float* __restrict__ v_dst, float* __restrict__ q_out,
    int8_t* __restrict__ greedy_out, uint32_t* __restrict__ residual, int32_t* __restrict__ bad_rows,
    int32_t* __restrict__ bad_flag, int32_t last) {
  static_assert(kMembers || !kRewards, "rewards per member come with the members");
  __shared__ float discounts[16];
  __shared__ uint32_t partial[kPlanThreads / 64];
  const int tid = (int)threadIdx.x, S = sp.S;
  if (tid < 16) discounts[tid] = sp.discounts[tid];
  __syncthreads();
  const int64_t per_member = (S + kPlanThreads - 1) / kPlanThreads;     // blocks of a member
  int bad = 0;
  int64_t block = blockIdx.x;
  do {
    const int64_t member = kMembers ? block / per_member : 0;
    const int s = (int)(block - member * per_member) * kPlanThreads + tid;
    const bool live = s < S;
    const int row = (live ? s : S - 1) * CAMPX_N_ACTIONS;                // any valid row
    const int64_t first = member * S;                                    // the member's pair 0
    const int64_t mine = first * CAMPX_N_ACTIONS + row;
    const float* vm = v_src + first;
    const float gamma = kMembers && gammas ? gammas[member] : sp.gamma;
    uint2 e[5];
    float w[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, c4 = 0.0f;
#pragma unroll
    for (int a = 0; a < 5; ++a) e[a] = entries[row + a];
    if (kRewards) {
#pragma unroll
      for (int a = 0; a < 5; ++a) e[a].x = __float_as_uint(reward[mine + a]);
    } else if (reward) {
#pragma unroll
      for (int a = 0; a < 5; ++a) e[a].x = __float_as_uint(reward[row + a]);
    }
    if (kPolicy) {
#pragma unroll
      for (int a = 0; a < 5; ++a) w[a] = policy[mine + a];
      c4 = policy_row_total(w);
    }
    const float before = vm[live ? s : S - 1];
    float q[5], vn[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) vn[a] = vm[entry_target(e[a].y, (uint32_t)S)];   // five in flight
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      q[a] = backup(real_reward(__uint_as_float(e[a].x)), e[a].y, gamma, discounts, vn[a]);
    }
    int arg;
    const float v = reduce_q<kPolicy>(q, w, c4, arg);
    uint32_t m = 0;
    if (live) {
      v_dst[first + s] = v;
      m = __float_as_uint(fabsf(v - before));
      if (last) {
        if (q_out) {
#pragma unroll
          for (int a = 0; a < 5; ++a) q_out[mine + a] = q[a];
        }
        if ((!kMembers || !kPolicy) && greedy_out) greedy_out[first + s] = (int8_t)arg;
        bad += kPolicy && c4 == 0.0f;
      }
    }
    m = wave_max(m);
    if ((tid & 63) == 0) partial[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int i = 1; i < kPlanThreads / 64; ++i) m = partial[i] > m ? partial[i] : m;
      if (m) atomicMax(residual + member, m);
    }
    if (kMembers) __syncthreads();   // `partial` is written again by the next block
  } while (kMembers && (block += gridDim.x) < sp.groups);
  report_bad(bad_rows, bad_flag, bad);
}

// Every entry point, their own NULL checks behind them: `members` policies (`policy` NULL: value
// iteration - one member, or with `slots` a population of them), `gammas` one factor per member or
// NULL for `gamma`; `slots`: the plan is a population's; `rewards`: a reward table per member
// (with `slots` only, never beside `reward_override`).  One member without a gamma of its own takes the instances compiled without
// members from either entry point; one member WITH a `gammas` takes the members instance (the
// other choice, a solo instance that reads gamma through the pointer, would put a load and a
// branch into evaluate_policy()'s kernels for a case that a population of one rarely is).  A greedy
// population and rewards per member have members instances only, for the same reason.
static int32_t sweeps_launch(const CampxWideSpec* s, const void* tables_dev, const float* policy,
                             int64_t members, bool slots, const float* reward_override,
                             const float* rewards, float gamma,
                             const float* gammas, const float* v_in, float* v_out, float* scratch,
                             float* q, int8_t* greedy, float* residual, int32_t* bad_rows,
                             int32_t* bad_flag, int32_t n_sweeps, int32_t path, void* stream) {
  if (members < 1 || n_sweeps < 1 || n_sweeps > kPlanMaxSweeps) return CAMPX_EINVAL;
  if (!gammas && !(fabsf(gamma) < INFINITY)) return CAMPX_EINVAL;
  if (rewards && (reward_override || !slots)) return CAMPX_EINVAL;
  if (!aligned_to(tables_dev, 8) || !aligned_to(policy, 4) || !aligned_to(reward_override, 4) ||
      !aligned_to(rewards, 4) || !aligned_to(gammas, 4) || !aligned_to(v_in, 4) || !aligned_to(v_out, 4) ||
      !aligned_to(scratch, 4) || !aligned_to(q, 4) || !aligned_to(residual, 4) ||
      !aligned_to(bad_rows, 4))
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  const int64_t S = s->n_states, P = members;
  if (P > kPlanMaxElements / (S * CAMPX_N_ACTIONS)) return CAMPX_EINVAL;
  const int64_t bytes = P * S * (int64_t)sizeof(float);
  // the values to start from and the values to leave are one array or two apart
  if (v_in != v_out && ranges_overlap(v_in, v_out, bytes)) return CAMPX_EINVAL;
  // the path is host arithmetic alone; rule (c) is not, and only a path 1 of several members has it
  const int64_t lds_max = knob(K_WIDE_LDS_MAX);
  const int32_t has_policy = policy ? 1 : 0, has_override = reward_override ? 1 : 0;
  const int32_t has_rewards = rewards ? 1 : 0;
  SweepsPlan plan;
  int32_t e = plan_sweeps(S, P, has_policy, slots, has_override, has_rewards, lds_max, 1, path, &plan);
  if (e != CAMPX_OK) return e;
  // Path 2: sweep k of n writes v_out when n - k is even and the scratch array when it is odd, so
  // that the last one writes v_out; sweep 1 reads v_in - or, where it would write the array it
  // reads (v_in == v_out, n odd), the copy of it that the first kernel leaves in the scratch array.
  if (plan.path == 2 &&
      (!scratch || ranges_overlap(scratch, v_in, bytes) || ranges_overlap(scratch, v_out, bytes)))
    return CAMPX_EINVAL;
  // (every refusal of an argument is decided above, before the device is asked anything)
  if (plan.path == 1 && P > 1) {
    e = plan_sweeps(S, P, has_policy, slots, has_override, has_rewards, lds_max, device_cus(), path,
                    &plan);
    if (e != CAMPX_OK) return e;
  }
  SweepParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.S = (int32_t)S;
  sp.n_sweeps = n_sweeps;
  sp.G = plan.G;
  sp.gamma = gamma;
  sp.P = P;
  sp.groups = plan.groups;
  wide_discounts(*s, sp.discounts);
  sp.off_red = plan.off_red;
  sp.off_gamma = plan.off_gamma;
  sp.off_v0 = plan.off_v0;
  sp.off_v1 = plan.off_v1;
  sp.off_w = plan.off_w;
  sp.off_c4 = plan.off_c4;
  sp.off_r = plan.off_r;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint2* entries = wide_tables(*s, tables_dev).entries;
  uint32_t* res = reinterpret_cast<uint32_t*>(residual);
  const bool solo = !slots || (policy && P == 1 && !gammas && !rewards);
  const float* reward = rewards ? rewards : reward_override;     // [P][S][5] / [S][5] or NULL
  if (plan.path == 1) {
    const auto kernel = rewards  ? (policy ? wide_sweeps_lds_kernel<true, true, true>
                                           : wide_sweeps_lds_kernel<false, true, true>)
                        : !policy ? (solo ? wide_sweeps_lds_kernel<false, false, false>
                                          : wide_sweeps_lds_kernel<false, true, false>)
                        : solo    ? wide_sweeps_lds_kernel<true, false, false>
                                  : wide_sweeps_lds_kernel<true, true, false>;
    CAMPX_ALLOW_LDS(kernel, (size_t)plan.lds_bytes);
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.grid), dim3((unsigned)plan.threads),
                       (size_t)plan.lds_bytes, hs, sp, entries, policy, reward, gammas, v_in,
                       v_out, q, greedy, res, bad_rows, bad_flag);
    return launch_status();
  }
  const bool copy = v_in == v_out && (n_sweeps & 1);
  {
    const int64_t slots_to_zero = (int64_t)n_sweeps * P, values = P * S;
    const int64_t most = (copy && values > slots_to_zero) ? values : slots_to_zero;
    const int64_t blocks = (most + 4 * kPlanThreads - 1) / (4 * kPlanThreads);
    hipLaunchKernelGGL(sweeps_prepare_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)),
                       dim3(kPlanThreads), 0, hs, res, slots_to_zero, v_in, copy ? scratch : nullptr,
                       values);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
  }
  const float* src = copy ? scratch : v_in;
  const auto sweep = rewards  ? (policy ? wide_sweep_kernel<true, true, true>
                                        : wide_sweep_kernel<false, true, true>)
                     : !policy ? (solo ? wide_sweep_kernel<false, false, false>
                                       : wide_sweep_kernel<false, true, false>)
                     : solo    ? wide_sweep_kernel<true, false, false>
                               : wide_sweep_kernel<true, true, false>;
  for (int32_t k = 1; k <= n_sweeps; ++k) {
    float* dst = ((n_sweeps - k) & 1) ? scratch : v_out;
    const int32_t last = k == n_sweeps;
    hipLaunchKernelGGL(sweep, dim3((unsigned)plan.grid), dim3(kPlanThreads), 0, hs, sp, entries, policy,
                       reward, gammas, src, dst, q, greedy, res + (int64_t)(k - 1) * P, bad_rows,
                       bad_flag, last);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
    src = dst;
  }
  return CAMPX_OK;
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_sweeps_plan(int64_t n_states, int32_t policy, int32_t has_override,
                               int64_t wide_lds_max, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SweepsPlan p;
  const int32_t e = plan_sweeps(n_states, 1, policy, false, has_override, 0, wide_lds_max, 1, path, &p);
  if (e == CAMPX_OK) plan_words(p, plan_out);
  return e;
}

int32_t campx_wide_sweeps_launch(const CampxWideSpec* s, const void* tables_dev, const float* policy,
                                 const float* reward_override, float gamma, const float* v_in,
                                 float* v_out, float* scratch, float* q, int8_t* greedy,
                                 float* residual, int32_t* bad_rows, int32_t* bad_flag,
                                 int32_t n_sweeps, int32_t path, void* stream) {
  if (!s || !tables_dev || !v_in || !v_out || !residual) return CAMPX_EINVAL;
  return sweeps_launch(s, tables_dev, policy, 1, false, reward_override, nullptr, gamma, nullptr, v_in,
                       v_out, scratch, q, greedy, residual, bad_rows, bad_flag, n_sweeps, path, stream);
}

int32_t campx_wide_population_sweeps_plan(int64_t n_states, int64_t members, int32_t has_override,
                                          int64_t wide_lds_max, int64_t n_cus, int32_t path,
                                          int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SweepsPlan p;
  const int32_t e =
      plan_sweeps(n_states, members, 1, true, has_override, 0, wide_lds_max, n_cus, path, &p);
  if (e == CAMPX_OK) {
    plan_words(p, plan_out);
    plan_out[4] = p.G;
  }
  return e;
}

int32_t campx_wide_population_sweeps_launch(const CampxWideSpec* s, const void* tables_dev,
                                            const float* policies, int64_t members,
                                            const float* reward_override, float gamma,
                                            const float* gammas, const float* v_in, float* v_out,
                                            float* scratch, float* q, float* residual,
                                            int32_t* bad_rows, int32_t* bad_flag, int32_t n_sweeps,
                                            int32_t path, void* stream) {
  if (!s || !tables_dev || !policies || !v_in || !v_out || !residual) return CAMPX_EINVAL;
  return sweeps_launch(s, tables_dev, policies, members, true, reward_override, nullptr, gamma, gammas,
                       v_in, v_out, scratch, q, nullptr, residual, bad_rows, bad_flag, n_sweeps, path,
                       stream);
}

int32_t campx_wide_population_solve_plan(int64_t n_states, int64_t members, int32_t policy,
                                         int32_t per_member_rewards, int64_t wide_lds_max,
                                         int64_t n_cus, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SweepsPlan p;
  const int32_t e = plan_sweeps(n_states, members, policy, true, 0, per_member_rewards, wide_lds_max,
                                n_cus, path, &p);
  if (e == CAMPX_OK) {
    plan_words(p, plan_out);
    plan_out[4] = p.G;
  }
  return e;
}

int32_t campx_wide_population_solve_launch(const CampxWideSpec* s, const void* tables_dev,
                                           const float* policies, const float* rewards,
                                           int64_t members, const float* reward_override, float gamma,
                                           const float* gammas, const float* v_in, float* v_out,
                                           float* scratch, float* q, int8_t* greedy, float* residual,
                                           int32_t* bad_rows, int32_t* bad_flag, int32_t n_sweeps,
                                           int32_t path, void* stream) {
  if (!s || !tables_dev || !v_in || !v_out || !residual) return CAMPX_EINVAL;
  if (policies && greedy) return CAMPX_EINVAL;       // the greedy actions are the greedy form's
  return sweeps_launch(s, tables_dev, policies, members, true, reward_override, rewards, gamma, gammas,
                       v_in, v_out, scratch, q, greedy, residual, bad_rows, bad_flag, n_sweeps, path,
                       stream);
}

}  // extern "C"
