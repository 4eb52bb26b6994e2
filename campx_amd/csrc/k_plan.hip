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
// wide_sweeps_lds_kernel   one workgroup holds the entries (reward already resolved: NaN -> 0, the
//     override taken), two value vectors and, for a policy, the weights and their totals in LDS and
//     runs ALL n sweeps of the call, one __syncthreads() per sweep.  Everything per (state, action)
//     is laid out [action][state], so that the lanes of a wave read consecutive addresses.
// wide_sweep_kernel        one launch per sweep, a lane per state: five 8-byte entries (40
//     contiguous bytes), five gathers from v, between two value buffers; the residual goes through
//     the workgroup and then one atomicMax per workgroup.  The n launches follow each other on the
//     stream: a sweep boundary is a kernel boundary, there is no barrier across workgroups.
// plan_sweeps() chooses; campx_wide_sweeps_plan() shows the choice to a test without a GPU.

#include "wide_table.hip.h"

namespace campx_impl {

constexpr int kPlanThreads = 256;          // global path
constexpr int64_t kPlanLdsHeader = 128;    // discount list, the two residual slots
constexpr int32_t kPlanMaxSweeps = 1 << 20;

struct SweepsPlan {
  TablePlan launch;
  int32_t off_v0, off_v1, off_w, off_c4;     // byte offsets into the dynamic LDS
};

// The LDS a table of S states takes: header, entries [5][S] x 8 bytes, two value vectors, and for
// a policy the weights [5][S] and the totals [S].  An override costs nothing: the staged entry
// holds the reward the sweeps use, wherever it came from.
inline int32_t plan_sweeps(int64_t S, int32_t policy, int32_t has_override, int64_t lds_max,
                           int32_t path, SweepsPlan* p, int64_t* plan_out) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || (policy & ~1) || (has_override & ~1)) return CAMPX_EINVAL;
  memset(p, 0, sizeof(*p));
  int64_t at = kPlanLdsHeader + up16(S * CAMPX_N_ACTIONS * (int64_t)sizeof(uint2));
  p->off_v0 = (int32_t)at;
  at += up16(S * 4);
  p->off_v1 = (int32_t)at;
  at += up16(S * 4);
  if (policy) {
    p->off_w = (int32_t)at;
    at += up16(S * CAMPX_N_ACTIONS * 4);
    p->off_c4 = (int32_t)at;
    at += up16(S * 4);
  }
  return plan_lds_or_launch(S, at, true, lds_max, path, kPlanThreads, &p->launch, plan_out);
}

struct SweepParams {
  int32_t S, n_sweeps;
  float gamma;
  float discounts[16];
  int32_t off_v0, off_v1, off_w, off_c4;
};

// q of one entry whose reward word is already the reward to use, given v[next].
__device__ __forceinline__ float backup(uint2 e, float gamma, const float* discounts, float vn) {
  const float r = __uint_as_float(e.x);
  const uint32_t done = entry_done(e.y), dcode = entry_dcode(e.y);
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

template <bool kPolicy>
__global__ __launch_bounds__(kTableLdsThreads) void wide_sweeps_lds_kernel(
    SweepParams sp, const uint2* __restrict__ g_entries, const float* __restrict__ g_policy,
    const float* __restrict__ g_reward, const float* v_in, float* v_out, float* __restrict__ q_out,
    int8_t* __restrict__ greedy_out, uint32_t* __restrict__ residual, int32_t* __restrict__ bad_rows,
    int32_t* __restrict__ bad_flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_plan[];
  float* discounts = reinterpret_cast<float*>(lds_plan);                 // [16]
  uint32_t* red = reinterpret_cast<uint32_t*>(lds_plan + 64);            // [2]: sweep k uses k & 1
  uint2* ent = reinterpret_cast<uint2*>(lds_plan + kPlanLdsHeader);      // [5][S]
  float* vi = reinterpret_cast<float*>(lds_plan + sp.off_v0);
  float* vo = reinterpret_cast<float*>(lds_plan + sp.off_v1);
  float* wts = reinterpret_cast<float*>(lds_plan + sp.off_w);            // [5][S]
  float* tot = reinterpret_cast<float*>(lds_plan + sp.off_c4);           // [S]
  const int S = sp.S, nt = (int)blockDim.x, tid = (int)threadIdx.x;
  for (int i = tid; i < S * CAMPX_N_ACTIONS; i += nt) {
    const uint2 e = g_entries[i];
    const float r = real_reward(g_reward ? g_reward[i] : __uint_as_float(e.x));
    const int s = i / CAMPX_N_ACTIONS, a = i - s * CAMPX_N_ACTIONS;
    ent[a * S + s] = make_uint2(__float_as_uint(r), e.y);
  }
  for (int s = tid; s < S; s += nt) {
    vi[s] = v_in[s];
    if (kPolicy) {
      float w[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) w[a] = g_policy[s * CAMPX_N_ACTIONS + a];
#pragma unroll
      for (int a = 0; a < 5; ++a) wts[a * S + s] = w[a];
      tot[s] = policy_row_total(w);
    }
  }
  if (tid < 16) discounts[tid] = sp.discounts[tid];
  if (tid < 2) red[tid] = 0;
  __syncthreads();

  int bad = 0;
  for (int k = 0; k < sp.n_sweeps; ++k) {
    const bool last = k == sp.n_sweeps - 1;
    uint32_t m = 0;
    for (int s = tid; s < S; s += nt) {
      float q[5], vn[5], w[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, c4 = 0.0f;
      uint2 e[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) e[a] = ent[a * S + s];
#pragma unroll
      for (int a = 0; a < 5; ++a) vn[a] = vi[entry_target(e[a].y, (uint32_t)S)];   // five in flight
#pragma unroll
      for (int a = 0; a < 5; ++a) q[a] = backup(e[a], sp.gamma, discounts, vn[a]);
      if (kPolicy) {
#pragma unroll
        for (int a = 0; a < 5; ++a) w[a] = wts[a * S + s];
        c4 = tot[s];
      }
      int arg;
      const float v = reduce_q<kPolicy>(q, w, c4, arg);
      vo[s] = v;
      const uint32_t diff = __float_as_uint(fabsf(v - vi[s]));
      m = diff > m ? diff : m;
      if (last) {
        if (q_out) {
#pragma unroll
          for (int a = 0; a < 5; ++a) q_out[s * CAMPX_N_ACTIONS + a] = q[a];
        }
        if (greedy_out) greedy_out[s] = (int8_t)arg;
        bad += kPolicy && c4 == 0.0f;
      }
    }
    m = wave_max(m);
    if ((tid & 63) == 0 && m) atomicMax(&red[k & 1], m);
    __syncthreads();               // v_k and its residual are complete; v_{k-1} is free
    if (tid == 0) {
      residual[k] = red[k & 1];
      red[k & 1] = 0;              // (used again by sweep k + 2, past the next barrier)
    }
    float* t = vi;
    vi = vo;
    vo = t;
  }
  for (int s = tid; s < S; s += nt) v_out[s] = vi[s];
  report_bad(bad_rows, bad_flag, bad);
}

// What the global path starts with: the residual slots to zero (the sweeps raise them with
// atomicMax) and - v_in == v_out with an odd number of sweeps - a copy of the values to start from.
__global__ __launch_bounds__(kPlanThreads) void sweeps_prepare_kernel(
    uint32_t* __restrict__ residual, int32_t n, const float* __restrict__ src,
    float* __restrict__ dst, int32_t S) {
  const int first = (int)(blockIdx.x * kPlanThreads + threadIdx.x);
  const int step = (int)(gridDim.x * kPlanThreads);
  for (int i = first; i < n; i += step) residual[i] = 0;
  if (dst)
    for (int i = first; i < S; i += step) dst[i] = src[i];
}

template <bool kPolicy>
__global__ __launch_bounds__(kPlanThreads) void wide_sweep_kernel(
    SweepParams sp, const uint2* __restrict__ entries, const float* __restrict__ policy,
    const float* __restrict__ reward, const float* __restrict__ v_src, float* __restrict__ v_dst,
    float* __restrict__ q_out, int8_t* __restrict__ greedy_out, uint32_t* __restrict__ residual,
    int32_t* __restrict__ bad_rows, int32_t* __restrict__ bad_flag, int32_t last) {
  __shared__ float discounts[16];
  __shared__ uint32_t partial[kPlanThreads / 64];
  const int tid = (int)threadIdx.x;
  if (tid < 16) discounts[tid] = sp.discounts[tid];
  __syncthreads();
  const int s = (int)(blockIdx.x * kPlanThreads) + tid;
  const bool live = s < sp.S;
  const int row = (live ? s : sp.S - 1) * CAMPX_N_ACTIONS;        // any valid row
  uint2 e[5];
  float w[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, c4 = 0.0f;
#pragma unroll
  for (int a = 0; a < 5; ++a) e[a] = entries[row + a];
  if (reward) {
#pragma unroll
    for (int a = 0; a < 5; ++a) e[a].x = __float_as_uint(reward[row + a]);
  }
  if (kPolicy) {
#pragma unroll
    for (int a = 0; a < 5; ++a) w[a] = policy[row + a];
    c4 = policy_row_total(w);
  }
  const float before = v_src[live ? s : sp.S - 1];
  float q[5], vn[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) vn[a] = v_src[entry_target(e[a].y, (uint32_t)sp.S)];   // five in flight
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    e[a].x = __float_as_uint(real_reward(__uint_as_float(e[a].x)));
    q[a] = backup(e[a], sp.gamma, discounts, vn[a]);
  }
  int arg;
  const float v = reduce_q<kPolicy>(q, w, c4, arg);
  uint32_t m = 0;
  if (live) {
    v_dst[s] = v;
    m = __float_as_uint(fabsf(v - before));
    if (last) {
      if (q_out) {
#pragma unroll
        for (int a = 0; a < 5; ++a) q_out[row + a] = q[a];
      }
      if (greedy_out) greedy_out[s] = (int8_t)arg;
    }
  }
  m = wave_max(m);
  if ((tid & 63) == 0) partial[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < kPlanThreads / 64; ++i) m = partial[i] > m ? partial[i] : m;
    if (m) atomicMax(residual, m);
  }
  if (last) report_bad(bad_rows, bad_flag, (live && kPolicy && c4 == 0.0f) ? 1 : 0);
}

// ---------------------------------------------------------------------------- a population
//
// evaluate_policy() for P policies at once: member m is the policy reduction above with
// policies[m] and gamma[m], nothing else.  Members share the table and nothing they write, so the
// only questions are where a member's vectors live and which lane takes which (member, state)
// pair - and by the rule neither can change a bit.
//
// population_sweeps_lds_kernel   a workgroup owns G consecutive members.  The entries are staged
//     once per workgroup, as above; behind them, per sweep parity, G residual slots; the members'
//     gammas; and the members' vectors, each FLAT over the pairs i = g * S + s: two value vectors
//     [G * S], the weights [5][G * S], the totals [G * S] - so that pair i is lane i's in every
//     one of them and a wave reads consecutive addresses whether it sits inside a member, across
//     two, or holds several.  One __syncthreads() per sweep for all G members, all n sweeps in
//     the one launch.
// population_sweep_kernel        one launch per sweep, a lane per pair, a workgroup per 256 states
//     of ONE member, the blocks of all members flattened into grid.x.
// Either grid stops at kPopMaxGrid workgroups; a workgroup takes the groups (or blocks) that are
// a whole grid apart, one after the other.

constexpr int64_t kPopMaxGrid = 1 << 20;
constexpr int64_t kPopMaxElements = 0x7fffffff;      // P * S * 5, the elements of `policies`

struct PopulationPlan {
  int32_t path, threads, G;
  int64_t grid, lds_bytes, groups;           // groups: of G members (path 1) / blocks of 256 states (path 2)
  int32_t off_red, off_gamma, off_v0, off_v1, off_w, off_c4;
};

// The LDS G members of S states take, and where its parts start.
inline int64_t population_lds(int64_t S, int64_t G, PopulationPlan* p) {
  int64_t at = kPlanLdsHeader + up16(S * CAMPX_N_ACTIONS * (int64_t)sizeof(uint2));
  const int64_t red = at;
  at += up16(2 * G * 4);
  const int64_t gam = at;
  at += up16(G * 4);
  const int64_t v0 = at;
  at += up16(G * S * 4);
  const int64_t v1 = at;
  at += up16(G * S * 4);
  const int64_t w = at;
  at += up16(G * S * CAMPX_N_ACTIONS * 4);
  const int64_t c4 = at;
  at += up16(G * S * 4);
  if (p && at <= 0x7fffffff) {
    p->off_red = (int32_t)red;
    p->off_gamma = (int32_t)gam;
    p->off_v0 = (int32_t)v0;
    p->off_v1 = (int32_t)v1;
    p->off_w = (int32_t)w;
    p->off_c4 = (int32_t)c4;
  }
  return at;
}

// How many members a workgroup of the LDS path takes.  The least of
//   (a) what fits lds_max;
//   (b) floor(kPopPackThreads / S), at least 1: members are packed until the workgroup has about
//       four waves of (member, state) pairs, no further;
//   (c) ceil(P / n_cus): a population smaller than G * n_cus would leave CUs idle, so it is spread
//       one workgroup per CU first and packed only beyond that.
// (b) is not the rule this started from, ceil(kTableLdsThreads / S) - pack until every one of the
// workgroup's 1 024 threads has a pair.  One run on an MI355X at P = 65 536, 64 sweeps, G bounded
// through (a) (NOTES.md has the table): the maze's 159 states 5.77 ms at G = 7 (1 113 pairs: a second
// round for 89 of them), 5.32 at 6, 3.71 at 3, 3.40 at G = 1; the boat race's 8 states 0.226 ms at
// G = 128 (1 024 threads), 0.185-0.199 from 64 down to 8, 0.319 at 4 and 1.15 at G = 1, where most
// of a wave idles.  Several small workgroups to a CU beat one large one, and a part-filled wave
// costs more than either: 256 threads is the size that is best or within a tenth of it at both,
// and a floor keeps a table of up to 256 states to one pair per thread.  Two sizes, one run: a
// choice with a reason, not a tuned one.  (c) has not been measured at all.
// Path 1 whenever one member fits.
constexpr int64_t kPopPackThreads = 256;
inline int32_t plan_population(int64_t S, int64_t P, int32_t has_override, int64_t lds_max,
                               int64_t n_cus, int32_t path, PopulationPlan* p, int64_t* plan_out) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || P < 1 || (has_override & ~1) || n_cus < 1 ||
      lds_max < 0 || path < 0 || path > 2)
    return CAMPX_EINVAL;
  if (P > kPopMaxElements / (S * CAMPX_N_ACTIONS)) return CAMPX_EINVAL;
  memset(p, 0, sizeof(*p));
  const bool fits = population_lds(S, 1, nullptr) <= lds_max;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  if (path == 1 || (path == 0 && fits)) {
    int64_t G = kPopPackThreads / S;                                  // (b)
    if (G < 1) G = 1;
    const int64_t spread = (P + n_cus - 1) / n_cus;                   // (c)
    if (spread < G) G = spread;
    if (population_lds(S, G, nullptr) > lds_max) {                    // (a): the largest that fits
      int64_t lo = 1, hi = G - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (population_lds(S, mid, nullptr) <= lds_max) lo = mid;
        else hi = mid - 1;
      }
      G = lo;
    }
    p->path = 1;
    p->G = (int32_t)G;
    p->lds_bytes = population_lds(S, G, p);
    const int64_t t = (G * S + 63) / 64 * 64;
    p->threads = (int32_t)(t > kTableLdsThreads ? kTableLdsThreads : t);
    p->groups = (P + G - 1) / G;
  } else {
    p->path = 2;
    p->G = 1;                                  // a workgroup serves one member
    p->threads = kPlanThreads;
    p->groups = (S + kPlanThreads - 1) / kPlanThreads * P;
  }
  p->grid = p->groups > kPopMaxGrid ? kPopMaxGrid : p->groups;
  if (plan_out) {
    plan_out[0] = p->path;
    plan_out[1] = p->lds_bytes;
    plan_out[2] = p->threads;
    plan_out[3] = p->grid;
    plan_out[4] = p->G;
  }
  return CAMPX_OK;
}

struct PopulationParams {
  int32_t S, n_sweeps, G;
  float gamma;                               // of every member, where there is no gamma per member
  int64_t P, groups;
  float discounts[16];
  int32_t off_red, off_gamma, off_v0, off_v1, off_w, off_c4;
};

__global__ __launch_bounds__(kTableLdsThreads) void population_sweeps_lds_kernel(
    PopulationParams pp, const uint2* __restrict__ g_entries, const float* __restrict__ g_policies,
    const float* __restrict__ g_reward, const float* __restrict__ g_gammas, const float* v_in,
    float* v_out, float* __restrict__ q_out, uint32_t* __restrict__ residual,
    int32_t* __restrict__ bad_rows, int32_t* __restrict__ bad_flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_pop[];
  float* discounts = reinterpret_cast<float*>(lds_pop);                  // [16]
  uint2* ent = reinterpret_cast<uint2*>(lds_pop + kPlanLdsHeader);       // [5][S]
  uint32_t* red = reinterpret_cast<uint32_t*>(lds_pop + pp.off_red);     // [2][G]: sweep k uses k & 1
  float* gam = reinterpret_cast<float*>(lds_pop + pp.off_gamma);         // [G]
  float* v0 = reinterpret_cast<float*>(lds_pop + pp.off_v0);             // [G * S]
  float* v1 = reinterpret_cast<float*>(lds_pop + pp.off_v1);
  float* wts = reinterpret_cast<float*>(lds_pop + pp.off_w);             // [5][G * S]
  float* tot = reinterpret_cast<float*>(lds_pop + pp.off_c4);            // [G * S]
  const int S = pp.S, G = pp.G, GS = G * S, nt = (int)blockDim.x, tid = (int)threadIdx.x;
  for (int i = tid; i < S * CAMPX_N_ACTIONS; i += nt) {
    const uint2 e = g_entries[i];
    const float r = real_reward(g_reward ? g_reward[i] : __uint_as_float(e.x));
    const int s = i / CAMPX_N_ACTIONS, a = i - s * CAMPX_N_ACTIONS;
    ent[a * S + s] = make_uint2(__float_as_uint(r), e.y);
  }
  if (tid < 16) discounts[tid] = pp.discounts[tid];

  int bad = 0;
  for (int64_t group = blockIdx.x; group < pp.groups; group += gridDim.x) {
    const int64_t m0 = group * G;                                        // the group's first member
    const int members = (int)(pp.P - m0 < G ? pp.P - m0 : G);            // (the last group may be short)
    const int n = members * S;                                           // its pairs
    const int64_t row0 = m0 * S;                                         // pair 0 among all P * S
    float *vi = v0, *vo = v1;
    for (int i = tid; i < n; i += nt) {
      vi[i] = v_in[row0 + i];
      float w[5];
#pragma unroll
      for (int a = 0; a < 5; ++a) w[a] = g_policies[(row0 + i) * CAMPX_N_ACTIONS + a];
#pragma unroll
      for (int a = 0; a < 5; ++a) wts[a * GS + i] = w[a];
      tot[i] = policy_row_total(w);
    }
    for (int g = tid; g < members; g += nt) {
      gam[g] = g_gammas ? g_gammas[m0 + g] : pp.gamma;
      red[g] = 0;
      red[G + g] = 0;
    }
    __syncthreads();

    for (int k = 0; k < pp.n_sweeps; ++k) {
      const bool last = k == pp.n_sweeps - 1;
      uint32_t* redk = red + (k & 1) * G;
      for (int base = 0; base < n; base += nt) {          // every thread of the workgroup goes round
        const int i = base + tid;
        const bool live = i < n;
        int g = -1;
        uint32_t m = 0;
        if (live) {
          g = G == 1 ? 0 : i / S;
          const int s = i - g * S;
          const float* vg = vi + g * S;
          const float gamma = gam[g];
          float q[5], vn[5], w[5];
          uint2 e[5];
#pragma unroll
          for (int a = 0; a < 5; ++a) e[a] = ent[a * S + s];
#pragma unroll
          for (int a = 0; a < 5; ++a) vn[a] = vg[entry_target(e[a].y, (uint32_t)S)];   // five in flight
#pragma unroll
          for (int a = 0; a < 5; ++a) q[a] = backup(e[a], gamma, discounts, vn[a]);
#pragma unroll
          for (int a = 0; a < 5; ++a) w[a] = wts[a * GS + i];
          const float c4 = tot[i];
          int arg;
          const float v = reduce_q<true>(q, w, c4, arg);
          vo[i] = v;
          m = __float_as_uint(fabsf(v - vi[i]));
          if (last) {
            if (q_out) {
#pragma unroll
              for (int a = 0; a < 5; ++a) q_out[(row0 + i) * CAMPX_N_ACTIONS + a] = q[a];
            }
            bad += c4 == 0.0f;
          }
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
      __syncthreads();             // v_k and its residuals are complete; v_{k-1} is free
      for (int g = tid; g < members; g += nt) {
        residual[(int64_t)k * pp.P + m0 + g] = redk[g];
        redk[g] = 0;               // (used again by sweep k + 2, past the next barrier)
      }
      float* t = vi;
      vi = vo;
      vo = t;
    }
    for (int i = tid; i < n; i += nt) v_out[row0 + i] = vi[i];
    __syncthreads();               // the next group of this workgroup stages over these vectors
  }
  report_bad(bad_rows, bad_flag, bad);
}

// sweeps_prepare_kernel for a population: `n` residual slots, `n_values` values to copy.
__global__ __launch_bounds__(kPlanThreads) void population_prepare_kernel(
    uint32_t* __restrict__ residual, int64_t n, const float* __restrict__ src,
    float* __restrict__ dst, int64_t n_values) {
  const int64_t first = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kPlanThreads;
  for (int64_t i = first; i < n; i += step) residual[i] = 0;
  if (dst)
    for (int64_t i = first; i < n_values; i += step) dst[i] = src[i];
}

// `residual` is the row of the sweep: [P].
__global__ __launch_bounds__(kPlanThreads) void population_sweep_kernel(
    PopulationParams pp, const uint2* __restrict__ entries, const float* __restrict__ policies,
    const float* __restrict__ reward, const float* __restrict__ gammas,
    const float* __restrict__ v_src, float* __restrict__ v_dst, float* __restrict__ q_out,
    uint32_t* __restrict__ residual, int32_t* __restrict__ bad_rows, int32_t* __restrict__ bad_flag,
    int32_t last) {
  __shared__ float discounts[16];
  __shared__ uint32_t partial[kPlanThreads / 64];
  const int tid = (int)threadIdx.x, S = pp.S;
  if (tid < 16) discounts[tid] = pp.discounts[tid];
  __syncthreads();
  const int64_t per_member = (S + kPlanThreads - 1) / kPlanThreads;     // blocks of a member
  int bad = 0;
  for (int64_t block = blockIdx.x; block < pp.groups; block += gridDim.x) {
    const int64_t member = block / per_member;
    const int s = (int)(block - member * per_member) * kPlanThreads + tid;
    const bool live = s < S;
    const int row = (live ? s : S - 1) * CAMPX_N_ACTIONS;                // any valid row
    const int64_t first = member * S;                                    // the member's pair 0
    const int64_t mine = (first + (live ? s : S - 1)) * CAMPX_N_ACTIONS;
    const float* vm = v_src + first;
    const float gamma = gammas ? gammas[member] : pp.gamma;
    uint2 e[5];
    float w[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) e[a] = entries[row + a];
    if (reward) {
#pragma unroll
      for (int a = 0; a < 5; ++a) e[a].x = __float_as_uint(reward[row + a]);
    }
#pragma unroll
    for (int a = 0; a < 5; ++a) w[a] = policies[mine + a];
    const float c4 = policy_row_total(w);
    const float before = vm[live ? s : S - 1];
    float q[5], vn[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) vn[a] = vm[entry_target(e[a].y, (uint32_t)S)];   // five in flight
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      e[a].x = __float_as_uint(real_reward(__uint_as_float(e[a].x)));
      q[a] = backup(e[a], gamma, discounts, vn[a]);
    }
    int arg;
    const float v = reduce_q<true>(q, w, c4, arg);
    uint32_t m = 0;
    if (live) {
      v_dst[first + s] = v;
      m = __float_as_uint(fabsf(v - before));
      if (last) {
        if (q_out) {
#pragma unroll
          for (int a = 0; a < 5; ++a) q_out[mine + a] = q[a];
        }
        bad += c4 == 0.0f;
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
    __syncthreads();               // `partial` is written again by the next block
  }
  report_bad(bad_rows, bad_flag, bad);
}

// Compute units of the current device (256 where it cannot be asked): rule (c) of the plan.
inline int64_t device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  return cus;
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_sweeps_plan(int64_t n_states, int32_t policy, int32_t has_override,
                               int64_t wide_lds_max, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SweepsPlan p;
  return plan_sweeps(n_states, policy, has_override, wide_lds_max, path, &p, plan_out);
}

int32_t campx_wide_sweeps_launch(const CampxWideSpec* s, const void* tables_dev, const float* policy,
                                 const float* reward_override, float gamma, const float* v_in,
                                 float* v_out, float* scratch, float* q, int8_t* greedy,
                                 float* residual, int32_t* bad_rows, int32_t* bad_flag,
                                 int32_t n_sweeps, int32_t path, void* stream) {
  if (!s || !tables_dev || !v_in || !v_out || !residual) return CAMPX_EINVAL;
  if (n_sweeps < 1 || n_sweeps > kPlanMaxSweeps || !(fabsf(gamma) < INFINITY)) return CAMPX_EINVAL;
  if (!aligned_to(tables_dev, 8) || !aligned_to(policy, 4) || !aligned_to(reward_override, 4) ||
      !aligned_to(v_in, 4) || !aligned_to(v_out, 4) || !aligned_to(scratch, 4) || !aligned_to(q, 4) ||
      !aligned_to(residual, 4) || !aligned_to(bad_rows, 4))
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  const int64_t S = s->n_states;
  SweepsPlan sweeps;
  const int32_t e = plan_sweeps(S, policy ? 1 : 0, reward_override ? 1 : 0, knob(K_WIDE_LDS_MAX), path,
                                &sweeps, nullptr);
  if (e != CAMPX_OK) return e;
  const TablePlan& plan = sweeps.launch;
  const int64_t bytes = S * (int64_t)sizeof(float);
  // the values to start from and the values to leave are one vector or two apart
  if (v_in != v_out && ranges_overlap(v_in, v_out, bytes)) return CAMPX_EINVAL;
  SweepParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.S = (int32_t)S;
  sp.n_sweeps = n_sweeps;
  sp.gamma = gamma;
  wide_discounts(*s, sp.discounts);
  sp.off_v0 = sweeps.off_v0;
  sp.off_v1 = sweeps.off_v1;
  sp.off_w = sweeps.off_w;
  sp.off_c4 = sweeps.off_c4;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint2* entries = wide_tables(*s, tables_dev).entries;
  uint32_t* res = reinterpret_cast<uint32_t*>(residual);
  if (plan.path == 1) {
    const auto kernel = policy ? wide_sweeps_lds_kernel<true> : wide_sweeps_lds_kernel<false>;
    CAMPX_ALLOW_LDS(kernel, (size_t)plan.lds_bytes);
    hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, hs, sp,
                       entries, policy, reward_override, v_in, v_out, q, greedy, res, bad_rows, bad_flag);
    return launch_status();
  }
  // Sweep k of n writes v_out when n - k is even and the scratch vector when it is odd, so that
  // the last one writes v_out; sweep 1 reads v_in - or, where it would write the vector it reads
  // (v_in == v_out, n odd), the copy of it that the first kernel leaves in the scratch vector.
  if (!scratch || ranges_overlap(scratch, v_in, bytes) || ranges_overlap(scratch, v_out, bytes))
    return CAMPX_EINVAL;
  const bool copy = v_in == v_out && (n_sweeps & 1);
  {
    const int64_t most = (copy && S > n_sweeps) ? S : n_sweeps;
    const int64_t blocks = (most + 4 * kPlanThreads - 1) / (4 * kPlanThreads);
    hipLaunchKernelGGL(sweeps_prepare_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)),
                       dim3(kPlanThreads), 0, hs, res, n_sweeps, v_in, copy ? scratch : nullptr,
                       (int32_t)S);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
  }
  const float* src = copy ? scratch : v_in;
  const auto sweep = policy ? wide_sweep_kernel<true> : wide_sweep_kernel<false>;
  for (int32_t k = 1; k <= n_sweeps; ++k) {
    float* dst = ((n_sweeps - k) & 1) ? scratch : v_out;
    const int32_t last = k == n_sweeps;
    hipLaunchKernelGGL(sweep, dim3((unsigned)plan.grid), dim3(kPlanThreads), 0, hs, sp, entries, policy,
                       reward_override, src, dst, q, greedy, res + (k - 1), bad_rows, bad_flag, last);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
    src = dst;
  }
  return CAMPX_OK;
}

int32_t campx_wide_population_sweeps_plan(int64_t n_states, int64_t members, int32_t has_override,
                                          int64_t wide_lds_max, int64_t n_cus, int32_t path,
                                          int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  PopulationPlan p;
  return plan_population(n_states, members, has_override, wide_lds_max, n_cus, path, &p, plan_out);
}

int32_t campx_wide_population_sweeps_launch(const CampxWideSpec* s, const void* tables_dev,
                                            const float* policies, int64_t members,
                                            const float* reward_override, float gamma,
                                            const float* gammas, const float* v_in, float* v_out,
                                            float* scratch, float* q, float* residual,
                                            int32_t* bad_rows, int32_t* bad_flag, int32_t n_sweeps,
                                            int32_t path, void* stream) {
  if (!s || !tables_dev || !policies || !v_in || !v_out || !residual) return CAMPX_EINVAL;
  if (members < 1 || n_sweeps < 1 || n_sweeps > kPlanMaxSweeps) return CAMPX_EINVAL;
  if (!gammas && !(fabsf(gamma) < INFINITY)) return CAMPX_EINVAL;
  if (!aligned_to(tables_dev, 8) || !aligned_to(policies, 4) || !aligned_to(reward_override, 4) ||
      !aligned_to(gammas, 4) || !aligned_to(v_in, 4) || !aligned_to(v_out, 4) ||
      !aligned_to(scratch, 4) || !aligned_to(q, 4) || !aligned_to(residual, 4) ||
      !aligned_to(bad_rows, 4))
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  const int64_t S = s->n_states, P = members;
  if (P > kPopMaxElements / (S * CAMPX_N_ACTIONS)) return CAMPX_EINVAL;
  const int64_t bytes = P * S * (int64_t)sizeof(float);
  // the values to start from and the values to leave are one array or two apart
  if (v_in != v_out && ranges_overlap(v_in, v_out, bytes)) return CAMPX_EINVAL;
  const int64_t lds_max = knob(K_WIDE_LDS_MAX);
  const bool fits = population_lds(S, 1, nullptr) <= lds_max;
  if (path < 0 || path > 2 || (path == 1 && !fits)) return CAMPX_EINVAL;
  if (path == 2 || !fits) {                   // the global path: it needs a second array of values
    if (!scratch || ranges_overlap(scratch, v_in, bytes) || ranges_overlap(scratch, v_out, bytes))
      return CAMPX_EINVAL;
  }
  // (every refusal of an argument is decided above, before the device is asked anything)
  PopulationPlan plan;
  const int32_t e = plan_population(S, P, reward_override ? 1 : 0, lds_max, device_cus(), path, &plan,
                                    nullptr);
  if (e != CAMPX_OK) return e;
  PopulationParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.S = (int32_t)S;
  pp.n_sweeps = n_sweeps;
  pp.G = plan.G;
  pp.gamma = gamma;
  pp.P = P;
  pp.groups = plan.groups;
  wide_discounts(*s, pp.discounts);
  pp.off_red = plan.off_red;
  pp.off_gamma = plan.off_gamma;
  pp.off_v0 = plan.off_v0;
  pp.off_v1 = plan.off_v1;
  pp.off_w = plan.off_w;
  pp.off_c4 = plan.off_c4;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint2* entries = wide_tables(*s, tables_dev).entries;
  uint32_t* res = reinterpret_cast<uint32_t*>(residual);
  if (plan.path == 1) {
    CAMPX_ALLOW_LDS(population_sweeps_lds_kernel, (size_t)plan.lds_bytes);
    hipLaunchKernelGGL(population_sweeps_lds_kernel, dim3((unsigned)plan.grid),
                       dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, hs, pp, entries, policies,
                       reward_override, gammas, v_in, v_out, q, res, bad_rows, bad_flag);
    return launch_status();
  }
  // As campx_wide_sweeps_launch(): sweep k of n writes v_out when n - k is even and the scratch
  // array when it is odd; sweep 1 reads v_in or - v_in == v_out, n odd - its copy in the scratch.
  const bool copy = v_in == v_out && (n_sweeps & 1);
  {
    const int64_t slots = (int64_t)n_sweeps * P, values = P * S;
    const int64_t most = (copy && values > slots) ? values : slots;
    const int64_t blocks = (most + 4 * kPlanThreads - 1) / (4 * kPlanThreads);
    hipLaunchKernelGGL(population_prepare_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)),
                       dim3(kPlanThreads), 0, hs, res, slots, v_in, copy ? scratch : nullptr, values);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
  }
  const float* src = copy ? scratch : v_in;
  for (int32_t k = 1; k <= n_sweeps; ++k) {
    float* dst = ((n_sweeps - k) & 1) ? scratch : v_out;
    const int32_t last = k == n_sweeps;
    hipLaunchKernelGGL(population_sweep_kernel, dim3((unsigned)plan.grid), dim3(kPlanThreads), 0, hs, pp,
                       entries, policies, reward_override, gammas, src, dst, q, res + (int64_t)(k - 1) * P,
                       bad_rows, bad_flag, last);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
    src = dst;
  }
  return CAMPX_OK;
}

}  // extern "C"
