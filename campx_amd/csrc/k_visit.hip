// k_visit.hip - exact state visitation of a policy on a game's state table: the FORWARD half of
// the deterministic MDP that k_plan.hip sweeps backwards.  Given the weights rollout_policy()
// samples from, how much probability sits in each state at each frame and how often each
// (state, action) is taken - what rollout_policy() + sum_by_state() can only estimate.
//
// The rule (include/campx_hip.h has it in full; tests/visitation_reference.py restates it in
// numpy): mass is an int64 in units of 2^-38.  Per state, N_i = how many of the sampler's 2^24
// values u play an action <= i, found by bisection on the sampler's own f32 product and
// comparison; a state's mass m splits into x_a = y_a - y_{a-1}, y_i = floor(m * N_i / 2^24), which
// sums to m exactly; x_a moves to the entry's next state, or - an entry that ends the episode -
// is counted into finished[t] and, with `restart`, moves to state 0.  Every addition is an integer
// addition: the scatter gives the same bits whatever order the lanes arrive in, so both paths
// below, a continued call and the numpy restatement agree bit for bit.
//
// visit_counts_kernel     a lane per state: the bisection, `counts`, the bad rows; on the global
//     path also the two mass buffers the first frame starts from and the zeroes of `finished`.
// visit_lds_kernel        one workgroup holds the entries' next / done words, N and two mass
//     vectors in LDS and runs ALL frames of the call, one __syncthreads() per frame; scatters are
//     64-bit LDS atomic adds; `visits` stays in the registers of the lane that owns the state.
// visit_frame_kernel      one launch per frame, a lane per state; scatters are no-return 64-bit
//     global atomic adds; the mass that ends an episode is summed across the wave first, so that
//     finished[t] and state 0 take one atomic per wave; the lane that reads d[s] clears it, so
//     that the buffer is zero when it is the target of the frame after next.
// plan_visit() chooses; campx_wide_visit_plan() shows the choice to a test without a GPU.
//
// A population: member m of P is the rule above with policies[m] and its own start, and nothing
// else.  Members share the table and nothing they write, so - as in k_plan.hip - the only questions
// are where a member's vectors live and which lane takes which (member, state) pair, and since
// only integers are added neither can change a bit.  The population has kernels of its own next to
// the three above, which stay as they are; both sets call the same device helpers.
// visit_population_counts_kernel   a lane per (member, state) row over all P * S rows; on the
//     global path also the two [P][S] mass buffers and the zeroes of finished[n_frames][P].  A
//     shared start is read with member stride 0.
// visit_population_lds_kernel      a workgroup stages the entries' second words [5][S] ONCE and
//     takes G consecutive members through ALL frames: per member N [4][S], two mass vectors [S] and
//     two slots of finished[t], FLAT over the pairs i = g * S + s.  G = 1: up to 1 024 lanes own up
//     to kVisitPerLane states each, as in visit_lds_kernel; G > 1: the G * S <= 256 pairs are one to
//     a lane.  A wave that holds pairs of several members (S < 64) hands its ended mass out lane by
//     lane, each to its own member's slot and state 0; a wave inside one member sums it first.
// visit_population_frame_kernel    one launch per frame for ALL members, a workgroup per 256 states
//     of ONE member (so a wave never holds two), the blocks of all members along grid.x.
// Either grid stops at kVisitMaxGrid workgroups; a workgroup takes the groups (or blocks) that are
// a whole grid apart, one after the other.  plan_visit_population() chooses;
// campx_wide_visit_population_plan() shows the choice to a test without a GPU.

#include "wide_table.hip.h"

namespace campx_impl {

typedef unsigned long long u64;

constexpr int kVisitPerLane = 3;           // states a lane of the LDS workgroup owns, at most
constexpr int kVisitThreads = 256;         // global path, and the counts
constexpr int64_t kVisitLdsHeader = 64;    // the two slots of finished[t]
constexpr int32_t kVisitMaxFrames = 1 << 20;
constexpr uint32_t kVisitWords = 1u << 24; // the sampler's values u

struct VisitPlan {
  TablePlan launch;
  int32_t off_n, off_d0, off_d1;     // byte offsets into the dynamic LDS
};

// The LDS a table of S states takes: header, the entries' second words [5][S] x 4 bytes, N [4][S]
// x 4 bytes and two mass vectors [S] x 8 bytes - 52 bytes per state.  A lane keeps the visits of
// the states it owns in registers, kVisitPerLane of them at most.
static inline int32_t plan_visit(int64_t S, int64_t lds_max, int32_t path, VisitPlan* p,
                                 int64_t* plan_out) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES) return CAMPX_EINVAL;
  memset(p, 0, sizeof(*p));
  int64_t at = kVisitLdsHeader + up16(S * CAMPX_N_ACTIONS * 4);
  p->off_n = (int32_t)at;
  at += up16(S * 4 * 4);
  p->off_d0 = (int32_t)at;
  at += up16(S * 8);
  p->off_d1 = (int32_t)at;
  at += up16(S * 8);
  return plan_lds_or_launch(S, at, S <= (int64_t)kTableLdsThreads * kVisitPerLane, lds_max, path,
                            kVisitThreads, &p->launch, plan_out);
}

// The smallest u in 0 .. 2^24 whose product reaches the threshold (2^24: none does): the
// sampler's own multiply and comparison, which are monotone in u.  25 steps halve 2^24 + 1
// candidates down to one.
__device__ __forceinline__ uint32_t first_word_reaching(float threshold, float c4) {
  uint32_t lo = 0, hi = kVisitWords;
#pragma unroll 1
  for (int step = 0; step < 25; ++step) {
    const uint32_t mid = (lo + hi) >> 1;
    const float u = (float)mid * 5.9604644775390625e-8f;     // 2^-24: exact
    const float r = u * c4;
    const bool ok = r >= threshold;
    hi = ok ? mid : hi;
    lo = ok ? lo : mid + 1;
  }
  return hi;
}

// y_i = floor(m * n / 2^24) for 0 <= m < 2^62, n <= 2^24, without overflow.
__device__ __forceinline__ u64 share(u64 m, uint32_t n) {
  return (m >> 24) * n + (((m & 0xffffffull) * n) >> 24);
}

// x[a]: the mass each action takes, from the counts of the row.
__device__ __forceinline__ void split_mass(u64 m, const uint32_t (&n)[4], u64 (&x)[5]) {
  const u64 y0 = share(m, n[0]), y1 = share(m, n[1]), y2 = share(m, n[2]), y3 = share(m, n[3]);
  x[0] = y0;
  x[1] = y1 - y0;
  x[2] = y2 - y1;
  x[3] = y3 - y2;
  x[4] = m - y3;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

__device__ __forceinline__ void lds_add(u64* p, u64 v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void global_add(u64* p, u64 v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `counts` and the bad rows of every state; with `d_first` (global path) also the mass the first
// frame reads - `start`, or one environment in state 0 -, zeroes where it scatters to, and the
// zeroes of finished[0 .. n_frames).  Each lane touches element s of each vector only, and reads
// start[s] before it writes, so `start` may be either buffer.
__global__ __launch_bounds__(kVisitThreads) void visit_counts_kernel(
    int32_t S, const float* __restrict__ policy, int32_t* __restrict__ counts, const u64* start,
    u64* d_first, u64* d_second, u64* __restrict__ finished, int32_t n_frames,
    int32_t* __restrict__ bad_rows, int32_t* __restrict__ bad_flag) {
  const int first = (int)(blockIdx.x * kVisitThreads + threadIdx.x);
  if (d_first) {
    const int step = (int)(gridDim.x * kVisitThreads);
    for (int i = first; i < n_frames; i += step) finished[i] = 0;
  }
  const int s = first;
  if (s >= S) return;
  float c[5];
  policy_thresholds(policy + (int64_t)s * CAMPX_N_ACTIONS, c);
  uint32_t before = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t n = first_word_reaching(c[i], c[4]);
    counts[s * CAMPX_N_ACTIONS + i] = (int32_t)(n - before);
    before = n;
  }
  counts[s * CAMPX_N_ACTIONS + 4] = (int32_t)(kVisitWords - before);
  if (d_first) {
    const u64 m = start ? start[s] : (s == 0 ? (1ull << CAMPX_VISIT_FRAC_BITS) : 0ull);
    d_second[s] = 0;
    d_first[s] = m;
  }
  report_bad(bad_rows, bad_flag, c[4] == 0.0f);
}

struct VisitParams {
  int32_t S, n_frames, restart;
  int32_t off_n, off_d0, off_d1;
};

__global__ __launch_bounds__(kTableLdsThreads) void visit_lds_kernel(
    VisitParams vp, const uint2* __restrict__ g_entries, const int32_t* __restrict__ g_counts,
    const u64* start, u64* __restrict__ visits, u64* __restrict__ finished, u64* final_out,
    u64* __restrict__ per_frame) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_visit[];
  u64* fin = reinterpret_cast<u64*>(lds_visit);                              // [2]: frame t uses t & 1
  uint32_t* ent = reinterpret_cast<uint32_t*>(lds_visit + kVisitLdsHeader);  // [5][S]
  uint32_t* cum = reinterpret_cast<uint32_t*>(lds_visit + vp.off_n);         // [4][S]
  u64* cur = reinterpret_cast<u64*>(lds_visit + vp.off_d0);
  u64* nxt = reinterpret_cast<u64*>(lds_visit + vp.off_d1);
  const int S = vp.S, nt = (int)blockDim.x, tid = (int)threadIdx.x;
  for (int i = tid; i < S * CAMPX_N_ACTIONS; i += nt) {
    const int s = i / CAMPX_N_ACTIONS, a = i - s * CAMPX_N_ACTIONS;
    ent[a * S + s] = g_entries[i].y;
  }
  for (int s = tid; s < S; s += nt) {
    uint32_t n = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      n += (uint32_t)g_counts[s * CAMPX_N_ACTIONS + a];
      cum[a * S + s] = n;
    }
    cur[s] = start ? start[s] : (s == 0 ? (1ull << CAMPX_VISIT_FRAC_BITS) : 0ull);
    nxt[s] = 0;
  }
  if (tid < 2) fin[tid] = 0;
  __syncthreads();

  u64 acc[kVisitPerLane][5];
#pragma unroll
  for (int j = 0; j < kVisitPerLane; ++j)
#pragma unroll
    for (int a = 0; a < 5; ++a) acc[j][a] = 0;

  for (int t = 0; t < vp.n_frames; ++t) {
    u64 over = 0;
#pragma unroll
    for (int j = 0; j < kVisitPerLane; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        const u64 m = cur[s];
        if (per_frame) per_frame[(int64_t)t * S + s] = m;
        if (m) {
          cur[s] = 0;            // the target of frame t + 1: nobody else touches it in frame t
          uint32_t n[4], e[5];
          u64 x[5];
#pragma unroll
          for (int a = 0; a < 4; ++a) n[a] = cum[a * S + s];
#pragma unroll
          for (int a = 0; a < 5; ++a) e[a] = ent[a * S + s];
          split_mass(m, n, x);
#pragma unroll
          for (int a = 0; a < 5; ++a) {
            acc[j][a] += x[a];
            if (x[a]) {
              if (entry_done(e[a])) over += x[a];
              else lds_add(&nxt[entry_target(e[a], (uint32_t)S)], x[a]);
            }
          }
        }
      }
    }
    over = wave_sum(over);
    if ((tid & 63) == 0 && over) {
      lds_add(&fin[t & 1], over);
      if (vp.restart) lds_add(&nxt[0], over);
    }
    __syncthreads();               // d_{t+1} and finished[t] are complete; d_t is all zero
    if (tid == 0) {
      finished[t] = fin[t & 1];
      fin[t & 1] = 0;              // (used again by frame t + 2, past the next barrier)
    }
    u64* swap = cur;
    cur = nxt;
    nxt = swap;
  }
#pragma unroll
  for (int j = 0; j < kVisitPerLane; ++j) {
    const int s = tid + j * nt;
    if (s < S) {
      const u64 m = cur[s];
      final_out[s] = m;
      if (per_frame) per_frame[(int64_t)vp.n_frames * S + s] = m;
#pragma unroll
      for (int a = 0; a < 5; ++a) visits[s * CAMPX_N_ACTIONS + a] = acc[j][a];
    }
  }
}

// One frame.  `src` is d_t and is left all zero, `dst` - zero when the launch starts, but for what
// the workgroups of this launch have added - becomes d_{t+1}.  `first`: visits are written, not
// added to.  `row`: per_frame[t], or NULL.
__global__ __launch_bounds__(kVisitThreads) void visit_frame_kernel(
    int32_t S, int32_t restart, int32_t first, const uint2* __restrict__ entries,
    const int32_t* __restrict__ counts, u64* src, u64* dst, u64* __restrict__ visits,
    u64* __restrict__ finished_t, u64* __restrict__ row) {
  const int s = (int)(blockIdx.x * kVisitThreads + threadIdx.x);
  u64 over = 0;
  if (s < S) {
    const u64 m = src[s];
    if (row) row[s] = m;
    u64 x[5] = {0, 0, 0, 0, 0};
    if (m) {
      src[s] = 0;                  // the target of the frame after next
      uint32_t n[4], word[5];
      const int at = s * CAMPX_N_ACTIONS;
#pragma unroll
      for (int a = 0; a < 5; ++a) word[a] = entries[at + a].y;
      uint32_t sum = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        sum += (uint32_t)counts[at + a];
        n[a] = sum;
      }
      split_mass(m, n, x);
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        if (x[a]) {
          if (entry_done(word[a])) over += x[a];
          else global_add(&dst[entry_target(word[a], (uint32_t)S)], x[a]);
        }
      }
    }
    if (first) {
#pragma unroll
      for (int a = 0; a < 5; ++a) visits[(int64_t)s * CAMPX_N_ACTIONS + a] = x[a];
    } else if (m) {
#pragma unroll
      for (int a = 0; a < 5; ++a) visits[(int64_t)s * CAMPX_N_ACTIONS + a] += x[a];
    }
  }
  // every lane of the wave is here: the mass that ended an episode goes out once per wave
  over = wave_sum(over);
  if ((threadIdx.x & 63) == 0 && over) {
    global_add(finished_t, over);
    if (restart) global_add(&dst[0], over);
  }
}

// per_frame[n_frames] = d_T, which the last frame left in `final`.
__global__ __launch_bounds__(kVisitThreads) void visit_last_row_kernel(
    int32_t S, const u64* __restrict__ final_in, u64* __restrict__ row) {
  const int s = (int)(blockIdx.x * kVisitThreads + threadIdx.x);
  if (s < S) row[s] = final_in[s];
}

// ------------------------------------------------------------------------------- a population

constexpr int64_t kVisitMaxGrid = 1 << 20;
constexpr int64_t kVisitMaxElements = 0x7fffffff;    // P * S * 5, the elements of `policies`
constexpr int64_t kVisitPackThreads = 256;           // pairs a workgroup is packed up to
constexpr int64_t kVisitMemberHeader = 16;           // a member's two slots of finished[t]

struct VisitPopulationPlan {
  int32_t path, threads, G;
  int64_t grid, lds_bytes, groups;   // groups: of G members (path 1) / blocks of 256 states (path 2)
  int32_t off_ent, off_n, off_d0, off_d1;            // byte offsets into the dynamic LDS
};

// The LDS G members of S states take: plan_visit()'s header, which has the first member's two
// slots of finished[t], and 16 bytes for those of each further member; the entries' second words
// [5][S] x 4 bytes once; per member N [4][S] x 4 bytes and two mass vectors [S] x 8 bytes, flat
// over the G * S pairs.  At G = 1 this is plan_visit()'s account, byte for byte.
inline int64_t visit_population_lds(int64_t S, int64_t G, VisitPopulationPlan* p) {
  int64_t at = kVisitLdsHeader + (G - 1) * kVisitMemberHeader;
  const int64_t ent = at;
  at += up16(S * CAMPX_N_ACTIONS * 4);
  const int64_t n = at;
  at += up16(G * S * 4 * 4);
  const int64_t d0 = at;
  at += up16(G * S * 8);
  const int64_t d1 = at;
  at += up16(G * S * 8);
  if (p && at <= 0x7fffffff) {
    p->off_ent = (int32_t)ent;
    p->off_n = (int32_t)n;
    p->off_d0 = (int32_t)d0;
    p->off_d1 = (int32_t)d1;
  }
  return at;
}

// The plan of P members.  Path 1 whenever one member fits, by plan_visit()'s own test.  How many
// members a workgroup of the LDS path takes is the rule of k_plan.hip's plan_sweeps(), taken over
// as it stands and NOT tuned for this kernel - the least of (a) what fits lds_max, (b)
// floor(kVisitPackThreads / S), at least 1, (c) ceil(P / n_cus).
inline int32_t plan_visit_population(int64_t S, int64_t P, int64_t lds_max, int64_t n_cus,
                                     int32_t path, VisitPopulationPlan* p) {
  if (S < 1 || S > CAMPX_WIDE_MAX_STATES || P < 1 || n_cus < 1 || lds_max < 0 || path < 0 || path > 2)
    return CAMPX_EINVAL;
  if (P > kVisitMaxElements / (S * CAMPX_N_ACTIONS)) return CAMPX_EINVAL;
  memset(p, 0, sizeof(*p));
  const bool fits = visit_population_lds(S, 1, nullptr) <= lds_max &&
                    S <= (int64_t)kTableLdsThreads * kVisitPerLane;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  if (path == 1 || (path == 0 && fits)) {
    int64_t G = kVisitPackThreads / S;                                // (b)
    if (G < 1) G = 1;
    const int64_t spread = (P + n_cus - 1) / n_cus;                   // (c)
    if (spread < G) G = spread;
    if (visit_population_lds(S, G, nullptr) > lds_max) {              // (a): the largest that fits
      int64_t lo = 1, hi = G - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (visit_population_lds(S, mid, nullptr) <= lds_max) lo = mid;
        else hi = mid - 1;
      }
      G = lo;
    }
    p->path = 1;
    p->G = (int32_t)G;
    p->lds_bytes = visit_population_lds(S, G, p);
    const int64_t t = (G * S + 63) / 64 * 64;        // G > 1: at most 256, a pair per lane
    p->threads = (int32_t)(t > kTableLdsThreads ? kTableLdsThreads : t);
    p->groups = (P + G - 1) / G;
  } else {
    p->path = 2;
    p->G = 1;                                        // a workgroup serves one member
    p->threads = kVisitThreads;
    p->groups = (S + kVisitThreads - 1) / kVisitThreads * P;
  }
  p->grid = p->groups > kVisitMaxGrid ? kVisitMaxGrid : p->groups;
  return CAMPX_OK;
}

struct VisitPopulationParams {
  int32_t S, n_frames, restart, G;
  int64_t P, groups;
  int64_t start_stride;              // S: a start per member; 0: one start shared by all
  int32_t off_ent, off_n, off_d0, off_d1;
};

// visit_counts_kernel for all P * S rows.  Row r = m * S + s reads start[m * start_stride + s]
// before it writes element r of either buffer, so a start per member may be either buffer.
__global__ __launch_bounds__(kVisitThreads) void visit_population_counts_kernel(
    int32_t S, int64_t rows, int64_t start_stride, const float* __restrict__ policies,
    int32_t* __restrict__ counts, const u64* start, u64* d_first, u64* d_second,
    u64* __restrict__ finished, int64_t n_finished, int32_t* __restrict__ bad_rows,
    int32_t* __restrict__ bad_flag) {
  const int64_t first = (int64_t)blockIdx.x * kVisitThreads + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kVisitThreads;
  if (d_first)
    for (int64_t i = first; i < n_finished; i += step) finished[i] = 0;
  int bad = 0;
  for (int64_t r = first; r < rows; r += step) {
    float c[5];
    policy_thresholds(policies + r * CAMPX_N_ACTIONS, c);
    uint32_t before = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t n = first_word_reaching(c[i], c[4]);
      counts[r * CAMPX_N_ACTIONS + i] = (int32_t)(n - before);
      before = n;
    }
    counts[r * CAMPX_N_ACTIONS + 4] = (int32_t)(kVisitWords - before);
    if (d_first) {
      const int64_t m = r / S, s = r - m * S;
      const u64 mass = start ? start[m * start_stride + s] : (s == 0 ? (1ull << CAMPX_VISIT_FRAC_BITS) : 0ull);
      d_second[r] = 0;
      d_first[r] = mass;
    }
    bad += c[4] == 0.0f;
  }
  report_bad(bad_rows, bad_flag, bad);
}

// The grid never exceeds vp.groups, so a workgroup's first group is its own index.  `finished` is
// [n_frames][P], `per_frame` [n_frames + 1][P][S]; everything else is a member's own, [P][...].
__global__ __launch_bounds__(kTableLdsThreads) void visit_population_lds_kernel(
    VisitPopulationParams vp, const uint2* __restrict__ g_entries, const int32_t* __restrict__ g_counts,
    const u64* start, u64* __restrict__ visits, u64* __restrict__ finished, u64* final_out,
    u64* __restrict__ per_frame) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_members[];
  u64* fin = reinterpret_cast<u64*>(lds_members);                        // [2][G]: frame t uses t & 1
  uint32_t* ent = reinterpret_cast<uint32_t*>(lds_members + vp.off_ent); // [5][S]
  uint32_t* cum = reinterpret_cast<uint32_t*>(lds_members + vp.off_n);   // [4][G * S]
  u64* d0 = reinterpret_cast<u64*>(lds_members + vp.off_d0);             // [G * S]
  u64* d1 = reinterpret_cast<u64*>(lds_members + vp.off_d1);
  const int S = vp.S, G = vp.G, GS = G * S, nt = (int)blockDim.x, tid = (int)threadIdx.x;
  const int64_t P = vp.P, PS = P * S;
  for (int i = tid; i < S * CAMPX_N_ACTIONS; i += nt) {
    const int s = i / CAMPX_N_ACTIONS, a = i - s * CAMPX_N_ACTIONS;
    ent[a * S + s] = g_entries[i].y;
  }

  int64_t group = blockIdx.x;
  do {
    const int64_t m0 = group * G;                                        // the group's first member
    const int members = (int)(P - m0 < G ? P - m0 : G);                  // (the last group may be short)
    const int n = members * S;                                           // its pairs
    const int64_t row0 = m0 * S;                                         // pair 0 among all P * S
    u64 *cur = d0, *nxt = d1;
    // everything the frames read or add to is written here, for every group: nothing of the group
    // before it is left in LDS
    for (int i = tid; i < n; i += nt) {
      const int g = G == 1 ? 0 : i / S, s = i - g * S;
      uint32_t sum = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        sum += (uint32_t)g_counts[(row0 + i) * CAMPX_N_ACTIONS + a];
        cum[a * GS + i] = sum;
      }
      cur[i] = start ? start[(m0 + g) * vp.start_stride + s]
                     : (s == 0 ? (1ull << CAMPX_VISIT_FRAC_BITS) : 0ull);
      nxt[i] = 0;
    }
    for (int g = tid; g < 2 * G; g += nt) fin[g] = 0;
    __syncthreads();

    // the lane's pairs are i = tid + j * nt; with G > 1 there is one (n <= nt), with G = 1 they
    // are all member 0's: one member per lane either way, -1 for a lane without a pair
    const int mine = tid < n ? (G == 1 ? 0 : tid / S) : -1;
    u64 acc[kVisitPerLane][5];
#pragma unroll
    for (int j = 0; j < kVisitPerLane; ++j)
#pragma unroll
      for (int a = 0; a < 5; ++a) acc[j][a] = 0;

    for (int t = 0; t < vp.n_frames; ++t) {
      u64 over = 0;
#pragma unroll
      for (int j = 0; j < kVisitPerLane; ++j) {
        const int i = tid + j * nt;
        if (i < n) {
          const u64 m = cur[i];
          if (per_frame) per_frame[(int64_t)t * PS + row0 + i] = m;
          if (m) {
            cur[i] = 0;          // the target of frame t + 1: nobody else touches it in frame t
            const int s = i - mine * S;
            uint32_t c[4], e[5];
            u64 x[5];
#pragma unroll
            for (int a = 0; a < 4; ++a) c[a] = cum[a * GS + i];
#pragma unroll
            for (int a = 0; a < 5; ++a) e[a] = ent[a * S + s];
            split_mass(m, c, x);
#pragma unroll
            for (int a = 0; a < 5; ++a) {
              acc[j][a] += x[a];
              if (x[a]) {
                if (entry_done(e[a])) over += x[a];
                else lds_add(&nxt[mine * S + (int)entry_target(e[a], (uint32_t)S)], x[a]);
              }
            }
          }
        }
      }
      // a wave inside one member sums its ended mass first; one that holds several members goes
      // lane by lane, each lane to its own member (lane 0 holds the wave's lowest pair: where it
      // has none, no lane of the wave has, and `over` is 0)
      const int g0 = __shfl(mine, 0);
      if (__all(mine < 0 || mine == g0)) {
        over = wave_sum(over);
        if ((tid & 63) == 0 && over) {
          lds_add(&fin[(t & 1) * G + g0], over);
          if (vp.restart) lds_add(&nxt[g0 * S], over);
        }
      } else if (over) {
        lds_add(&fin[(t & 1) * G + mine], over);
        if (vp.restart) lds_add(&nxt[mine * S], over);
      }
      __syncthreads();             // d_{t+1} and finished[t] are complete; d_t is all zero
      for (int g = tid; g < members; g += nt) {
        finished[(int64_t)t * P + m0 + g] = fin[(t & 1) * G + g];
        fin[(t & 1) * G + g] = 0;  // (used again by frame t + 2, past the next barrier)
      }
      u64* swap = cur;
      cur = nxt;
      nxt = swap;
    }
    // `visits` lives in registers: written for every pair, with or without mass
#pragma unroll
    for (int j = 0; j < kVisitPerLane; ++j) {
      const int i = tid + j * nt;
      if (i < n) {
        const u64 m = cur[i];
        final_out[row0 + i] = m;
        if (per_frame) per_frame[(int64_t)vp.n_frames * PS + row0 + i] = m;
#pragma unroll
        for (int a = 0; a < 5; ++a) visits[(row0 + i) * CAMPX_N_ACTIONS + a] = acc[j][a];
      }
    }
    __syncthreads();               // the next group of this workgroup stages over these vectors
  } while ((group += gridDim.x) < vp.groups);
}

// One frame of all members.  `src`, `dst`, `visits`: [P][S]..., `finished_t`: [P], `row`:
// per_frame[t] = [P][S] or NULL.  A workgroup is 256 states of ONE member, so wave_sum() adds up
// one member's ended mass.  The grid never exceeds `blocks`.
__global__ __launch_bounds__(kVisitThreads) void visit_population_frame_kernel(
    int32_t S, int64_t blocks, int32_t restart, int32_t first, const uint2* __restrict__ entries,
    const int32_t* __restrict__ counts, u64* src, u64* dst, u64* __restrict__ visits,
    u64* __restrict__ finished_t, u64* __restrict__ row) {
  const int64_t per_member = (S + kVisitThreads - 1) / kVisitThreads;
  int64_t block = blockIdx.x;
  do {
    const int64_t member = block / per_member;
    const int s = (int)(block - member * per_member) * kVisitThreads + (int)threadIdx.x;
    const int64_t r = member * S + s;
    u64 over = 0;
    if (s < S) {
      const u64 m = src[r];
      if (row) row[r] = m;
      u64 x[5] = {0, 0, 0, 0, 0};
      if (m) {
        src[r] = 0;                // the target of the frame after next
        uint32_t n[4], word[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) word[a] = entries[s * CAMPX_N_ACTIONS + a].y;
        uint32_t sum = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          sum += (uint32_t)counts[r * CAMPX_N_ACTIONS + a];
          n[a] = sum;
        }
        split_mass(m, n, x);
#pragma unroll
        for (int a = 0; a < 5; ++a) {
          if (x[a]) {
            if (entry_done(word[a])) over += x[a];
            else global_add(&dst[member * S + entry_target(word[a], (uint32_t)S)], x[a]);
          }
        }
      }
      if (first) {
#pragma unroll
        for (int a = 0; a < 5; ++a) visits[r * CAMPX_N_ACTIONS + a] = x[a];
      } else if (m) {
#pragma unroll
        for (int a = 0; a < 5; ++a) visits[r * CAMPX_N_ACTIONS + a] += x[a];
      }
    }
    // every lane of the wave is here, block after block: the loop's bounds are the workgroup's
    over = wave_sum(over);
    if ((threadIdx.x & 63) == 0 && over) {
      global_add(finished_t + member, over);
      if (restart) global_add(&dst[member * S], over);
    }
  } while ((block += gridDim.x) < blocks);
}

// per_frame[n_frames] = d_T of every member, which the last frame left in `final`.
__global__ __launch_bounds__(kVisitThreads) void visit_population_last_row_kernel(
    int64_t n, const u64* __restrict__ final_in, u64* __restrict__ row) {
  const int64_t step = (int64_t)gridDim.x * kVisitThreads;
  for (int64_t i = (int64_t)blockIdx.x * kVisitThreads + threadIdx.x; i < n; i += step) row[i] = final_in[i];
}

// [a, a + na) and [b, b + nb) share a byte
inline bool spans_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// Compute units of the current device (256 where it cannot be asked): rule (c) of the plan.
inline int64_t visit_device_cus() {
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

int32_t campx_wide_visit_plan(int64_t n_states, int64_t wide_lds_max, int32_t path,
                              int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  VisitPlan p;
  return plan_visit(n_states, wide_lds_max, path, &p, plan_out);
}

int32_t campx_wide_visit_launch(const CampxWideSpec* s, const void* tables_dev, const float* policy,
                                const int64_t* start, int32_t restart, int32_t n_frames,
                                int64_t* visits, int64_t* finished, int64_t* final_mass,
                                int64_t* per_frame, int32_t* counts, int64_t* scratch,
                                int32_t* bad_rows, int32_t* bad_flag, int32_t path, void* stream) {
  if (!s || !tables_dev || !policy || !visits || !finished || !final_mass || !counts)
    return CAMPX_EINVAL;
  if (n_frames < 1 || n_frames > kVisitMaxFrames || (restart & ~1)) return CAMPX_EINVAL;
  if (!aligned_to(tables_dev, 8) || !aligned_to(policy, 4) || !aligned_to(start, 8) ||
      !aligned_to(visits, 8) || !aligned_to(finished, 8) || !aligned_to(final_mass, 8) ||
      !aligned_to(per_frame, 8) || !aligned_to(counts, 4) || !aligned_to(scratch, 8) ||
      !aligned_to(bad_rows, 4) || !aligned_to(bad_flag, 4))
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  const int64_t S = s->n_states;
  VisitPlan visit;
  const int32_t e = plan_visit(S, knob(K_WIDE_LDS_MAX), path, &visit, nullptr);
  if (e != CAMPX_OK) return e;
  const TablePlan& plan = visit.launch;
  const int64_t bytes = S * (int64_t)sizeof(int64_t);
  // the mass to start from and the mass to leave are one vector or two apart
  if (start && start != final_mass && ranges_overlap(start, final_mass, bytes)) return CAMPX_EINVAL;
  if (plan.path == 2 &&
      (!scratch || ranges_overlap(scratch, final_mass, bytes) ||
       (start && ranges_overlap(scratch, start, bytes))))
    return CAMPX_EINVAL;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint2* entries = wide_tables(*s, tables_dev).entries;
  const u64* d_start = reinterpret_cast<const u64*>(start);
  u64* d_visits = reinterpret_cast<u64*>(visits);
  u64* d_finished = reinterpret_cast<u64*>(finished);
  u64* d_final = reinterpret_cast<u64*>(final_mass);
  u64* d_rows = reinterpret_cast<u64*>(per_frame);
  u64* d_scratch = reinterpret_cast<u64*>(scratch);
  const dim3 per_state((unsigned)((S + kVisitThreads - 1) / kVisitThreads));
  // Frame k of n scatters into `final` when n - k is even and into the scratch vector when it is
  // odd, so that the last one leaves d_T in `final`; frame 1 reads the other of the two.
  u64* src = (n_frames & 1) ? d_scratch : d_final;
  u64* dst = (n_frames & 1) ? d_final : d_scratch;
  const bool global = plan.path == 2;
  hipLaunchKernelGGL(visit_counts_kernel, per_state, dim3(kVisitThreads), 0, hs, (int32_t)S, policy,
                     counts, d_start, global ? src : nullptr, global ? dst : nullptr, d_finished,
                     n_frames, bad_rows, bad_flag);
  const int32_t launched = launch_status();
  if (launched != CAMPX_OK) return launched;
  if (!global) {
    VisitParams vp;
    memset(&vp, 0, sizeof(vp));
    vp.S = (int32_t)S;
    vp.n_frames = n_frames;
    vp.restart = restart;
    vp.off_n = visit.off_n;
    vp.off_d0 = visit.off_d0;
    vp.off_d1 = visit.off_d1;
    CAMPX_ALLOW_LDS(visit_lds_kernel, (size_t)plan.lds_bytes);
    hipLaunchKernelGGL(visit_lds_kernel, dim3(1), dim3((unsigned)plan.threads),
                       (size_t)plan.lds_bytes, hs, vp, entries, counts, d_start, d_visits,
                       d_finished, d_final, d_rows);
    return launch_status();
  }
  for (int32_t k = 1; k <= n_frames; ++k) {
    hipLaunchKernelGGL(visit_frame_kernel, per_state, dim3(kVisitThreads), 0, hs, (int32_t)S, restart,
                       (int32_t)(k == 1), entries, counts, src, dst, d_visits, d_finished + (k - 1),
                       d_rows ? d_rows + (int64_t)(k - 1) * S : nullptr);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
    u64* swap = src;
    src = dst;
    dst = swap;
  }
  if (d_rows) {
    hipLaunchKernelGGL(visit_last_row_kernel, per_state, dim3(kVisitThreads), 0, hs, (int32_t)S,
                       d_final, d_rows + (int64_t)n_frames * S);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
  }
  return CAMPX_OK;
}

int32_t campx_wide_visit_population_plan(int64_t n_states, int64_t members, int64_t wide_lds_max,
                                         int64_t n_cus, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  VisitPopulationPlan p;
  const int32_t e = plan_visit_population(n_states, members, wide_lds_max, n_cus, path, &p);
  if (e == CAMPX_OK) {
    plan_out[0] = p.path;
    plan_out[1] = p.lds_bytes;
    plan_out[2] = p.threads;
    plan_out[3] = p.grid;
    plan_out[4] = p.G;
  }
  return e;
}

int32_t campx_wide_visit_population_launch(const CampxWideSpec* s, const void* tables_dev,
                                           const float* policies, int64_t members,
                                           const int64_t* start, int32_t start_per_member,
                                           int32_t restart, int32_t n_frames, int64_t* visits,
                                           int64_t* finished, int64_t* final_mass,
                                           int64_t* per_frame, int32_t* counts, int64_t* scratch,
                                           int32_t* bad_rows, int32_t* bad_flag, int32_t path,
                                           void* stream) {
  if (!s || !tables_dev || !policies || !visits || !finished || !final_mass || !counts)
    return CAMPX_EINVAL;
  if (members < 1 || n_frames < 1 || n_frames > kVisitMaxFrames || (restart & ~1) ||
      (start_per_member & ~1))
    return CAMPX_EINVAL;
  if (!aligned_to(tables_dev, 8) || !aligned_to(policies, 4) || !aligned_to(start, 8) ||
      !aligned_to(visits, 8) || !aligned_to(finished, 8) || !aligned_to(final_mass, 8) ||
      !aligned_to(per_frame, 8) || !aligned_to(counts, 4) || !aligned_to(scratch, 8) ||
      !aligned_to(bad_rows, 4) || !aligned_to(bad_flag, 4))
    return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  const int64_t S = s->n_states, P = members;
  if (P > kVisitMaxElements / (S * CAMPX_N_ACTIONS)) return CAMPX_EINVAL;
  // the path is host arithmetic alone; rule (c) is not, and only a path 1 of several members has it
  const int64_t lds_max = knob(K_WIDE_LDS_MAX);
  VisitPopulationPlan plan;
  int32_t e = plan_visit_population(S, P, lds_max, 1, path, &plan);
  if (e != CAMPX_OK) return e;
  const int64_t bytes = P * S * (int64_t)sizeof(int64_t);
  const int64_t start_bytes = start_per_member ? bytes : S * (int64_t)sizeof(int64_t);
  // a start per member and the mass to leave are one array or two apart; a shared start is read
  // by every member and overlaps nothing that is written
  if (start && !(start_per_member && start == final_mass) &&
      spans_overlap(start, start_bytes, final_mass, bytes))
    return CAMPX_EINVAL;
  if (plan.path == 2 &&
      (!scratch || ranges_overlap(scratch, final_mass, bytes) ||
       (start && spans_overlap(start, start_bytes, scratch, bytes))))
    return CAMPX_EINVAL;
  // (every refusal of an argument is decided above, before the device is asked anything)
  if (plan.path == 1 && P > 1) {
    e = plan_visit_population(S, P, lds_max, visit_device_cus(), path, &plan);
    if (e != CAMPX_OK) return e;
  }
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const uint2* entries = wide_tables(*s, tables_dev).entries;
  const u64* d_start = reinterpret_cast<const u64*>(start);
  u64* d_visits = reinterpret_cast<u64*>(visits);
  u64* d_finished = reinterpret_cast<u64*>(finished);
  u64* d_final = reinterpret_cast<u64*>(final_mass);
  u64* d_rows = reinterpret_cast<u64*>(per_frame);
  u64* d_scratch = reinterpret_cast<u64*>(scratch);
  const int64_t rows = P * S, stride = start_per_member ? S : 0;
  int64_t row_blocks = (rows + kVisitThreads - 1) / kVisitThreads;
  if (row_blocks > kVisitMaxGrid) row_blocks = kVisitMaxGrid;
  // as in campx_wide_visit_launch(): the last frame leaves d_T in `final`
  u64* src = (n_frames & 1) ? d_scratch : d_final;
  u64* dst = (n_frames & 1) ? d_final : d_scratch;
  const bool global = plan.path == 2;
  hipLaunchKernelGGL(visit_population_counts_kernel, dim3((unsigned)row_blocks), dim3(kVisitThreads), 0,
                     hs, (int32_t)S, rows, stride, policies, counts, d_start, global ? src : nullptr,
                     global ? dst : nullptr, d_finished, (int64_t)n_frames * P, bad_rows, bad_flag);
  const int32_t launched = launch_status();
  if (launched != CAMPX_OK) return launched;
  if (!global) {
    VisitPopulationParams vp;
    memset(&vp, 0, sizeof(vp));
    vp.S = (int32_t)S;
    vp.n_frames = n_frames;
    vp.restart = restart;
    vp.G = plan.G;
    vp.P = P;
    vp.groups = plan.groups;
    vp.start_stride = stride;
    vp.off_ent = plan.off_ent;
    vp.off_n = plan.off_n;
    vp.off_d0 = plan.off_d0;
    vp.off_d1 = plan.off_d1;
    CAMPX_ALLOW_LDS(visit_population_lds_kernel, (size_t)plan.lds_bytes);
    hipLaunchKernelGGL(visit_population_lds_kernel, dim3((unsigned)plan.grid),
                       dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, hs, vp, entries, counts,
                       d_start, d_visits, d_finished, d_final, d_rows);
    return launch_status();
  }
  for (int32_t k = 1; k <= n_frames; ++k) {
    hipLaunchKernelGGL(visit_population_frame_kernel, dim3((unsigned)plan.grid), dim3(kVisitThreads), 0,
                       hs, (int32_t)S, plan.groups, restart, (int32_t)(k == 1), entries, counts, src, dst,
                       d_visits, d_finished + (int64_t)(k - 1) * P,
                       d_rows ? d_rows + (int64_t)(k - 1) * rows : nullptr);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
    u64* swap = src;
    src = dst;
    dst = swap;
  }
  if (d_rows) {
    hipLaunchKernelGGL(visit_population_last_row_kernel, dim3((unsigned)row_blocks), dim3(kVisitThreads),
                       0, hs, rows, d_final, d_rows + (int64_t)n_frames * rows);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
  }
  return CAMPX_OK;
}

}  // extern "C"
