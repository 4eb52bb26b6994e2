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
// A population: member m of P is the rule above with policies[m] and its own start, and nothing
// else.  Members share the table and nothing they write, so - as in k_plan.hip - the only questions
// are where a member's vectors live and which lane takes which (member, state) pair, and since
// only integers are added neither can change a bit.  The kernels of the two paths are compiled
// with the members (kMembers) and without: one member, no division by S, no slot per member, one
// workgroup's one group.  One member takes the instances without, whichever call it came from.
//
// visit_counts_kernel   a lane per (member, state) row over all P * S rows: the bisection,
//     `counts`, the bad rows; on the global path also the two [P][S] mass buffers the first frame
//     starts from and the zeroes of finished[n_frames][P].  A shared start is read with member
//     stride 0.
// visit_lds_kernel      a workgroup stages the entries' next / done words [5][S] ONCE and takes G
//     consecutive members through ALL frames, one __syncthreads() per frame: per member N [4][S],
//     two mass vectors [S] and two slots of finished[t], FLAT over the pairs i = g * S + s.
//     Scatters are 64-bit LDS atomic adds; `visits` stays in the registers of the lane that owns
//     the pair.  G = 1: up to 1 024 lanes own up to kVisitPerLane states each; G > 1: the G * S <=
//     256 pairs are one to a lane.  A wave that holds pairs of several members (S < 64) hands its
//     ended mass out lane by lane, each to its own member's slot and state 0; a wave inside one
//     member sums it first.
// visit_frame_kernel    one launch per frame for ALL members, a lane per pair, a workgroup per 256
//     states of ONE member (so a wave never holds two), the blocks of all members along grid.x.
//     Scatters are no-return 64-bit global atomic adds; the mass that ends an episode is summed
//     across the wave first, so that finished[t] and state 0 take one atomic per wave; the lane
//     that reads d[s] clears it, so that the buffer is zero when it is the target of the frame
//     after next.
// Either grid stops at kVisitMaxGrid workgroups; a workgroup takes the groups (or blocks) that are
// a whole grid apart, one after the other.  plan_visit_population() chooses;
// campx_wide_visit_plan() and campx_wide_visit_population_plan() show the choice to a test without
// a GPU.

#include "wide_table.hip.h"

namespace campx_impl {

typedef unsigned long long u64;

constexpr int kVisitPerLane = 3;           // states a lane of the LDS workgroup owns, at most
constexpr int kVisitThreads = 256;         // global path, and the counts
constexpr int64_t kVisitLdsHeader = 64;    // the two slots of finished[t] of the first member
constexpr int64_t kVisitMemberHeader = 16; // those of each further member
constexpr int32_t kVisitMaxFrames = 1 << 20;
constexpr uint32_t kVisitWords = 1u << 24; // the sampler's values u
constexpr int64_t kVisitMaxGrid = 1 << 20;
constexpr int64_t kVisitMaxElements = 0x7fffffff;    // P * S * 5, the elements of `policies`
constexpr int64_t kVisitPackThreads = 256;           // pairs a workgroup is packed up to

struct VisitPopulationPlan {
  int32_t path, threads, G;
  int64_t grid, lds_bytes, groups;   // groups: of G members (path 1) / blocks of 256 states (path 2)
  int32_t off_ent, off_n, off_d0, off_d1;            // byte offsets into the dynamic LDS
};

// The LDS G members of S states take: the header, which has the first member's two slots of
// finished[t], and 16 bytes for those of each further member; the entries' second words [5][S] x
// 4 bytes once; per member N [4][S] x 4 bytes and two mass vectors [S] x 8 bytes, flat over the
// G * S pairs - 20 bytes per state and 32 per pair.  A lane keeps the visits of the pairs it owns
// in registers, kVisitPerLane of them at most.
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

// The plan of P members (a single policy is P = 1 on one compute unit).  Path 1 whenever one
// member fits lds_max and a lane's kVisitPerLane states; how many members a workgroup of it takes
// is members_per_workgroup()'s rule (wide_table.hip.h).
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
    const int64_t G = members_per_workgroup(S, P, n_cus, lds_max, kVisitPackThreads, [&](int64_t g) {
      return visit_population_lds(S, g, nullptr);
    });
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

// The words both _plan() entry points show: path, LDS bytes, threads, grid.
inline void plan_words(const VisitPopulationPlan& p, int64_t* plan_out) {
  plan_out[0] = p.path;
  plan_out[1] = p.lds_bytes;
  plan_out[2] = p.threads;
  plan_out[3] = p.grid;
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

// `counts` and the bad rows of all `rows` = P * S rows; with `d_first` (global path) also the mass
// the first frame reads - `start`, or one environment in state 0 -, zeroes where it scatters to,
// and the zeroes of the `n_finished` = n_frames * P slots of `finished`.  Row r = m * S + s reads
// start[m * start_stride + s] before it writes element r of either buffer, and touches no other,
// so a start per member may be either buffer.
__global__ __launch_bounds__(kVisitThreads) void visit_counts_kernel(
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

struct VisitPopulationParams {
  int32_t S, n_frames, restart, G;
  int64_t P, groups;
  int64_t start_stride;              // S: a start per member; 0: one start shared by all
  int32_t off_ent, off_n, off_d0, off_d1;
};

// `finished` is [n_frames][P], `per_frame` [n_frames + 1][P][S]; everything else is a member's
// own, [P][...].  The grid never exceeds vp.groups, so a workgroup's first group is its own index;
// without members there is one group of one member, the launch's one workgroup's.
template <bool kMembers>
__global__ __launch_bounds__(kTableLdsThreads) void visit_lds_kernel(
    VisitPopulationParams vp, const uint2* __restrict__ g_entries, const int32_t* __restrict__ g_counts,
    const u64* start, u64* __restrict__ visits, u64* __restrict__ finished, u64* final_out,
    u64* __restrict__ per_frame) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_visit[];
  u64* fin = reinterpret_cast<u64*>(lds_visit);                          // [2][G]: frame t uses t & 1
  uint32_t* ent =                                                        // [5][S]
      reinterpret_cast<uint32_t*>(lds_visit + (kMembers ? (int64_t)vp.off_ent : kVisitLdsHeader));
  uint32_t* cum = reinterpret_cast<uint32_t*>(lds_visit + vp.off_n);     // [4][G * S]
  u64* d0 = reinterpret_cast<u64*>(lds_visit + vp.off_d0);               // [G * S]
  u64* d1 = reinterpret_cast<u64*>(lds_visit + vp.off_d1);
  const int S = vp.S, G = kMembers ? vp.G : 1, GS = G * S, nt = (int)blockDim.x, tid = (int)threadIdx.x;
  const int64_t P = kMembers ? vp.P : 1, PS = P * S;
  for (int i = tid; i < S * CAMPX_N_ACTIONS; i += nt) {
    const int s = i / CAMPX_N_ACTIONS, a = i - s * CAMPX_N_ACTIONS;
    ent[a * S + s] = g_entries[i].y;
  }

  int64_t group = kMembers ? blockIdx.x : 0;
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
    const int base = kMembers ? mine * S : 0;                            // the member's pair 0
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
            const int s = i - base;
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
                else lds_add(&nxt[base + (int)entry_target(e[a], (uint32_t)S)], x[a]);
              }
            }
          }
        }
      }
      // every lane of the workgroup is here.  A wave inside one member sums its ended mass first;
      // one that holds several members goes lane by lane, each lane to its own member (lane 0
      // holds the wave's lowest pair: where it has none, no lane of the wave has, and `over` is 0)
      const int g0 = kMembers ? __shfl(mine, 0) : 0;
      if (!kMembers || __all(mine < 0 || mine == g0)) {
        over = wave_sum(over);
        if ((tid & 63) == 0 && over) {
          lds_add(&fin[(t & 1) * G + g0], over);
          if (vp.restart) lds_add(&nxt[g0 * S], over);
        }
      } else if (over) {
        lds_add(&fin[(t & 1) * G + mine], over);
        if (vp.restart) lds_add(&nxt[base], over);
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
    if (kMembers) __syncthreads();   // the next group of this workgroup stages over these vectors
  } while (kMembers && (group += gridDim.x) < vp.groups);
}

// One frame of all members.  `src` is d_t and is left all zero, `dst` - zero when the launch
// starts, but for what the workgroups of this launch have added - becomes d_{t+1}; both and
// `visits` are [P][S]..., `finished_t` is [P].  `first`: visits are written, not added to.  `row`:
// per_frame[t] = [P][S], or NULL.  A workgroup is 256 states of ONE member, so wave_sum() adds up
// one member's ended mass.  The grid never exceeds `blocks`; without members it is the blocks of
// the one member, each its workgroup's only one.
template <bool kMembers>
__global__ __launch_bounds__(kVisitThreads) void visit_frame_kernel(
    int32_t S, int64_t blocks, int32_t restart, int32_t first, const uint2* __restrict__ entries,
    const int32_t* __restrict__ counts, u64* src, u64* dst, u64* __restrict__ visits,
    u64* __restrict__ finished_t, u64* __restrict__ row) {
  const int64_t per_member = (S + kVisitThreads - 1) / kVisitThreads;
  int64_t block = blockIdx.x;
  do {
    const int64_t member = kMembers ? block / per_member : 0;
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
  } while (kMembers && (block += gridDim.x) < blocks);
}

// per_frame[n_frames] = d_T of every member, which the last frame left in `final`.
__global__ __launch_bounds__(kVisitThreads) void visit_last_row_kernel(
    int64_t n, const u64* __restrict__ final_in, u64* __restrict__ row) {
  const int64_t step = (int64_t)gridDim.x * kVisitThreads;
  for (int64_t i = (int64_t)blockIdx.x * kVisitThreads + threadIdx.x; i < n; i += step) row[i] = final_in[i];
}

// Both entry points, their own NULL checks behind them: `members` policies, each from its own
// `start` row (`start_per_member`; campx_wide_visit_launch()'s one start is its one member's) or
// all from one shared [S].  One member takes the instances compiled without members from either
// entry point - a shared start is then read at member 0, where the stride is moot.
static int32_t visit_launch(const CampxWideSpec* s, const void* tables_dev, const float* policies,
                            int64_t members, const int64_t* start, int32_t start_per_member,
                            int32_t restart, int32_t n_frames, int64_t* visits, int64_t* finished,
                            int64_t* final_mass, int64_t* per_frame, int32_t* counts, int64_t* scratch,
                            int32_t* bad_rows, int32_t* bad_flag, int32_t path, void* stream) {
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
  // by every member; neither overlaps anything else that is written
  const auto start_overlaps = [&](const void* written, bool may_be) {
    return start && !(may_be && start == written) && spans_overlap(start, start_bytes, written, bytes);
  };
  if (start_overlaps(final_mass, start_per_member)) return CAMPX_EINVAL;
  if (plan.path == 2 &&
      (!scratch || ranges_overlap(scratch, final_mass, bytes) || start_overlaps(scratch, false)))
    return CAMPX_EINVAL;
  // (every refusal of an argument is decided above, before the device is asked anything)
  if (plan.path == 1 && P > 1) {
    e = plan_visit_population(S, P, lds_max, device_cus(), path, &plan);
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
  // Frame k of n scatters into `final` when n - k is even and into the scratch array when it is
  // odd, so that the last one leaves d_T in `final`; frame 1 reads the other of the two.
  u64* src = (n_frames & 1) ? d_scratch : d_final;
  u64* dst = (n_frames & 1) ? d_final : d_scratch;
  const bool global = plan.path == 2, solo = P == 1;
  hipLaunchKernelGGL(visit_counts_kernel, dim3((unsigned)row_blocks), dim3(kVisitThreads), 0, hs,
                     (int32_t)S, rows, stride, policies, counts, d_start, global ? src : nullptr,
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
    const auto kernel = solo ? visit_lds_kernel<false> : visit_lds_kernel<true>;
    CAMPX_ALLOW_LDS(kernel, (size_t)plan.lds_bytes);
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.grid), dim3((unsigned)plan.threads),
                       (size_t)plan.lds_bytes, hs, vp, entries, counts, d_start, d_visits, d_finished,
                       d_final, d_rows);
    return launch_status();
  }
  const auto frame = solo ? visit_frame_kernel<false> : visit_frame_kernel<true>;
  for (int32_t k = 1; k <= n_frames; ++k) {
    hipLaunchKernelGGL(frame, dim3((unsigned)plan.grid), dim3(kVisitThreads), 0, hs, (int32_t)S,
                       plan.groups, restart, (int32_t)(k == 1), entries, counts, src, dst, d_visits,
                       d_finished + (int64_t)(k - 1) * P,
                       d_rows ? d_rows + (int64_t)(k - 1) * rows : nullptr);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
    u64* swap = src;
    src = dst;
    dst = swap;
  }
  if (d_rows) {
    hipLaunchKernelGGL(visit_last_row_kernel, dim3((unsigned)row_blocks), dim3(kVisitThreads), 0, hs,
                       rows, d_final, d_rows + (int64_t)n_frames * rows);
    return launch_status();
  }
  return CAMPX_OK;
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_visit_plan(int64_t n_states, int64_t wide_lds_max, int32_t path,
                              int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  VisitPopulationPlan p;
  const int32_t e = plan_visit_population(n_states, 1, wide_lds_max, 1, path, &p);
  if (e == CAMPX_OK) plan_words(p, plan_out);
  return e;
}

int32_t campx_wide_visit_launch(const CampxWideSpec* s, const void* tables_dev, const float* policy,
                                const int64_t* start, int32_t restart, int32_t n_frames,
                                int64_t* visits, int64_t* finished, int64_t* final_mass,
                                int64_t* per_frame, int32_t* counts, int64_t* scratch,
                                int32_t* bad_rows, int32_t* bad_flag, int32_t path, void* stream) {
  if (!s || !tables_dev || !policy || !visits || !finished || !final_mass || !counts)
    return CAMPX_EINVAL;
  return visit_launch(s, tables_dev, policy, 1, start, 1, restart, n_frames, visits, finished,
                      final_mass, per_frame, counts, scratch, bad_rows, bad_flag, path, stream);
}

int32_t campx_wide_visit_population_plan(int64_t n_states, int64_t members, int64_t wide_lds_max,
                                         int64_t n_cus, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  VisitPopulationPlan p;
  const int32_t e = plan_visit_population(n_states, members, wide_lds_max, n_cus, path, &p);
  if (e == CAMPX_OK) {
    plan_words(p, plan_out);
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
  return visit_launch(s, tables_dev, policies, members, start, start_per_member, restart, n_frames,
                      visits, finished, final_mass, per_frame, counts, scratch, bad_rows, bad_flag,
                      path, stream);
}

}  // extern "C"
