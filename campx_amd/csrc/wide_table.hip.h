// wide_table.hip.h - what the kernels of the state-table tier (k_wide, k_policy, k_learn,
// k_plan, k_visit, k_states, k_window) and their launchers agree on, each said once: the
// table entry's format, the policy-row rule, the sampler's Philox block, the lazy error report -
// and, host side, the table blob's layout and the view a launcher takes of it, the discount list,
// the choice between one LDS workgroup and one launch per step, and how many members of a
// population a workgroup takes.
#ifndef CAMPX_WIDE_TABLE_HIP_H_
#define CAMPX_WIDE_TABLE_HIP_H_

#include "campx_common.hip.h"

#include <math.h>

namespace campx_impl {

// Table-blob entry of (state, action), 8 bytes: x = the reward's bits; y = [0:23] the state after
// the frame, [24] done, [25:28] discount code.  (The state the NEXT frame starts from is state 0
// when the frame ended the episode: the rebuild is one select on the chain.)  The accessors take
// the y word; campx_amd/_hip.py names the same masks and shifts for table_arrays().
__host__ __device__ __forceinline__ uint32_t wide_pack(uint32_t next, uint32_t done, uint32_t dcode) {
  return next | (done << 24) | (dcode << 25);
}
__device__ __forceinline__ uint32_t entry_next(uint32_t y) { return y & 0xffffffu; }
__device__ __forceinline__ uint32_t entry_done(uint32_t y) { return (y >> 24) & 1u; }
__device__ __forceinline__ uint32_t entry_dcode(uint32_t y) { return (y >> 25) & 15u; }
// Where an entry leads.  (A next state outside the table cannot come out of
// campx_wide_tables_build(); it stands for state 0 rather than for an element past a vector.)
__device__ __forceinline__ uint32_t entry_target(uint32_t y, uint32_t S) {
  const uint32_t next = entry_next(y);
  return next < S ? next : 0u;
}

// The test of a policy row, given its total c4 in the sampler's f32 order: no weight negative or
// NaN, the total a positive finite number.  A macro, not a function: the two readers below must
// compile to the code they had when each spelled the test out, and hipcc gives the && chain another
// shape (no branch round the sum, other registers) once it comes through a call, inlined or not.
#define CAMPX_POLICY_ROW_GOOD(w0, w1, w2, w3, w4, c4)                                            \
  ((w0) >= 0.0f && (w1) >= 0.0f && (w2) >= 0.0f && (w3) >= 0.0f && (w4) >= 0.0f && (c4) > 0.0f && \
   (c4) < INFINITY)

// A policy row's thresholds, in the sampler's f32 order.  A bad row becomes {-1, -1, -1, -1, 0}:
// r = u * 0 = 0 passes all four tests - action 4 - and c4 == 0, which no good row has, is what
// counts as bad.
__device__ __forceinline__ void policy_thresholds(const float* w, float (&c)[5]) {
  const float w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
  c[0] = w0;
  c[1] = c[0] + w1;
  c[2] = c[1] + w2;
  c[3] = c[2] + w3;
  c[4] = c[3] + w4;
  const bool good = CAMPX_POLICY_ROW_GOOD(w0, w1, w2, w3, w4, c[4]);
  if (!good) {
    c[0] = c[1] = c[2] = c[3] = -1.0f;
    c[4] = 0.0f;
  }
}

// c[4] of policy_thresholds() alone, for a reader that needs no threshold (k_plan.hip): the row's
// total - the same sum in the same order - or 0 for a bad row.
__device__ __forceinline__ float policy_row_total(const float (&w)[5]) {
  const float c4 = (((w[0] + w[1]) + w[2]) + w[3]) + w[4];
  const bool good = CAMPX_POLICY_ROW_GOOD(w[0], w[1], w[2], w[3], w[4], c4);
  return good ? c4 : 0.0f;
}

// A row of PREFERENCES h[0..4] as the sampler's weights w[0..4]: the softmax's numerators by the
// exponent rule of include/campx_hip.h ("Actor-critic online learners", rule 1) - NOT expf(): every
// operation below is one f32 operation rounded on its own (-ffp-contract=off), so that numpy and
// torch restate it bit for bit.  m is the row's maximum by the greedy reduction (the lowest index
// wins ties, NaN never wins); the row is good when (m - m) == 0 and no element is above m or NaN;
// w = 2^k * p(f) with t = (h - m) * log2e, k = rint(t), f = t - k, p the degree-6 polynomial of
// 2^f, and w = +0 for t < -100.  The maximum's weight is exactly 1: c4 lies in [1, 5].  A row that
// is not good gets five zeros - policy_thresholds() then calls it bad - and `false` is returned.
constexpr float kSoftmaxLog2e = 0x1.715476p+0f;
constexpr float kSoftmaxCut = -100.0f;
constexpr float kSoftmaxPoly[7] = {0x1p+0f,         0x1.62e43p-1f,   0x1.ebfbep-3f,  0x1.c6b08ep-5f,
                                   0x1.3b2ab6p-7f,  0x1.5d87fep-10f, 0x1.430912p-13f};
__device__ __forceinline__ bool softmax_weights(const float (&h)[5], float (&w)[5]) {
  float m = h[0];
#pragma unroll
  for (int a = 1; a < 5; ++a) m = h[a] > m ? h[a] : m;
  bool good = (m - m) == 0.0f;
#pragma unroll
  for (int a = 0; a < 5; ++a) good = good && h[a] <= m;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    const float t = (h[a] - m) * kSoftmaxLog2e;
    const bool some = good && t >= kSoftmaxCut;
    const float tt = some ? t : 0.0f;                  // (k stays within -100 .. 0)
    const float k = rintf(tt);                         // ties to even
    const float f = tt - k;
    float p = kSoftmaxPoly[6];
#pragma unroll
    for (int n = 5; n >= 0; --n) p = p * f + kSoftmaxPoly[n];
    // 2^k as a float, k in -100 .. 0: the product is exact, no result is subnormal
    const float scale = __uint_as_float((uint32_t)((int)k + 127) << 23);
    w[a] = some ? p * scale : 0.0f;
  }
  return good;
}

// One Philox4x32-10 block: the sampler of the closed-loop rollouts (k_policy.hip;
// include/campx_hip.h has the rule).
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// What a kernel found wrong in its input and went on from, for the host to read later: `n` more on
// the device counter, and the pinned flag raised (either may be NULL).
__device__ __forceinline__ void report_bad(int32_t* count, int32_t* flag, int n) {
  if (n) {
    if (count) atomicAdd(count, n);
    if (flag) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---------------------------------------------------------------------------- host side

inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// [a, a + bytes) and [b, b + bytes) share a byte
inline bool ranges_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  const uintptr_t n = (uintptr_t)bytes;
  return x < y ? y - x < n : x - y < n;
}

// [a, a + na) and [b, b + nb) share a byte
inline bool spans_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// Compute units of the current device (256 where it cannot be asked): rule (c) below.
inline int64_t device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  return cus;
}

// Where the parts of the state-table blob are: [entries uint2 x 5S, padded to 16][cells 8 x uint16
// x S][perf int8 x 5S, padded to 16][rot_obs][rot_board][pieces: 16 words for the layered rows, 16
// for the flat board].  wide_layout() (k_wide.hip) is the one place that computes the offsets;
// campx_wide_tables_build() fills a blob by them and wide_tables() below reads one.
struct WideLayout {
  int64_t n_entries, cells_off, perf_off, rot_obs_off, rot_board_off, pieces_off, total;
  int pitch_obs, pitch_board;
  int n_variants;          // sets of rotations (1: the scenery never changes)
  int n_planes;            // planes of the trace: the things, plus the variant's when there are several,
                           // or the mask of the pieces that show
};
WideLayout wide_layout(const CampxWideSpec& s);

// A blob on the device as its launchers read it: the layout and a typed pointer to each part.
struct WideTables {
  WideLayout lay;
  const uint2* entries;
  const u32x4* cells;
  const int8_t* perf;
  const int8_t *rot_obs, *rot_board;            // variant v's rotations start v * 16 * pitch bytes on
  const uint32_t *pieces_obs, *pieces_board;    // NULL for a scenery without pieces
};
inline WideTables wide_tables(const CampxWideSpec& s, const void* tables_dev) {
  WideTables t;
  t.lay = wide_layout(s);
  const char* blob = static_cast<const char*>(tables_dev);
  t.entries = reinterpret_cast<const uint2*>(blob);
  t.cells = reinterpret_cast<const u32x4*>(blob + t.lay.cells_off);
  t.perf = reinterpret_cast<const int8_t*>(blob + t.lay.perf_off);
  t.rot_obs = reinterpret_cast<const int8_t*>(blob + t.lay.rot_obs_off);
  t.rot_board = reinterpret_cast<const int8_t*>(blob + t.lay.rot_board_off);
  t.pieces_obs = s.n_pieces > 0 ? reinterpret_cast<const uint32_t*>(blob + t.lay.pieces_off) : nullptr;
  t.pieces_board = s.n_pieces > 0 ? t.pieces_obs + CAMPX_WIDE_MAX_PIECES : nullptr;
  return t;
}

// The discount a kernel reports for each code of an entry: code 0 has none of its own (slot 0
// is 1), codes 1 .. 15 are the game's list.
inline void wide_discounts(const CampxWideSpec& s, float (&discounts)[16]) {
  discounts[0] = 1.0f;
  for (int i = 1; i < 16; ++i) discounts[i] = s.discount_list[i];
}

// Work that runs n steps over a table's S states, a lane per state, each step reading what the one
// before it wrote: ONE workgroup that keeps everything in LDS and runs all steps, a barrier between
// them (path 1) - or one launch per step (path 2).
// threads of the LDS workgroup, at most; it has a multiple of 64 that covers the states
constexpr int kTableLdsThreads = 1024;
struct TablePlan {
  int32_t path;            // 1 LDS, 2 global
  int32_t threads;         // of a workgroup
  int64_t grid;            // workgroups of a step
  int64_t lds_bytes;
};

// S is within 1 .. CAMPX_WIDE_MAX_STATES (the caller's byte arithmetic needed that already).
// `lds_bytes`: what the LDS workgroup would take; it is chosen (`path` 0) or allowed (`path` 1)
// when that is within `lds_max` and `fits_too` holds.  `plan_out`: the four words the
// campx_wide_*_plan() entry points show, or NULL.
inline int32_t plan_lds_or_launch(int64_t S, int64_t lds_bytes, bool fits_too, int64_t lds_max,
                                  int32_t path, int32_t global_threads, TablePlan* p,
                                  int64_t* plan_out) {
  if (lds_max < 0 || path < 0 || path > 2) return CAMPX_EINVAL;
  const bool fits = lds_bytes <= lds_max && fits_too;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  if (path == 1 || (path == 0 && fits)) {
    p->path = 1;
    const int64_t t = (S + 63) / 64 * 64;
    p->threads = (int32_t)(t > kTableLdsThreads ? kTableLdsThreads : t);
    p->grid = 1;
    p->lds_bytes = lds_bytes;
  } else {
    p->path = 2;
    p->threads = global_threads;
    p->grid = (S + global_threads - 1) / global_threads;
    p->lds_bytes = 0;
  }
  if (plan_out) {
    plan_out[0] = p->path;
    plan_out[1] = p->lds_bytes;
    plan_out[2] = p->threads;
    plan_out[3] = p->grid;
  }
  return CAMPX_OK;
}

// The same work for a population of P members that share the table (k_plan.hip, k_visit.hip): how
// many members G a workgroup of the LDS path takes - the least of
//   (a) what fits lds_max (`lds_of(G)`: the LDS bytes of G members; one member fits);
//   (b) floor(pack / S), at least 1: members are packed until the workgroup has about four waves
//       of (member, state) pairs (pack = 256), no further;
//   (c) ceil(P / n_cus): a population smaller than G * n_cus would leave CUs idle, so it is spread
//       one workgroup per CU first and packed only beyond that.
// (b) is not the rule this started from, ceil(kTableLdsThreads / S) - pack until every one of the
// workgroup's 1 024 threads has a pair.  One run of k_plan.hip's sweeps on an MI355X at P = 65 536,
// 64 sweeps, G bounded through (a) (NOTES.md has the table): the maze's 159 states 5.77 ms at G = 7
// (1 113 pairs: a second round for 89 of them), 5.32 at 6, 3.71 at 3, 3.40 at G = 1; the boat race's
// 8 states 0.226 ms at G = 128 (1 024 threads), 0.185-0.199 from 64 down to 8, 0.319 at 4 and 1.15
// at G = 1, where most of a wave idles.  Several small workgroups to a CU beat one large one, and a
// part-filled wave costs more than either: 256 threads is the size that is best or within a tenth
// of it at both, and a floor keeps a table of up to 256 states to one pair per thread.  Two sizes,
// one run: a choice with a reason, not a tuned one.  (c) has not been measured at all, and the
// visitation takes the rule over as it stands, NOT tuned for its kernel.
template <class LdsOf>
inline int64_t members_per_workgroup(int64_t S, int64_t P, int64_t n_cus, int64_t lds_max,
                                     int64_t pack, LdsOf lds_of) {
  int64_t G = pack / S;                                               // (b)
  if (G < 1) G = 1;
  const int64_t spread = (P + n_cus - 1) / n_cus;                     // (c)
  if (spread < G) G = spread;
  if (lds_of(G) > lds_max) {                                          // (a): the largest that fits
    int64_t lo = 1, hi = G - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (lds_of(mid) <= lds_max) lo = mid;
      else hi = mid - 1;
    }
    G = lo;
  }
  return G;
}

}  // namespace campx_impl

#endif  // CAMPX_WIDE_TABLE_HIP_H_
