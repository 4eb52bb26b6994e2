// k_vtrace.hip - V-trace targets and advantages of a rollout's [T, B] streams: the off-policy
// correction of a learner whose data was sampled by other policies, one backward pass in one
// launch, aware of the episode ends INSIDE the rollout and of NaN rewards like returns_kernel.
//
// The rule (include/campx_hip.h has it in full; tests/vtrace_reference.py restates it in numpy):
// for t = T-1 down to 0, per environment, every operation an f32 operation rounded on its own
//     r = isnan(reward) ? 0 : reward          c = gamma * discount     (gamma without a discount)
//     w0 = ratio                              or   target[(s % Nt) * A + a] / behaviour[s * A + a]
//     w = w0 > 0 ? w0 : +0        rho, cs, rpg = w clipped from above at rho_bar, c_bar, pg_rho_bar
//     delta = rho * ((done ? r : r + c * v_next) - v)
//     D = done ? delta : delta + ((c * lam) * cs) * D_next
//     vs = v + D                  adv = rpg * ((done ? r : r + c * vs_next) - v)
//
// A lane per environment walks its column backwards in chunks of eight frames (streams.hip.h:
// walk_back() and its Chunk, the head of the rule, the id test, table staging, the counters), a
// chunk issues ALL its loads - coalesced along B - before its arithmetic, and everything that does
// not depend on the frame after (r, c, w, the three clips, delta, the factor of D_next) is
// computed off the chain, which stays one multiply and one add per frame (D).  vs and adv hang
// off it and feed nothing back.  Stores are plain: the learner reads them next.
//
// Table mode: the ratio is a function of (state, action) on two small tables, so it is looked up
// and divided here instead of being written as a stream (two lookups, a division: three launches
// and 12 bytes per environment-frame).  The sixteen gathers of a chunk depend on its index loads
// and on nothing else; they are issued together, behind the index loads and before any
// arithmetic.  A frame whose ids are out of range forms no address from them: its gathers are
// not executed, its w is 0 and it is counted.  Two places for the tables: both staged in LDS once
// per workgroup (path 1) or read through L1 / L2 (path 2); plan_vtrace() chooses by
// table_staged() and campx_vtrace_plan() shows the choice to a test without a GPU.

#include "streams.hip.h"

#include <cmath>

namespace campx_impl {

enum VtraceMode : int { kVtraceRatio = 0, kVtraceLds = 1, kVtraceGlobal = 2 };

struct VtracePlan {
  int32_t path;            // 0 ratio mode (no tables), 1 LDS, 2 global
  int64_t lds_bytes;
  int64_t grid;
};

// Where the tables of a launch live: table_staged()'s rule for both tables together, a workgroup
// looking up all T frames.
inline int32_t plan_vtrace(int64_t Nt, int64_t Nb, int32_t A, int64_t B, int32_t T, int32_t path,
                           VtracePlan* p) {
  if (Nt < 1 || Nb < Nt || Nb > 0x7fffffffll || Nb % Nt != 0 || A < 1 || A > 128 ||
      !stream_shape_ok(B, T) || path < 0 || path > 2)
    return CAMPX_EINVAL;
  const int64_t entries = (Nt + Nb) * A;                   // <= 2^32 * 128
  if (path == 1 && !table_fits_lds(entries)) return CAMPX_EINVAL;
  const bool lds = path == 1 || (path == 0 && table_staged(entries, T));
  p->path = lds ? 1 : 2;
  p->lds_bytes = lds ? entries * 4 : 0;
  p->grid = stream_blocks(B);
  return CAMPX_OK;
}

// n / d for every n below 2^31 as (n * m) >> shift in 64 bits (Granlund and Montgomery 1994, the
// round-up multiplier for 31-bit numerators): l = ceil(log2(d)), m = ceil(2^(31 + l) / d) < 2^32.
inline void vtrace_modulus(uint32_t d, uint32_t* m, uint32_t* shift) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  *shift = 31 + l;
  *m = (uint32_t)(((1ull << *shift) + d - 1) / d);
}

struct VtraceParams {
  float gamma, lam, rho_bar, c_bar, pg_rho_bar;
  int32_t T;
  int64_t B;
  uint32_t Nt, Nb, A;
  uint32_t mod_m, mod_shift;     // vtrace_modulus(Nt)
  // elements from one frame's row to the next, per stream
  int64_t p_reward, p_done, p_discount, p_values, p_ratio, p_states, p_actions, p_vs, p_adv;
};

template <bool kDiscount, int kMode>
__global__ __launch_bounds__(kStreamThreads) void vtrace_kernel(
    VtraceParams vp, const float* __restrict__ reward, const uint8_t* __restrict__ done,
    const float* __restrict__ discount, const float* __restrict__ values,
    const float* __restrict__ bootstrap, const float* __restrict__ ratio,
    const float* __restrict__ target, const float* __restrict__ behaviour,
    const int32_t* __restrict__ states, const int8_t* __restrict__ actions,
    float* __restrict__ vs_out, float* __restrict__ adv_out, u64* __restrict__ bad_count) {
  constexpr bool kTable = kMode != kVtraceRatio;
  constexpr bool kLds = kMode == kVtraceLds;
  extern __shared__ __align__(16) float lds_tables[];       // kLds: target [Nt * A], behaviour [Nb * A]
  __shared__ u64 counters[2];                               // [0]: the frames with a bad id
  const int tid = threadIdx.x;
  const uint32_t n_target = vp.Nt * vp.A;                   // (fits 32 bits whenever it is used)
  if (kLds) {
    stage_table(lds_tables, target, n_target);
    stage_table(lds_tables + n_target, behaviour, vp.Nb * vp.A);
  }
  if (kTable) {
    if (tid < 2) counters[tid] = 0;
    __syncthreads();
  }
  const int64_t env = (int64_t)blockIdx.x * kStreamThreads + tid;
  u64 n_bad = 0;
  if (env < vp.B) {
    const float boot = bootstrap ? bootstrap[env] : 0.0f;
    const float gamma = vp.gamma, lam = vp.lam;
    const float rho_bar = vp.rho_bar, c_bar = vp.c_bar, pg_rho_bar = vp.pg_rho_bar;
    float D = 0.0f, v_after = boot, vs_after = boot;        // of the frame after the one in hand
    walk_back(vp.T, [&](auto chunk) {
      float r[kStreamChunk], c[kStreamChunk], v[kStreamChunk], w[kStreamChunk];
      uint8_t d[kStreamChunk];
      int32_t s[kStreamChunk];
      int8_t a[kStreamChunk];
      // the index loads first: the gathers wait for them alone (the wait counter is in order)
      if (kTable) {
#pragma unroll
        for (int j = 0; j < kStreamChunk; ++j) {
          s[j] = states[chunk.load_t(j) * vp.p_states + env];
          a[j] = actions[chunk.load_t(j) * vp.p_actions + env];
        }
      }
#pragma unroll
      for (int j = 0; j < kStreamChunk; ++j) {
        const int64_t t = chunk.load_t(j);
        if (!kTable) w[j] = ratio[t * vp.p_ratio + env];
        r[j] = reward[t * vp.p_reward + env];
        d[j] = done[t * vp.p_done + env];
        c[j] = kDiscount ? discount[t * vp.p_discount + env] : 1.0f;
        v[j] = values[t * vp.p_values + env];
      }
      // (the scheduler otherwise pulls each index load and its range check to the front, waits
      // for them one by one, and issues the rest of the chunk's loads behind that)
      __builtin_amdgcn_sched_barrier(0);
      if (kTable) {
        // the sixteen gathers, before any arithmetic; an id out of range forms no address
        float tg[kStreamChunk], bh[kStreamChunk];
        bool ok[kStreamChunk], all_ok = true;
#pragma unroll
        for (int j = 0; j < kStreamChunk; ++j) {
          ok[j] = ids_in_range(s[j], a[j], vp.Nb, vp.A);
          all_ok = all_ok & ok[j];
        }
        auto gather = [&](int j) {
          const uint32_t state = (uint32_t)s[j];
          // state % Nt for a state below 2^31, by the multiplier of the launch (vtrace_modulus())
          const uint32_t member_state = state - (uint32_t)(((uint64_t)state * vp.mod_m) >> vp.mod_shift) * vp.Nt;
          if (kLds) {
            tg[j] = lds_tables[bin_of<uint32_t>(member_state, a[j], vp.A)];
            bh[j] = lds_tables[n_target + bin_of<uint32_t>(s[j], a[j], vp.A)];
          } else {
            tg[j] = target[bin_of<int64_t>(member_state, a[j], vp.A)];
            bh[j] = behaviour[bin_of<int64_t>(s[j], a[j], vp.A)];
          }
        };
        // A wave whose chunk holds no bad id - every wave of a sound rollout - issues the sixteen
        // back to back.  Loads under a per-lane condition are loads the wait counters cannot
        // count on, so each waits for the one before: only a wave that met a bad id takes them,
        // a frame at a time, and finishes with them before it goes on.
        if (__all(all_ok)) {
#pragma unroll
          for (int j = 0; j < kStreamChunk; ++j) gather(j);
#pragma unroll
          for (int j = 0; j < kStreamChunk; ++j) w[j] = __fdiv_rn(tg[j], bh[j]);
        } else {
#pragma unroll
          for (int j = 0; j < kStreamChunk; ++j) {
            w[j] = 0.0f;
            if (ok[j]) {
              gather(j);
              w[j] = __fdiv_rn(tg[j], bh[j]);
            } else if (chunk.has(j)) {
              ++n_bad;
            }
          }
        }
      }
      // off the chain: the reward that counts, the factor, the clipped ratios, delta and the
      // factor of D_next
      float delta[kStreamChunk], k[kStreamChunk], rpg[kStreamChunk];
#pragma unroll
      for (int j = 0; j < kStreamChunk; ++j) {
        r[j] = reward_that_counts(r[j]);
        c[j] = frame_factor<kDiscount>(gamma, c[j]);
        const float wj = w[j] > 0.0f ? w[j] : 0.0f;         // NaN, negatives and -0 count as +0
        const float rho = wj < rho_bar ? wj : rho_bar;
        const float cs = wj < c_bar ? wj : c_bar;
        rpg[j] = wj < pg_rho_bar ? wj : pg_rho_bar;
        const float q = CAMPX_UNLESS_DONE(d[j], r[j], c[j], j == 0 ? v_after : v[j - 1]);
        delta[j] = __fmul_rn(rho, __fsub_rn(q, v[j]));
        k[j] = __fmul_rn(__fmul_rn(c[j], lam), cs);
      }
      // the chain: a multiply and an add per frame; vs and adv hang off it
#pragma unroll
      for (int j = 0; j < kStreamChunk; ++j) {
        if (chunk.has(j)) {
          D = CAMPX_UNLESS_DONE(d[j], delta[j], k[j], D);
          const float vs = __fadd_rn(v[j], D);
          const float qs = CAMPX_UNLESS_DONE(d[j], r[j], c[j], vs_after);
          vs_out[(int64_t)chunk.t(j) * vp.p_vs + env] = vs;
          adv_out[(int64_t)chunk.t(j) * vp.p_adv + env] = __fmul_rn(rpg[j], __fsub_rn(qs, v[j]));
          vs_after = vs;
          v_after = v[j];
        }
      }
    });
  }
  if (kTable) {
    // counted per lane, summed in LDS, one global atomic per workgroup that met a bad frame
    count_in_block(counters, n_bad, 0);
    __syncthreads();
    report_block_counts(counters, bad_count, nullptr);
  }
}

// The instances, at [kDiscount][kMode].
using VtraceKernel = decltype(&vtrace_kernel<false, kVtraceRatio>);
static const VtraceKernel kVtraceKernels[2][3] = {
    {vtrace_kernel<false, kVtraceRatio>, vtrace_kernel<false, kVtraceLds>,
     vtrace_kernel<false, kVtraceGlobal>},
    {vtrace_kernel<true, kVtraceRatio>, vtrace_kernel<true, kVtraceLds>,
     vtrace_kernel<true, kVtraceGlobal>}};

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_vtrace_plan(int64_t n_target_states, int64_t n_behaviour_states, int32_t n_actions,
                          int64_t B, int32_t T, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  VtracePlan p;
  const int32_t e = plan_vtrace(n_target_states, n_behaviour_states, n_actions, B, T, path, &p);
  if (e != CAMPX_OK) return e;
  plan_out[0] = p.path;
  plan_out[1] = p.lds_bytes;
  plan_out[2] = p.grid;
  return CAMPX_OK;
}

int32_t campx_vtrace_launch(const CampxVtrace* v, int64_t B, int32_t T, void* stream) {
  if (!v || !v->reward || !v->done || !v->values || !v->vs || !v->advantages || !stream_shape_ok(B, T))
    return CAMPX_EINVAL;
  const int n_table = (v->target != nullptr) + (v->behaviour != nullptr) + (v->states != nullptr) +
                      (v->actions != nullptr);
  if (n_table != 0 && n_table != 4) return CAMPX_EINVAL;
  const bool table = n_table == 4;
  if (table == (v->ratio != nullptr)) return CAMPX_EINVAL;
  if (v->path < 0 || v->path > 2) return CAMPX_EINVAL;
  if (!std::isfinite(v->gamma) || !std::isfinite(v->lam)) return CAMPX_EINVAL;
  for (const float bar : {v->rho_bar, v->c_bar, v->pg_rho_bar})
    if (!std::isfinite(bar) || bar < 0.0f) return CAMPX_EINVAL;
  if (!all_aligned(4, {v->reward, v->discount, v->values, v->bootstrap, v->ratio, v->target, v->behaviour,
                       v->states, v->vs, v->advantages}) ||
      !aligned_to(v->bad_count, 8))
    return CAMPX_EINVAL;
  if (!pitches_ok(B, T, {{v->reward, v->reward_pitch}, {v->done, v->done_pitch},
                         {v->discount, v->discount_pitch}, {v->values, v->values_pitch},
                         {v->ratio, v->ratio_pitch}, {v->states, v->states_pitch},
                         {v->actions, v->actions_pitch}, {v->vs, v->vs_pitch},
                         {v->advantages, v->advantages_pitch}}))
    return CAMPX_EINVAL;
  VtracePlan plan{kVtraceRatio, 0, stream_blocks(B)};
  VtraceParams vp{v->gamma, v->lam, v->rho_bar, v->c_bar, v->pg_rho_bar, T, B, 0, 0, 0, 0, 0,
                  v->reward_pitch, v->done_pitch, v->discount_pitch, v->values_pitch, v->ratio_pitch,
                  v->states_pitch, v->actions_pitch, v->vs_pitch, v->advantages_pitch};
  if (table) {
    const int32_t e = plan_vtrace(v->n_target_states, v->n_behaviour_states, v->n_actions, B, T,
                                  v->path, &plan);
    if (e != CAMPX_OK) return e;
    vp.Nt = (uint32_t)v->n_target_states;
    vp.Nb = (uint32_t)v->n_behaviour_states;
    vp.A = (uint32_t)v->n_actions;
    vtrace_modulus(vp.Nt, &vp.mod_m, &vp.mod_shift);
  }
  hipStream_t hs = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kVtraceKernels[v->discount != nullptr][plan.path], dim3((unsigned)plan.grid),
                     dim3(kStreamThreads), (size_t)plan.lds_bytes, hs, vp, v->reward, v->done,
                     v->discount, v->values, v->bootstrap, v->ratio, v->target, v->behaviour,
                     v->states, v->actions, v->vs, v->advantages,
                     reinterpret_cast<u64*>(v->bad_count));
  return launch_status();
}

}  // extern "C"
