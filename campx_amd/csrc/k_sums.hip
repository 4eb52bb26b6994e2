// k_sums.hip - per-(state, action) sums of a rollout's [T, B] streams in one launch, and the
// lookup that goes with them: the learner's half of a tabular episode.
//
// The rule (include/campx_hip.h has it in full; tests/state_sums_reference.py restates it in
// numpy): every value is quantised ONCE to 64-bit fixed point,
//     d = double(x) * 2^f      q = llrint(d)      NaN -> 0, |d| > lim -> +-lim, both counted
//     acc[0][bin] += 1         acc[1 + k][bin] += q_k          bin = state * A + action
// with lim = 2^(62 - ceil(log2(T * B))): integer additions that cannot overflow, so any order and
// any privatisation give the same bits.  A frame with a state or action out of range is skipped
// and counted.
//
// state_sums_kernel: a lane per environment walks a slice of the frames (the grid is B / 256 x
// slices of T, so that a batch of a few thousand still fills the chip; streams.hip.h has
// walk_forward() and its Chunk, the id test and bin, table staging and the counters).  The walk is
// bound by latency, so a chunk of eight frames issues all its loads - coalesced along B, each
// stream with its own pitch - before its first atomic.  Two ways to accumulate:
//   LDS     (K + 1) * bins int64 accumulators in LDS, `copies` of them interleaved so that copy c
//           of an accumulator sits 8 bytes after copy c - 1: lane l adds into copy l % copies.
//           The boat race has 40 bins and the 64 lanes of a wave often sit in two or three of
//           them; one LDS address would take their adds one after the other, 64 copies spread a
//           wave's adds to one bin over 64 addresses in 64 banks.  The workgroup ends by folding
//           the copies and adding its non-zero accumulators to global memory.
//   global  no-return global_atomic_add_x2 straight into `acc`: tables that do not fit LDS.
// plan_sums() chooses; campx_state_sums_plan() shows the choice to a test without a GPU.
//
// table_lookup_kernel: out[t, e] = table[state * A + action], the same walk without atomics.

#include "streams.hip.h"

namespace campx_impl {

constexpr int kSumsMaxCopies = 64;
constexpr int64_t kSumsTargetBlocks = 2048;       // 256 CUs x 8 workgroups

struct SumsPlan {
  int32_t path;            // 1 LDS, 2 global
  int32_t copies;
  int64_t grid_b, grid_t;
  int32_t frames;          // per workgroup along T, a multiple of kStreamChunk
  int64_t lds_bytes;
  int32_t n2;
};

// How [T, B] is cut into workgroups: 256 environments x `frames` frames each, the frames a whole
// number of chunks, as many slices of T as bring the grid to about kSumsTargetBlocks.
inline void cut_frames(int64_t B, int32_t T, int64_t* grid_b, int64_t* grid_t, int32_t* frames) {
  const int64_t nb = stream_blocks(B);
  const int64_t chunks = ((int64_t)T + kStreamChunk - 1) / kStreamChunk;
  int64_t slices = kSumsTargetBlocks / nb;
  slices = slices < 1 ? 1 : (slices > chunks ? chunks : slices);
  const int64_t per = (chunks + slices - 1) / slices;      // chunks per slice
  *frames = (int32_t)(per * kStreamChunk > 0x7ffffff8ll ? 0x7ffffff8ll : per * kStreamChunk);
  *grid_t = ((int64_t)T + *frames - 1) / *frames;
  *grid_b = nb;
}

inline bool sums_shape_ok(int64_t S, int32_t A, int64_t B, int32_t T) {
  return S >= 1 && S <= 0x7fffffffll && A >= 1 && A <= 128 && stream_shape_ok(B, T);
}

inline int32_t plan_sums(int64_t S, int32_t A, int32_t K, int64_t B, int32_t T, int32_t frac_bits,
                         int32_t path, SumsPlan* p) {
  if (!sums_shape_ok(S, A, B, T) || K < 0 || K > CAMPX_SUMS_MAX_VALUES || path < 0 || path > 2)
    return CAMPX_EINVAL;
  const int64_t N = (int64_t)T * B;
  int32_t n2 = 0;
  while (n2 < 62 && (1ll << n2) < N) ++n2;
  if (frac_bits < 0 || 62 - n2 - frac_bits < 0) return CAMPX_EINVAL;
  memset(p, 0, sizeof(*p));
  p->n2 = n2;
  cut_frames(B, T, &p->grid_b, &p->grid_t, &p->frames);
  const int64_t accs = S * A * (K + 1);                    // <= 2^31 * 128 * 5
  const int64_t room = kStreamLdsBudget / 8;                 // accumulators the budget holds
  const bool fits = accs <= room;
  if (path == 1 && !fits) return CAMPX_EINVAL;
  // the flush is one global atomic per non-zero accumulator: "small" is a quarter of the frames
  // the workgroup reduces (each of which would otherwise cost K + 1 global atomics)
  const int64_t block_frames = (int64_t)kStreamThreads * p->frames;
  const bool lds = path == 1 || (path == 0 && fits && accs * 4 <= block_frames);
  p->path = lds ? 1 : 2;
  p->copies = 1;
  if (lds) {
    // copies: a power of two, at most one per lane of a wave, within the budget - and, beyond the
    // first, no more than the workgroup has frames to spread over them (zeroing and folding the
    // copies is work per workgroup too)
    int32_t c = kSumsMaxCopies;
    while (c > 1 && (accs * c > room || accs * c > block_frames)) c >>= 1;
    p->copies = c;
    p->lds_bytes = accs * c * 8;
  }
  return CAMPX_OK;
}

struct SumsParams {
  int32_t T, frames;
  int64_t B;
  uint32_t S, A;
  int32_t accs;            // LDS path: (K + 1) * bins
  int32_t copies;
  int64_t bins;
  double scale, lim;
  long long lim_q;
  int64_t p_states, p_actions;
  int64_t p_values[CAMPX_SUMS_MAX_VALUES];
  const float* values[CAMPX_SUMS_MAX_VALUES];
};

__device__ __forceinline__ long long quantise(float x, double scale, double lim, long long lim_q,
                                              u64& clamped) {
  const double d = (double)x * scale;
  if (!(fabs(d) <= lim)) {                  // NaN, +-Inf, past the limit
    ++clamped;
    return d != d ? 0ll : (d > 0.0 ? lim_q : -lim_q);
  }
  return __double2ll_rn(d);
}

// What a launch that does not accumulate starts with: the accumulators and both counters to zero,
// as one kernel on the launch's stream.
__global__ __launch_bounds__(kStreamThreads) void sums_zero_kernel(u64* __restrict__ acc, int64_t n,
                                                                 u64* __restrict__ skipped,
                                                                 u64* __restrict__ clamped) {
  const int64_t first = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kStreamThreads;
  for (int64_t i = first; i < n; i += step) acc[i] = 0;
  if (first == 0) {
    *skipped = 0;
    *clamped = 0;
  }
}

template <int K, bool kActions, bool kLds>
__global__ __launch_bounds__(kStreamThreads) void state_sums_kernel(
    SumsParams sp, const int32_t* __restrict__ states, const int8_t* __restrict__ actions,
    u64* __restrict__ acc, u64* __restrict__ skipped, u64* __restrict__ clamped) {
  extern __shared__ __align__(16) u64 lds_acc[];     // kLds: [accs][copies]
  __shared__ u64 counters[2];
  const int tid = threadIdx.x;
  if (kLds)
    for (int i = tid; i < sp.accs * sp.copies; i += kStreamThreads) lds_acc[i] = 0;
  if (tid < 2) counters[tid] = 0;
  __syncthreads();
  const int64_t env = (int64_t)blockIdx.x * kStreamThreads + tid;
  const bool live = env < sp.B;
  const int64_t col = live ? env : 0;                // any valid column
  const int32_t t_begin = (int32_t)blockIdx.y * sp.frames;
  const int32_t t_end = sp.T - t_begin < sp.frames ? sp.T : t_begin + sp.frames;
  const uint32_t copy = (uint32_t)tid & (uint32_t)(sp.copies - 1);
  u64 n_skipped = 0, n_clamped = 0;
  auto add = [&](int plane, int32_t state, int8_t action, u64 v) {
    if (kLds) {
      const uint32_t i = (uint32_t)plane * (uint32_t)sp.bins + bin_of<uint32_t>(state, action, sp.A);
      __hip_atomic_fetch_add(&lds_acc[i * (uint32_t)sp.copies + copy], v, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      const int64_t i = plane * sp.bins + bin_of<int64_t>(state, action, sp.A);
      __hip_atomic_fetch_add(&acc[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  walk_forward(t_begin, t_end, [&](auto chunk) {
    int32_t s[kStreamChunk];
    int8_t a[kStreamChunk];
    float x[K ? K : 1][kStreamChunk];
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      const int64_t t = chunk.load_t(j);
      s[j] = states[t * sp.p_states + col];
      a[j] = kActions ? actions[t * sp.p_actions + col] : (int8_t)0;
#pragma unroll
      for (int k = 0; k < K; ++k) x[k][j] = sp.values[k][t * sp.p_values[k] + col];
    }
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      if (live && chunk.has(j)) {
        if (ids_in_range(s[j], a[j], sp.S, sp.A)) {
          add(0, s[j], a[j], 1ull);
#pragma unroll
          for (int k = 0; k < K; ++k)
            add(1 + k, s[j], a[j], (u64)quantise(x[k][j], sp.scale, sp.lim, sp.lim_q, n_clamped));
        } else {
          ++n_skipped;
        }
      }
    }
  });
  if (kLds) {
    __syncthreads();
    for (int i = tid; i < sp.accs; i += kStreamThreads) {
      u64 sum = 0;
      for (int c = 0; c < sp.copies; ++c) sum += lds_acc[i * sp.copies + c];
      if (sum) __hip_atomic_fetch_add(&acc[i], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  count_in_block(counters, n_skipped, n_clamped);
  __syncthreads();
  report_block_counts(counters, skipped, clamped);
}

struct LookupParams {
  int32_t T, frames;
  int64_t B;
  uint32_t S, A;
  int32_t entries;         // LDS path: S * A
  int64_t p_states, p_actions, p_out;
};

template <bool kActions, bool kLds>
__global__ __launch_bounds__(kStreamThreads) void table_lookup_kernel(
    LookupParams lp, const float* __restrict__ table, const int32_t* __restrict__ states,
    const int8_t* __restrict__ actions, float* __restrict__ out, u64* __restrict__ bad_count) {
  extern __shared__ __align__(16) float lds_table[];
  __shared__ u64 counters[2];
  const int tid = threadIdx.x;
  if (kLds) stage_table(lds_table, table, (uint32_t)lp.entries);
  if (tid < 2) counters[tid] = 0;
  __syncthreads();
  const int64_t env = (int64_t)blockIdx.x * kStreamThreads + tid;
  const bool live = env < lp.B;
  const int64_t col = live ? env : 0;
  const int32_t t_begin = (int32_t)blockIdx.y * lp.frames;
  const int32_t t_end = lp.T - t_begin < lp.frames ? lp.T : t_begin + lp.frames;
  u64 n_bad = 0;
  walk_forward(t_begin, t_end, [&](auto chunk) {
    int32_t s[kStreamChunk];
    int8_t a[kStreamChunk];
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      const int64_t t = chunk.load_t(j);
      s[j] = states[t * lp.p_states + col];
      a[j] = kActions ? actions[t * lp.p_actions + col] : (int8_t)0;
    }
    // every read of the table before the first store; a bad index reads entry 0 and shows 0.0
    float v[kStreamChunk];
    bool ok[kStreamChunk];
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      ok[j] = ids_in_range(s[j], a[j], lp.S, lp.A);
      const int64_t i = ok[j] ? bin_of<int64_t>(s[j], a[j], lp.A) : 0;
      v[j] = kLds ? lds_table[(uint32_t)i] : table[i];
    }
#pragma unroll
    for (int j = 0; j < kStreamChunk; ++j) {
      if (live && chunk.has(j)) {
        out[(int64_t)chunk.t(j) * lp.p_out + env] = ok[j] ? v[j] : 0.0f;
        n_bad += ok[j] ? 0 : 1;
      }
    }
  });
  count_in_block(counters, n_bad, 0);
  __syncthreads();
  report_block_counts(counters, bad_count, nullptr);
}

// The instances, at [K][kActions][kLds] and [kActions][kLds].
using SumsKernel = decltype(&state_sums_kernel<0, false, false>);
static const SumsKernel kSumsKernels[CAMPX_SUMS_MAX_VALUES + 1][2][2] = {
    {{state_sums_kernel<0, false, false>, state_sums_kernel<0, false, true>},
     {state_sums_kernel<0, true, false>, state_sums_kernel<0, true, true>}},
    {{state_sums_kernel<1, false, false>, state_sums_kernel<1, false, true>},
     {state_sums_kernel<1, true, false>, state_sums_kernel<1, true, true>}},
    {{state_sums_kernel<2, false, false>, state_sums_kernel<2, false, true>},
     {state_sums_kernel<2, true, false>, state_sums_kernel<2, true, true>}},
    {{state_sums_kernel<3, false, false>, state_sums_kernel<3, false, true>},
     {state_sums_kernel<3, true, false>, state_sums_kernel<3, true, true>}},
    {{state_sums_kernel<4, false, false>, state_sums_kernel<4, false, true>},
     {state_sums_kernel<4, true, false>, state_sums_kernel<4, true, true>}}};
using LookupKernel = decltype(&table_lookup_kernel<false, false>);
static const LookupKernel kLookupKernels[2][2] = {
    {table_lookup_kernel<false, false>, table_lookup_kernel<false, true>},
    {table_lookup_kernel<true, false>, table_lookup_kernel<true, true>}};

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_state_sums_plan(int64_t n_states, int32_t n_actions, int32_t n_values, int64_t B,
                              int32_t T, int32_t frac_bits, int32_t path, int64_t* plan_out) {
  if (!plan_out) return CAMPX_EINVAL;
  SumsPlan p;
  const int32_t e = plan_sums(n_states, n_actions, n_values, B, T, frac_bits, path, &p);
  if (e != CAMPX_OK) return e;
  plan_out[0] = p.path;
  plan_out[1] = p.copies;
  plan_out[2] = p.grid_b;
  plan_out[3] = p.grid_t;
  plan_out[4] = p.frames;
  plan_out[5] = p.lds_bytes;
  plan_out[6] = p.n2;
  plan_out[7] = 62 - p.n2;
  return CAMPX_OK;
}

int32_t campx_state_sums_launch(const CampxStateSums* s, int64_t B, int32_t T, void* stream) {
  if (!s || !s->states || !s->acc || !s->skipped || !s->clamped) return CAMPX_EINVAL;
  SumsPlan plan;
  const int32_t e = plan_sums(s->n_states, s->n_actions, s->n_values, B, T, s->frac_bits, s->path, &plan);
  if (e != CAMPX_OK) return e;
  const int K = s->n_values;
  if (!s->actions && s->n_actions != 1) return CAMPX_EINVAL;
  if (!aligned_to(s->states, 4) || !all_aligned(8, {s->acc, s->skipped, s->clamped})) return CAMPX_EINVAL;
  if (!pitches_ok(B, T, {{s->states, s->states_pitch}, {s->actions, s->actions_pitch}})) return CAMPX_EINVAL;
  for (int k = 0; k < K; ++k)
    if (!s->values[k] || !aligned_to(s->values[k], 4) || !pitches_ok(B, T, {{s->values[k], s->values_pitch[k]}}))
      return CAMPX_EINVAL;
  SumsParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.T = T;
  sp.frames = plan.frames;
  sp.B = B;
  sp.S = (uint32_t)s->n_states;
  sp.A = (uint32_t)s->n_actions;
  sp.bins = s->n_states * s->n_actions;
  sp.accs = plan.path == 1 ? (int32_t)(sp.bins * (K + 1)) : 0;
  sp.copies = plan.copies;
  sp.scale = (double)(1ll << s->frac_bits);
  sp.lim_q = 1ll << (62 - plan.n2);
  sp.lim = (double)sp.lim_q;
  sp.p_states = s->states_pitch;
  sp.p_actions = s->actions_pitch;
  for (int k = 0; k < K; ++k) {
    sp.values[k] = s->values[k];
    sp.p_values[k] = s->values_pitch[k];
  }
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)plan.grid_b, (unsigned)plan.grid_t);
  u64* acc = reinterpret_cast<u64*>(s->acc);
  u64* skipped = reinterpret_cast<u64*>(s->skipped);
  u64* clamped = reinterpret_cast<u64*>(s->clamped);
  if (!s->accumulate) {
    const int64_t n = sp.bins * (K + 1);
    const int64_t blocks = (n + 4 * kStreamThreads - 1) / (4 * kStreamThreads);
    hipLaunchKernelGGL(sums_zero_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)),
                       dim3(kStreamThreads), 0, hs, acc, n, skipped, clamped);
    const int32_t launched = launch_status();
    if (launched != CAMPX_OK) return launched;
  }
  hipLaunchKernelGGL(kSumsKernels[K][s->actions != nullptr][plan.path == 1], grid, dim3(kStreamThreads),
                     (size_t)plan.lds_bytes, hs, sp, s->states, s->actions, acc, skipped, clamped);
  return launch_status();
}

int32_t campx_table_lookup_launch(const CampxTableLookup* l, int64_t B, int32_t T, void* stream) {
  if (!l || !l->table || !l->states || !l->out) return CAMPX_EINVAL;
  if (!sums_shape_ok(l->n_states, l->n_actions, B, T)) return CAMPX_EINVAL;
  if (!l->actions && l->n_actions != 1) return CAMPX_EINVAL;
  if (!all_aligned(4, {l->table, l->states, l->out}) || !aligned_to(l->bad_count, 8)) return CAMPX_EINVAL;
  if (!pitches_ok(B, T, {{l->states, l->states_pitch}, {l->out, l->out_pitch}, {l->actions, l->actions_pitch}}))
    return CAMPX_EINVAL;
  LookupParams lp;
  memset(&lp, 0, sizeof(lp));
  int64_t grid_b, grid_t;
  cut_frames(B, T, &grid_b, &grid_t, &lp.frames);
  lp.T = T;
  lp.B = B;
  lp.S = (uint32_t)l->n_states;
  lp.A = (uint32_t)l->n_actions;
  lp.p_states = l->states_pitch;
  lp.p_actions = l->actions_pitch;
  lp.p_out = l->out_pitch;
  const int64_t entries = l->n_states * l->n_actions;
  const bool lds = table_staged(entries, lp.frames);
  lp.entries = lds ? (int32_t)entries : 0;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)grid_b, (unsigned)grid_t);
  u64* bad = reinterpret_cast<u64*>(l->bad_count);
  hipLaunchKernelGGL(kLookupKernels[l->actions != nullptr][lds], grid, dim3(kStreamThreads),
                     (size_t)(lds ? entries * 4 : 0), hs, lp, l->table, l->states, l->actions, l->out, bad);
  return launch_status();
}

}  // extern "C"
