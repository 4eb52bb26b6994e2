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

}  // extern "C"
