// k_states.hip - the observations of given STATES of a state-table game: what a network that is
// evaluated once per state (the policy table of k_policy.hip) is evaluated on.
//
// A state's observation is a function of its row of the table blob's `cells` (where each thing
// shows, plus the scenery's variant or the mask of its pieces) - the very entries the update
// kernels write into the trace for the state a frame REACHES.  So: wide_state_rows_kernel writes
// the given states' entries as a one-frame trace of N "environments", and the rollout's render
// kernel (k_render.hip, through wide_render_source) renders it with T = 1 and B := N.  Nothing
// about the render is restated here.

#include "wide_table.hip.h"

namespace campx_impl {

constexpr int kStateRowsThreads = 256;

// One lane per row: id -> clamped id -> cells[id] -> the row's entry of every plane.
// `ids` NULL: row i is state i.  An id outside [0, n_states) is rendered as state 0 and counted.
template <bool kIdx64>
__global__ __launch_bounds__(kStateRowsThreads) void wide_state_rows_kernel(
    const u32x4* __restrict__ cells, const void* __restrict__ ids, int32_t n_states, int32_t K,
    uint16_t* __restrict__ trace, int64_t P, int64_t N, int32_t* __restrict__ bad_count,
    int32_t* __restrict__ bad_flag) {
  const int64_t row = (int64_t)blockIdx.x * kStateRowsThreads + threadIdx.x;
  const bool live = row < N;
  int64_t id = row;
  if (live && ids) {
    if (kIdx64) id = static_cast<const int64_t*>(ids)[row];
    else id = static_cast<const int32_t*>(ids)[row];
  }
  const bool bad = live && (id < 0 || id >= n_states);
  id = (!live || bad) ? 0 : id;
  const u32x4 c = cells[id];
  if (live) {
    uint16_t* at = trace + row;
    at[0] = (uint16_t)c.x;
    if (K > 1) at[P] = (uint16_t)(c.x >> 16);
    if (K > 2) at[2 * P] = (uint16_t)c.y;
    if (K > 3) at[3 * P] = (uint16_t)(c.y >> 16);
    if (K > 4) at[4 * P] = (uint16_t)c.z;
    if (K > 5) at[5 * P] = (uint16_t)(c.z >> 16);
    if (K > 6) at[6 * P] = (uint16_t)c.w;
    if (K > 7) at[7 * P] = (uint16_t)(c.w >> 16);
  }
  // one atomic per wave that met a bad id (every lane of the wave is here: nothing returned early)
  const unsigned long long met = __ballot(bad);
  if (met && (threadIdx.x & (kWave - 1)) == 0) {
    if (bad_count) atomicAdd(bad_count, (int)__popcll(met));
    if (bad_flag) __hip_atomic_store(bad_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// rows of the one-frame trace are padded like the other per-frame streams
static int64_t state_rows_pitch(int64_t N) { return (N + 15) & ~(int64_t)15; }

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int64_t campx_wide_render_states_scratch_bytes(const CampxWideSpec* s, int64_t N) {
  if (wide_validate_plain(s) != CAMPX_OK || N <= 0 || N > (1ll << 40)) return 0;
  return (int64_t)wide_layout(*s).n_planes * state_rows_pitch(N) * (int64_t)sizeof(uint16_t);
}

int32_t campx_wide_render_states_launch(const CampxWideSpec* s, const void* tables_dev,
                                        const void* state_ids, int32_t ids64, int64_t N, void* obs,
                                        int32_t obs_format, void* scratch, int64_t scratch_bytes,
                                        int32_t* bad_count, int32_t* bad_flag, void* stream) {
  if (!s || !tables_dev || !obs || !scratch || N <= 0 || N > (1ll << 40)) return CAMPX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(obs) & 15) || (reinterpret_cast<uintptr_t>(scratch) & 15) ||
      (reinterpret_cast<uintptr_t>(state_ids) & (ids64 ? 7 : 3)) ||
      (reinterpret_cast<uintptr_t>(bad_count) & 3) || (reinterpret_cast<uintptr_t>(bad_flag) & 3))
    return CAMPX_EINVAL;
  if (obs_format < CAMPX_OBS_INT8 || obs_format > CAMPX_OBS_BF16) return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  const WideTables t = wide_tables(*s, tables_dev);
  const int64_t P = state_rows_pitch(N);
  if (scratch_bytes < (int64_t)t.lay.n_planes * P * (int64_t)sizeof(uint16_t)) return CAMPX_EINVAL;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  uint16_t* trace = static_cast<uint16_t*>(scratch);
  const dim3 grid((unsigned)((N + kStateRowsThreads - 1) / kStateRowsThreads));
  hipLaunchKernelGGL(ids64 ? wide_state_rows_kernel<true> : wide_state_rows_kernel<false>, grid,
                     dim3(kStateRowsThreads), 0, hs, t.cells, state_ids, s->n_states, t.lay.n_planes, trace,
                     P, N, bad_count, bad_flag);
  const int32_t launched = launch_status();
  if (launched != CAMPX_OK) return launched;
  // One render launch addresses rows x row bytes < 2^32 - 65536: more rows go as several launches
  // of a multiple of 16 rows each (every part's output then starts on a 16-byte boundary); the
  // planes of the trace stay P entries apart whatever part is rendered.
  const RenderSource src = wide_render_source(*s, tables_dev);
  const int64_t R = (int64_t)s->n_layers * s->rows * s->cols;
  const int64_t elem = obs_format == CAMPX_OBS_INT8 ? 1 : 2;
  const int64_t most = (((1ll << 32) - 65536 - 1) / R) & ~(int64_t)15;
  for (int64_t n0 = 0; n0 < N; n0 += most) {
    const int64_t n = N - n0 < most ? N - n0 : most;
    const int32_t rc = launch_render_from(src, trace + n0, static_cast<int8_t*>(obs) + n0 * R * elem,
                                          n, 1, P, P, false, obs_format, hs);
    if (rc != CAMPX_OK) return rc;
  }
  return CAMPX_OK;
}

}  // extern "C"
