// k_gather.hip - gather_kernel: renders an arbitrary list of (frame, environment) pairs from a
// stored trace into a dense minibatch of observations.
#include "campx_common.hip.h"

namespace campx_impl {

// ---------------------------------------------------------------------------
// The output is N rows of R = L*H*W bytes back to back: "one frame of N environments" to
// render_kernel's window scheme (k_render.hip) - one-shot waves, windows aligned in MEMORY,
// the scenery's chunk from the pre-rotated rows, patches in LDS, one aligned 16-byte store per
// lane.  The one difference: row i's trace entries are not at `i` of each plane but at
//     t_idx[i] * pitch + e_idx[i],
// one more dependent load.  Everything a row needs from the trace hangs off ONE lane per row:
// it loads the row's two indices first (before anything else the wave does), clamps them,
// loads the row's entry from every plane and parks them in LDS; the patch pass then reads LDS
// only.  (Per row, not per slot or per chunk: a row of boat race has two patch slots and eleven
// chunks, and k_render.hip's notes on its variant path say what gathers per chunk cost.)
// Patches are laid per (row, thing) with the thing a uniform loop, so the thing count is a
// run-time value here and there is one instantiation per (format, entry width, scenery kind).
struct GatherParams {
  uint32_t R;                 // row bytes
  uint32_t m, sh1, sh2;       // exact n / R for 32-bit n (Granlund-Montgomery)
  uint32_t total;             // N * R
  uint32_t shift;             // bytes (16-bit formats: elements) from the first window's start to dst
  uint32_t n_rows;            // N
  int32_t n_dyn, n_planes, cells, n_variants, n_pieces;
  int32_t idx64;              // the indices are int64 (else int32)
  int32_t nt;                 // streaming stores (else plain ones)
  int64_t B, T;               // what the indices are clamped to
  int64_t pitch, plane;       // entries from one frame's row to the next, from one plane to the next
  int32_t dyn_off[CAMPX_WIDE_MAX_DYN];
  const int8_t* rot;          // device: the 16 rotations of the scenery row (per variant)
  const uint8_t* top_layer;   // device: scenery layer per cell (one-byte trace only)
  int64_t rot_stride;
  const uint32_t* pieces;     // device, per piece: (byte it sets) | (byte it clears) << 16
  const void* t_idx;
  const void* e_idx;
  int32_t* bad_count;
  int32_t* bad_flag;
};

// One-cell tier: cell | visible << 7.  State-table tier: cell | covered layer << 10 | shows << 15.
template <bool kWide>
struct GatherEntry {
  using Entry = uint8_t;
  static constexpr int kPlanes = CAMPX_MAX_DYN;
  static __device__ __forceinline__ uint32_t cell(uint32_t e) { return e & 0x7fu; }
  static __device__ __forceinline__ bool visible(uint32_t e) { return (e >> 7) != 0; }
};
template <>
struct GatherEntry<true> {
  using Entry = uint16_t;
  static constexpr int kPlanes = CAMPX_WIDE_MAX_DYN + 1;
  static __device__ __forceinline__ uint32_t cell(uint32_t e) { return e & 0x3ffu; }
  static __device__ __forceinline__ bool visible(uint32_t e) { return (e >> 15) != 0; }
  static __device__ __forceinline__ uint32_t covered(uint32_t e) { return (e >> 10) & 0xfu; }
};

constexpr int kGatherWaves = 2;

// kFmt: 0 int8, 1 f16, 2 bf16 (a wave's window is 2 KiB of what it WRITES: 2 KiB of the int8
// image, 1 KiB of it for the 16-bit formats).  kScen: 0 plain scenery, 1 variants, 2 pieces.
template <int kFmt, bool kWide, int kScen>
__global__ __launch_bounds__(kGatherWaves * kWave) void gather_kernel(
    GatherParams gp, const typename GatherEntry<kWide>::Entry* __restrict__ trace,
    int8_t* __restrict__ dst) {
  using Fmt = GatherEntry<kWide>;
  using Entry = typename Fmt::Entry;
  constexpr bool kVar = kScen == 1, kMask = kScen == 2;
  constexpr int kWin = kFmt ? 1 : 2;
  constexpr int kPlanes = Fmt::kPlanes;
  // rows a window overlaps, and the one after (rows of at least 16 bytes): span / 16 + 2
  constexpr int kRowIter = kFmt ? 2 : 3;
  constexpr int kRowCap = kRowIter * kWave;
  static_assert(1024 * kWin / 16 + 2 <= kRowCap, "a window's rows fit the staging area");
  __shared__ __attribute__((aligned(16))) int8_t lds[kGatherWaves * kWin * 1024];
  __shared__ uint16_t scen_off_all[kGatherWaves][kWide ? 2 : CAMPX_MAX_CELLS];
  __shared__ Entry row_ent_all[kGatherWaves][kRowCap * kPlanes];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t bx = blockIdx.x;
  bx = (bx & 7u) * (gridDim.x >> 3) + (bx >> 3);     // gridDim.x is a multiple of 8: one XCD, one eighth
  const uint32_t span = 1024u * kWin;
  const uint32_t widx = bx * (uint32_t)kGatherWaves + (uint32_t)wave;
  if ((uint64_t)widx * span >= (uint64_t)gp.total + gp.shift) return;
  // (offsets are modulo 2^32: the first window starts `shift` before the output, its lanes
  // before it fail the one `off < total` test)
  const uint32_t woff0 = widx * span - gp.shift;
  const uint32_t wlo = widx * span < gp.shift ? 0u : woff0;
  int8_t* win0 = lds + wave * (kWin * 1024);
  uint16_t* scen_off = scen_off_all[wave];
  Entry* row_ent = row_ent_all[wave];
  const int R = (int)gp.R;
  const int rot_pitch = ((R + 15) & ~15) + 16;
  auto div_r = [&](uint32_t n) -> uint32_t {
    const uint32_t hi = __umulhi(gp.m, n);
    return (((n - hi) >> gp.sh1) + hi) >> gp.sh2;
  };
  const uint32_t first_row = div_r(wlo);
  const uint32_t wend = (woff0 + span - 1u < gp.total) ? woff0 + span - 1u : gp.total - 1u;
  const uint32_t last_row = div_r(wend);
  const int n_here = (int)(last_row - first_row + 1u);
  const int n_stage = n_here + 1;      // (the row after: a chunk may run over into it)

  // ---- the rows' indices: HBM loads, issued before anything else
  int64_t ti[kRowIter], ei[kRowIter];
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    uint32_t row = first_row + (uint32_t)(lane + it * kWave);
    row = row < gp.n_rows ? row : gp.n_rows - 1u;      // clamp: entry unused
    ti[it] = ei[it] = 0;
    if (it == 0 || n_stage > it * kWave) {
      if (gp.idx64) {
        ti[it] = static_cast<const int64_t*>(gp.t_idx)[row];
        ei[it] = static_cast<const int64_t*>(gp.e_idx)[row];
      } else {
        ti[it] = static_cast<const int32_t*>(gp.t_idx)[row];
        ei[it] = static_cast<const int32_t*>(gp.e_idx)[row];
      }
    }
  }

  // ---- scenery (the plain kind needs nothing from the trace): issue the loads
  u32x4 scen[kWin];
  if constexpr (!kVar) {
#pragma unroll
    for (int j = 0; j < kWin; ++j) {
      const uint32_t off = woff0 + j * 1024u + (uint32_t)lane * 16u;
      int k = (int)(off - div_r(off) * gp.R);                        // off % R
      // (a chunk that starts before the output: its last bytes are row 0's first)
      if (off >= 0xfffffff0u) k = R - (int)(0u - off);
      scen[j] = *reinterpret_cast<const u32x4*>(gp.rot + (k & 15) * rot_pitch + (k & ~15));
    }
  }
  uint32_t top2 = 0;
  if (!kWide) top2 = *reinterpret_cast<const uint16_t*>(gp.top_layer + 2 * lane);

  // ---- indices -> clamped position in a plane -> the row's entry of every plane
  int bad = 0;
  Entry ent[kRowIter][kPlanes];
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    const int i = lane + it * kWave;
    int64_t t = ti[it], e = ei[it];
    const bool out_of_range = t < 0 || t >= gp.T || e < 0 || e >= gp.B;
    // a row is counted by the one wave whose window it STARTS in
    bad += (out_of_range && i < n_here && (first_row + (uint32_t)i) * gp.R >= wlo) ? 1 : 0;
    t = t < 0 ? 0 : (t >= gp.T ? gp.T - 1 : t);
    e = e < 0 ? 0 : (e >= gp.B ? gp.B - 1 : e);
    const int64_t at = t * gp.pitch + e;
#pragma unroll
    for (int d = 0; d < kPlanes; ++d) {
      ent[it][d] = 0;
      if ((it == 0 || n_stage > it * kWave) && d < gp.n_planes) ent[it][d] = trace[(int64_t)d * gp.plane + at];
    }
  }
  if (bad) {
    if (gp.bad_count) atomicAdd(gp.bad_count, bad);
    if (gp.bad_flag) __hip_atomic_store(gp.bad_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    const int i = lane + it * kWave;
#pragma unroll
    for (int d = 0; d < kPlanes; ++d)
      if ((it == 0 || n_stage > it * kWave) && d < gp.n_planes && i < n_stage) row_ent[i * kPlanes + d] = ent[it][d];
  }
  __builtin_amdgcn_wave_barrier();

  if constexpr (kVar) {
    // a scenery in variants: plane n_dyn names each row's; a chunk that runs over the end of a
    // row takes the rest from the NEXT row's variant (merge_rows, as render_kernel<kVar>)
#pragma unroll
    for (int j = 0; j < kWin; ++j) {
      const uint32_t off = woff0 + j * 1024u + (uint32_t)lane * 16u;
      const uint32_t row = div_r(off);
      int k = (int)(off - row * gp.R);
      const bool before = off >= 0xfffffff0u;
      if (before) k = R - (int)(0u - off);
      uint32_t i0 = before ? 0u : row - first_row, i1 = before ? 0u : row + 1u - first_row;
      i0 = i0 < (uint32_t)n_stage ? i0 : (uint32_t)n_stage - 1u;
      i1 = i1 < (uint32_t)n_stage ? i1 : (uint32_t)n_stage - 1u;
      const uint32_t vmax = (uint32_t)gp.n_variants - 1u;
      uint32_t v0 = Fmt::cell(row_ent[i0 * kPlanes + gp.n_dyn]), v1 = Fmt::cell(row_ent[i1 * kPlanes + gp.n_dyn]);
      v0 = v0 < vmax ? v0 : vmax;        // (a trace from anywhere: nothing is read outside the tables)
      v1 = v1 < vmax ? v1 : vmax;
      const int8_t* here = gp.rot + (k & 15) * rot_pitch + (k & ~15);
      u32x4 mine = variant_chunk(here, gp.rot_stride, (int)v0);
      const int left = R - k;
      if (left < 16 && v1 != v0) mine = merge_rows(mine, variant_chunk(here, gp.rot_stride, (int)v1), left);
      scen[j] = mine;
    }
  }

#pragma unroll
  for (int j = 0; j < kWin; ++j)
    *reinterpret_cast<u32x4*>(win0 + j * 1024 + lane * 16) = scen[j];
  if (!kWide) {
    const uint32_t c = 2u * (uint32_t)lane;
    const uint32_t lo = (top2 & 0xffu) * (uint32_t)gp.cells + c;
    const uint32_t hi2 = (top2 >> 8) * (uint32_t)gp.cells + c + 1u;
    *reinterpret_cast<uint32_t*>(scen_off + c) = lo | (hi2 << 16);
  }
  __builtin_amdgcn_wave_barrier();

  // ---- patches: per row of the window, per thing, one byte set and one cleared
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    const int i = lane + it * kWave;
    if (it > 0 && n_here <= it * kWave) break;
    const bool mine = i < n_here;
    // (a patch left of the window wraps to a huge unsigned value and fails the one comparison)
    const uint32_t row0 = (first_row + (uint32_t)i) * gp.R - woff0;
    for (int d = 0; d < gp.n_dyn; ++d) {
      const uint32_t e = mine ? (uint32_t)row_ent[i * kPlanes + d] : 0u;
      const uint32_t cell = Fmt::cell(e);
      uint32_t under;
      if constexpr (kWide) under = Fmt::covered(e) * (uint32_t)gp.cells + cell;
      else under = scen_off[cell];
      const uint32_t a = row0 + (uint32_t)gp.dyn_off[d] + cell, b = row0 + under;
      if (mine && Fmt::visible(e)) {
        if (b < span) win0[b] = 0;
        if (a < span) win0[a] = 1;
      }
    }
    if constexpr (kMask) {
      const uint32_t shown = mine ? (uint32_t)row_ent[i * kPlanes + gp.n_dyn] : 0u;
      for (int p = 0; p < gp.n_pieces; ++p) {
        const uint32_t piece = gp.pieces[p];
        const uint32_t a = row0 + (piece & 0xffffu), b = row0 + (piece >> 16);
        if ((shown >> p) & 1u) {
          if (a < span) win0[a] = 1;
          if (b < span) win0[b] = 0;
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();

  // ---- out: aligned, contiguous KiB stores; the output's last chunk byte by byte
  if (kFmt == 0) {
#pragma unroll
    for (int j = 0; j < kWin; ++j) {
      const uint32_t off = woff0 + j * 1024u + (uint32_t)lane * 16u;
      if (off < gp.total) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(win0 + j * 1024 + lane * 16);
        if (off + 16u > gp.total) {
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
          for (uint32_t i = 0; off + i < gp.total; ++i) dst[off + i] = (int8_t)(w[i >> 2] >> ((i & 3u) * 8u));
        } else if (gp.nt) {
          store16_streaming_at(dst, off, v);
        } else {
          *reinterpret_cast<u32x4*>(dst + off) = v;
        }
      }
    }
  } else {
    constexpr uint32_t kOne = (kFmt == 1) ? 0x3C00u : 0x3F80u;
    uint16_t* dst16 = reinterpret_cast<uint16_t*>(dst);
#pragma unroll
    for (int h = 0; h < 2 * kWin; ++h) {
      const uint32_t elem = woff0 + (uint32_t)h * 512u + (uint32_t)lane * 8u;
      if (elem < gp.total) {
        const uint2 b = *reinterpret_cast<const uint2*>(win0 + h * 512 + lane * 8);
        u32x4 v;
        v.x = ((b.x & 0xffu) | ((b.x << 8) & 0x00ff0000u)) * kOne;
        v.y = (((b.x >> 16) & 0xffu) | ((b.x >> 8) & 0x00ff0000u)) * kOne;
        v.z = ((b.y & 0xffu) | ((b.y << 8) & 0x00ff0000u)) * kOne;
        v.w = (((b.y >> 16) & 0xffu) | ((b.y >> 8) & 0x00ff0000u)) * kOne;
        if (elem + 8u > gp.total) {
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
          for (uint32_t i = 0; elem + i < gp.total; ++i)
            dst16[elem + i] = (uint16_t)(w[i >> 1] >> ((i & 1u) * 16u));
        } else if (gp.nt) {
          store16_streaming(reinterpret_cast<u32x4*>(dst16 + elem), v);
        } else {
          *reinterpret_cast<u32x4*>(dst16 + elem) = v;
        }
      }
    }
  }
}

// The launch arithmetic, on its own so that campx_render_gather_plan() can hand it to a test:
// tests/test_gather_api.py restates it and checks the division over every row length.
GatherPlan gather_plan(int64_t N, int64_t R, int fmt, uint64_t dst_addr) {
  GatherPlan p;
  memset(&p, 0, sizeof(p));
  // exact unsigned 32-bit division by R (Granlund & Montgomery 1994, fig. 4.1)
  uint32_t l = 0;
  while ((1ull << l) < (uint64_t)R) ++l;
  p.m = (uint32_t)(((1ull << 32) * ((1ull << l) - (uint64_t)R)) / (uint64_t)R + 1);
  p.sh1 = l < 1 ? l : 1;
  p.sh2 = l > 0 ? l - 1 : 0;
  p.total = (uint32_t)(N * R);
  const uint32_t wspan = fmt ? 1024u : 2048u;          // image bytes of one wave's window
  // windows aligned in memory; for the 16-bit formats in units of image bytes = elements
  p.shift = (uint32_t)((dst_addr >> (fmt ? 1 : 0)) & (wspan - 1u));
  const uint64_t span = (uint64_t)wspan * kGatherWaves;
  // rounded up to a multiple of 8 for the XCD remap; surplus blocks exit at once
  p.grid = (uint32_t)(((((uint64_t)p.total + p.shift + span - 1u) / span) + 7u) & ~(uint64_t)7);
  return p;
}

int32_t launch_gather_from(const RenderSource& src, const CampxGather& g, int64_t B, hipStream_t stream) {
  const int HW = src.rows * src.cols;
  const int64_t R = (int64_t)src.n_layers * HW;
  const GatherPlan plan = gather_plan(g.N, R, g.obs_format, reinterpret_cast<uintptr_t>(g.obs));
  GatherParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.R = (uint32_t)R;
  gp.m = plan.m;
  gp.sh1 = plan.sh1;
  gp.sh2 = plan.sh2;
  gp.total = plan.total;
  gp.shift = plan.shift;
  gp.n_rows = (uint32_t)g.N;
  gp.n_dyn = src.n_dyn;
  gp.n_planes = (int32_t)g.n_planes;
  gp.cells = HW;
  gp.n_variants = src.n_variants > 1 ? src.n_variants : 1;
  gp.n_pieces = src.n_pieces;
  gp.idx64 = g.idx64 ? 1 : 0;
  gp.nt = g.streaming ? 1 : 0;
  gp.B = B;
  gp.T = g.T;
  gp.pitch = g.pitch;
  gp.plane = g.plane;
  for (int d = 0; d < src.n_dyn; ++d) gp.dyn_off[d] = src.dyn_layer[d] * HW;
  gp.rot = src.rot_obs;
  gp.top_layer = src.top_layer;
  gp.rot_stride = src.rot_obs_stride;
  gp.pieces = src.pieces_obs;
  gp.t_idx = g.t_idx;
  gp.e_idx = g.e_idx;
  gp.bad_count = g.bad_count;
  gp.bad_flag = g.bad_flag;
  const dim3 grid(plan.grid), block(kGatherWaves * kWave);
  int8_t* dst = static_cast<int8_t*>(g.obs);
#define CAMPX_GATHER2(FMT, WIDE, SCEN)                                                      \
  hipLaunchKernelGGL((gather_kernel<FMT, WIDE, SCEN>), grid, block, 0, stream, gp,          \
                     static_cast<const typename GatherEntry<WIDE>::Entry*>(g.trace), dst)
#define CAMPX_GATHER(WIDE, SCEN)                                              \
  do {                                                                        \
    if (g.obs_format == CAMPX_OBS_F16) CAMPX_GATHER2(1, WIDE, SCEN);          \
    else if (g.obs_format == CAMPX_OBS_BF16) CAMPX_GATHER2(2, WIDE, SCEN);    \
    else CAMPX_GATHER2(0, WIDE, SCEN);                                        \
  } while (0)
  if (!src.wide) CAMPX_GATHER(false, 0);
  else if (src.n_variants > 1) CAMPX_GATHER(true, 1);
  else if (src.n_pieces > 0) CAMPX_GATHER(true, 2);
  else CAMPX_GATHER(true, 0);
#undef CAMPX_GATHER
#undef CAMPX_GATHER2
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CAMPX_OK : hip_failed(e);
}

// What both gather entry points ask of a request, given the game's row bytes and plane count;
// before anything touches a device.
int32_t gather_check(const CampxGather* g, int64_t B, int64_t R, int64_t n_planes, int entry_bytes) {
  if (!g || !g->trace || !g->t_idx || !g->e_idx || !g->obs) return CAMPX_EINVAL;
  if (g->N <= 0 || B <= 0 || g->T <= 0) return CAMPX_EINVAL;
  if (reinterpret_cast<uintptr_t>(g->obs) & 15) return CAMPX_EINVAL;
  if (reinterpret_cast<uintptr_t>(g->trace) & (uintptr_t)(entry_bytes - 1)) return CAMPX_EINVAL;
  const uintptr_t idx_align = g->idx64 ? 7 : 3;
  if ((reinterpret_cast<uintptr_t>(g->t_idx) | reinterpret_cast<uintptr_t>(g->e_idx)) & idx_align) return CAMPX_EINVAL;
  if (g->obs_format < CAMPX_OBS_INT8 || g->obs_format > CAMPX_OBS_BF16) return CAMPX_EINVAL;
  if (g->pitch < B) return CAMPX_EINVAL;
  if (g->n_planes != n_planes) return CAMPX_EINVAL;
  // (positions inside a plane stay below 2^40: no product below overflows)
  if (g->T > (1ll << 40) / g->pitch) return CAMPX_EINVAL;
  if (n_planes > 1 && g->plane < g->T * g->pitch) return CAMPX_EINVAL;
  if (R < 16) return CAMPX_EINVAL;
  if (g->N > ((1ll << 32) - 65536 - 1) / R) return CAMPX_EINVAL;
  return CAMPX_OK;
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_render_gather_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev,
                                   const CampxGather* g, int64_t B, void* stream) {
  if (!spec_host || !spec_dev) return CAMPX_EINVAL;
  const int32_t v = campx_spec_validate(spec_host);
  if (v != CAMPX_OK) return v;
  if (!spec_host->render_valid) return CAMPX_ESPEC;
  const int64_t R = (int64_t)spec_host->n_layers * spec_host->rows * spec_host->cols;
  const int32_t rc = gather_check(g, B, R, spec_host->n_dyn, 1);
  if (rc != CAMPX_OK) return rc;
  RenderSource src;
  memset(&src, 0, sizeof(src));
  src.rows = spec_host->rows;
  src.cols = spec_host->cols;
  src.n_layers = spec_host->n_layers;
  src.n_dyn = spec_host->n_dyn;
  for (int d = 0; d < spec_host->n_dyn; ++d) src.dyn_layer[d] = spec_host->dyn_layer[d];
  const char* blob = reinterpret_cast<const char*>(spec_dev);
  src.rot_obs = reinterpret_cast<const int8_t*>(blob + offsetof(CampxSpec, rot_obs));
  src.top_layer = reinterpret_cast<const uint8_t*>(blob + offsetof(CampxSpec, static_top_layer));
  src.wide = false;
  return launch_gather_from(src, *g, B, static_cast<hipStream_t>(stream));
}

int32_t campx_render_gather_plan(int64_t N, int32_t R, int32_t obs_format, uint64_t dst_addr,
                                 int64_t* plan_out) {
  if (!plan_out || N <= 0 || R < 16 || R > CAMPX_MAX_LAYERS * CAMPX_WIDE_MAX_CELLS ||
      obs_format < CAMPX_OBS_INT8 || obs_format > CAMPX_OBS_BF16 || (dst_addr & 15) ||
      N > ((1ll << 32) - 65536 - 1) / R)
    return CAMPX_EINVAL;
  const GatherPlan p = gather_plan(N, R, obs_format, dst_addr);
  plan_out[0] = p.m;
  plan_out[1] = p.sh1;
  plan_out[2] = p.sh2;
  plan_out[3] = p.total;
  plan_out[4] = p.shift;
  plan_out[5] = p.grid;
  plan_out[6] = obs_format ? 1024 : 2048;
  plan_out[7] = kGatherWaves;
  return CAMPX_OK;
}

}  // extern "C"
