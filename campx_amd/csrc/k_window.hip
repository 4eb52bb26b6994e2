// k_window.hip - window_kernel: observation WINDOWS of a state-table game - h x w cells round a
// tracked thing (egocentric) or at a fixed place of the board - rendered straight from trace
// entries, without the full [L, H, W] observation ever being written.
#include "wide_table.hip.h"

namespace campx_impl {

// ---------------------------------------------------------------------------
// The output is N rows of Rw = L*h*w bytes back to back, and gather_kernel's output scheme
// (k_gather.hip) is taken as it stands: one-shot waves, a wave owns a window of the OUTPUT that is
// aligned in memory (2 KiB of int8, 1 KiB of image for the 16-bit formats), builds it in LDS and
// stores aligned 16-byte chunks; one lane per row loads the row's indices, then its entry of every
// plane, and parks them in LDS.  (Two meanings of "window" meet here: a wave's window of the
// output, `win0`, and the game's h x w window, which is what a ROW holds.)
//
// What differs is the fill.  A row is not a contiguous slice of the pre-rotated scenery row, so
// each output byte is computed:   (layer_of_cell[variant][board cell] == l)   on the board, and
// (l == pad layer) off it.  A lane walks its 16 bytes with (row, l, y, x) as counters - divisions
// only for the chunk's first byte.  The things' patches and the pieces are then laid wherever
// their cell falls inside the row's h x w window (one unsigned comparison per axis), in the order
// gather_kernel lays them, so that a window is bit for bit a crop of the full observation.
struct WindowParams {
  uint32_t R;                 // Rw: row bytes, L*h*w
  uint32_t m, sh1, sh2;       // exact n / Rw for 32-bit n (gather_plan)
  uint32_t total;             // N * Rw
  uint32_t shift;
  uint32_t n_rows;            // N
  int32_t n_dyn, n_planes, n_variants, n_pieces;
  int32_t H, W, HW, L;
  int32_t h, w, hw;           // the window, and h*w
  uint32_t mW;                // ceil(2^20 / W): cell / W == (cell * mW) >> 20 for cell < 1024
  int32_t thing;              // egocentric: the plane whose entry centres the window; -1: fixed
  int32_t r0, c0;             // fixed: board coordinates of the window's top-left cell
  int32_t pad;                // layer set off the board, or 0xff for none
  int32_t idx64, nt;
  int32_t n_states;
  int64_t B, T;               // what the indices are clamped to (whole trace: row i is (i / B, i % B))
  int64_t pitch, plane;
  int32_t dyn_layer[CAMPX_WIDE_MAX_DYN];
  uint32_t pieces[CAMPX_WIDE_MAX_PIECES];   // col | row << 8 | layer it sets << 16 | layer it clears << 24
  const uint8_t* loc;         // device: layer_of_cell, CAMPX_WIDE_MAX_CELLS bytes per variant
  const uint16_t* trace;
  const u32x4* cells;         // the blob's per-state entries (k_states.hip)
  const void* t_idx;          // (state ids: t_idx holds them, NULL for arange)
  const void* e_idx;
  int32_t* bad_count;
  int32_t* bad_flag;
};

constexpr int kWindowWaves = 2;      // (gather_plan() sizes the grid for workgroups of two waves)
constexpr int kWindowPlanes = CAMPX_WIDE_MAX_DYN;   // things + the variant's / the mask's plane: at most 8

// what the row's lane leaves in LDS for the fill: (r0 + 256) | (c0 + 256) << 10 | variant << 20
__device__ __forceinline__ uint32_t pack_anchor(int r0, int c0, uint32_t variant) {
  return (uint32_t)(r0 + 256) | ((uint32_t)(c0 + 256) << 10) | (variant << 20);
}

// kFmt: 0 int8, 1 f16, 2 bf16.  kSrc: CAMPX_WINDOWS_PAIRS / _TRACE / _STATES.  kScen: 0 plain
// scenery, 1 variants, 2 pieces.
template <int kFmt, int kSrc, int kScen>
__global__ __launch_bounds__(kWindowWaves * kWave) void window_kernel(WindowParams wp,
                                                                      int8_t* __restrict__ dst) {
  constexpr bool kVar = kScen == 1, kMask = kScen == 2;
  constexpr int kWin = kFmt ? 1 : 2;
  constexpr int kPlanes = kWindowPlanes;
  constexpr int kRowIter = kFmt ? 2 : 3;              // rows of at least 16 bytes: span / 16 + 2
  constexpr int kRowCap = kRowIter * kWave;
  static_assert(1024 * kWin / 16 + 2 <= kRowCap, "a window's rows fit the staging area");
  __shared__ __attribute__((aligned(16))) int8_t lds[kWindowWaves * kWin * 1024];
  __shared__ __attribute__((aligned(16))) uint8_t loc_all[kWindowWaves][kVar ? 16 : CAMPX_WIDE_MAX_CELLS];
  __shared__ uint16_t row_ent_all[kWindowWaves][kRowCap * kPlanes];
  __shared__ uint32_t row_anchor_all[kWindowWaves][kRowCap];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t bx = blockIdx.x;
  bx = (bx & 7u) * (gridDim.x >> 3) + (bx >> 3);     // gridDim.x is a multiple of 8: one XCD, one eighth
  const uint32_t span = 1024u * kWin;
  const uint32_t widx = bx * (uint32_t)kWindowWaves + (uint32_t)wave;
  if ((uint64_t)widx * span >= (uint64_t)wp.total + wp.shift) return;
  const uint32_t woff0 = widx * span - wp.shift;
  const uint32_t wlo = widx * span < wp.shift ? 0u : woff0;
  int8_t* win0 = lds + wave * (kWin * 1024);
  uint8_t* loc_lds = loc_all[wave];
  uint16_t* row_ent = row_ent_all[wave];
  uint32_t* row_anchor = row_anchor_all[wave];
  auto div_r = [&](uint32_t n) -> uint32_t {
    const uint32_t hi = __umulhi(wp.m, n);
    return (((n - hi) >> wp.sh1) + hi) >> wp.sh2;
  };
  const uint32_t first_row = div_r(wlo);
  const uint32_t wend = (woff0 + span - 1u < wp.total) ? woff0 + span - 1u : wp.total - 1u;
  const uint32_t last_row = div_r(wend);
  const int n_here = (int)(last_row - first_row + 1u);
  const int n_stage = n_here + 1;      // (the row after: a chunk may run over into it)

  // ---- the rows' indices: HBM loads, issued before anything else
  int64_t ti[kRowIter], ei[kRowIter];
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    uint32_t row = first_row + (uint32_t)(lane + it * kWave);
    row = row < wp.n_rows ? row : wp.n_rows - 1u;      // clamp: entry unused
    ti[it] = ei[it] = 0;
    if (it == 0 || n_stage > it * kWave) {
      if constexpr (kSrc == CAMPX_WINDOWS_PAIRS) {
        if (wp.idx64) {
          ti[it] = static_cast<const int64_t*>(wp.t_idx)[row];
          ei[it] = static_cast<const int64_t*>(wp.e_idx)[row];
        } else {
          ti[it] = static_cast<const int32_t*>(wp.t_idx)[row];
          ei[it] = static_cast<const int32_t*>(wp.e_idx)[row];
        }
      } else if constexpr (kSrc == CAMPX_WINDOWS_TRACE) {
        const uint32_t t = row / (uint32_t)wp.B;       // (N = T * B < 2^32)
        ti[it] = t;
        ei[it] = row - t * (uint32_t)wp.B;
      } else {
        ti[it] = row;
        if (wp.t_idx) {
          if (wp.idx64) ti[it] = static_cast<const int64_t*>(wp.t_idx)[row];
          else ti[it] = static_cast<const int32_t*>(wp.t_idx)[row];
        }
      }
    }
  }

  // ---- the scenery's layer per cell (plain, pieces): once per wave, 16 bytes a lane
  u32x4 loc16 = {0u, 0u, 0u, 0u};
  if constexpr (!kVar) loc16 = *reinterpret_cast<const u32x4*>(wp.loc + lane * 16);

  // ---- indices -> clamped position -> the row's entry of every plane
  int bad = 0;
  uint16_t ent[kRowIter][kPlanes];
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    const int i = lane + it * kWave;
    const bool staged = it == 0 || n_stage > it * kWave;
    int64_t t = ti[it], e = ei[it];
    bool out_of_range;
    if constexpr (kSrc == CAMPX_WINDOWS_STATES) out_of_range = t < 0 || t >= wp.n_states;
    else out_of_range = t < 0 || t >= wp.T || e < 0 || e >= wp.B;
    // a row is counted by the one wave whose window it STARTS in
    bad += (out_of_range && i < n_here && (first_row + (uint32_t)i) * wp.R >= wlo) ? 1 : 0;
    if constexpr (kSrc == CAMPX_WINDOWS_STATES) {
      t = out_of_range ? 0 : t;
      u32x4 c = {0u, 0u, 0u, 0u};
      if (staged) c = wp.cells[t];
      ent[it][0] = (uint16_t)c.x;
      ent[it][1] = (uint16_t)(c.x >> 16);
      ent[it][2] = (uint16_t)c.y;
      ent[it][3] = (uint16_t)(c.y >> 16);
      ent[it][4] = (uint16_t)c.z;
      ent[it][5] = (uint16_t)(c.z >> 16);
      ent[it][6] = (uint16_t)c.w;
      ent[it][7] = (uint16_t)(c.w >> 16);
    } else {
      t = t < 0 ? 0 : (t >= wp.T ? wp.T - 1 : t);
      e = e < 0 ? 0 : (e >= wp.B ? wp.B - 1 : e);
      const int64_t at = t * wp.pitch + e;
#pragma unroll
      for (int d = 0; d < kPlanes; ++d) {
        ent[it][d] = 0;
        if (staged && d < wp.n_planes) ent[it][d] = wp.trace[(int64_t)d * wp.plane + at];
      }
    }
  }
  if (bad) {
    if (wp.bad_count) atomicAdd(wp.bad_count, bad);
    if (wp.bad_flag) __hip_atomic_store(wp.bad_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // the row's anchor: where its h x w window starts on the board (and which variant it shows)
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    const int i = lane + it * kWave;
    if ((it == 0 || n_stage > it * kWave) && i < n_stage) {
      int r0 = wp.r0, c0 = wp.c0;
      uint32_t centre = 0;
#pragma unroll
      for (int d = 0; d < kPlanes; ++d) centre = d == wp.thing ? (uint32_t)ent[it][d] : centre;
      if (wp.thing >= 0) {
        uint32_t cell = centre & 0x3ffu;
        cell = cell < (uint32_t)wp.HW ? cell : (uint32_t)wp.HW - 1u;
        const uint32_t cy = (cell * wp.mW) >> 20;
        r0 = (int)cy - (wp.h >> 1);
        c0 = (int)(cell - cy * (uint32_t)wp.W) - (wp.w >> 1);
      }
      uint32_t variant = 0;
      if constexpr (kVar) {
        uint32_t v = 0;
#pragma unroll
        for (int d = 0; d < kPlanes; ++d) v = d == wp.n_dyn ? (uint32_t)ent[it][d] : v;
        v &= 0x3ffu;
        const uint32_t vmax = (uint32_t)wp.n_variants - 1u;
        variant = v < vmax ? v : vmax;     // (a trace from anywhere: nothing is read outside the tables)
      }
      row_anchor[i] = pack_anchor(r0, c0, variant);
#pragma unroll
      for (int d = 0; d < kPlanes; ++d)
        if (d < wp.n_planes) row_ent[i * kPlanes + d] = ent[it][d];
    }
  }
  if constexpr (!kVar) *reinterpret_cast<u32x4*>(loc_lds + lane * 16) = loc16;
  __builtin_amdgcn_wave_barrier();

  // ---- fill: every byte of the chunks this lane will store
  const uint32_t pad = (uint32_t)wp.pad;
#pragma unroll
  for (int j = 0; j < kWin; ++j) {
    const uint32_t off = woff0 + j * 1024u + (uint32_t)lane * 16u;
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    // A chunk that starts before the output: offsets are multiples of 16 with int8 (the output is
    // 16-byte aligned), so there the chunk before the output holds none of it; with the 16-bit
    // formats they are multiples of 8 ELEMENTS, and for an output at 16 (mod 32) bytes the chunk
    // at -8 holds row 0's first 8 bytes in its upper half - which the store loop's half at
    // element 0 reads.  It is filled as the chunk at 0 and moved up below.
    const bool before = kFmt != 0 && off == 0u - 8u;
    const uint32_t from = before ? 0u : off;
    if (from < wp.total) {     // (other chunks before the output wrap to huge offsets and fail this too)
      const uint32_t row = div_r(from);
      const uint32_t k = from - row * wp.R;
      uint32_t i = row - first_row;
      uint32_t l = k / (uint32_t)wp.hw;
      const uint32_t rem = k - l * (uint32_t)wp.hw;
      uint32_t y = rem / (uint32_t)wp.w;
      uint32_t x = rem - y * (uint32_t)wp.w;
      uint32_t anchor = row_anchor[i];
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int by = (int)(anchor & 0x3ffu) - 256 + (int)y;
        const int bxx = (int)((anchor >> 10) & 0x3ffu) - 256 + (int)x;
        const bool on = (uint32_t)by < (uint32_t)wp.H && (uint32_t)bxx < (uint32_t)wp.W;
        const uint32_t cell = on ? (uint32_t)(by * wp.W + bxx) : 0u;
        uint32_t layer;
        if constexpr (kVar) layer = wp.loc[(anchor >> 20) * CAMPX_WIDE_MAX_CELLS + cell];
        else layer = loc_lds[cell];
        layer = on ? layer : pad;
        word[b >> 2] |= (layer == l ? 1u : 0u) << ((b & 3) * 8);
        // the next byte: x, then y, then the layer, then the row
        ++x;
        const bool wx = x == (uint32_t)wp.w;
        x = wx ? 0u : x;
        y += wx ? 1u : 0u;
        const bool wy = y == (uint32_t)wp.h;
        y = wy ? 0u : y;
        l += wy ? 1u : 0u;
        if (l == (uint32_t)wp.L) {      // (i + 1 <= n_here: the row after is staged)
          l = 0u;
          ++i;
          anchor = row_anchor[i];
        }
      }
    }
    if (before) {
      word[2] = word[0];
      word[3] = word[1];
      word[0] = word[1] = 0u;
    }
    *reinterpret_cast<u32x4*>(win0 + j * 1024 + lane * 16) = u32x4{word[0], word[1], word[2], word[3]};
  }
  __builtin_amdgcn_wave_barrier();

  // ---- patches: per row of the window, per thing, one byte cleared and one set - where the
  // thing's cell is inside the row's h x w window
#pragma unroll
  for (int it = 0; it < kRowIter; ++it) {
    const int i = lane + it * kWave;
    if (it > 0 && n_here <= it * kWave) break;
    const bool mine = i < n_here;
    // (a patch left of the wave's window wraps to a huge unsigned value and fails the one comparison)
    const uint32_t row0 = (first_row + (uint32_t)i) * wp.R - woff0;
    const uint32_t anchor = mine ? row_anchor[i] : 0u;
    const int r0 = (int)(anchor & 0x3ffu) - 256, c0 = (int)((anchor >> 10) & 0x3ffu) - 256;
    for (int d = 0; d < wp.n_dyn; ++d) {
      const uint32_t e = mine ? (uint32_t)row_ent[i * kPlanes + d] : 0u;
      const uint32_t cell = e & 0x3ffu;
      const uint32_t cy = (cell * wp.mW) >> 20;
      const uint32_t py = (uint32_t)((int)cy - r0), px = (uint32_t)((int)(cell - cy * (uint32_t)wp.W) - c0);
      const uint32_t p = py * (uint32_t)wp.w + px;
      const uint32_t a = row0 + (uint32_t)wp.dyn_layer[d] * (uint32_t)wp.hw + p;
      const uint32_t b = row0 + ((e >> 10) & 0xfu) * (uint32_t)wp.hw + p;
      if (mine && (e >> 15) != 0 && cell < (uint32_t)wp.HW && py < (uint32_t)wp.h && px < (uint32_t)wp.w) {
        if (b < span) win0[b] = 0;
        if (a < span) win0[a] = 1;
      }
    }
    if constexpr (kMask) {
      const uint32_t shown = mine ? (uint32_t)row_ent[i * kPlanes + wp.n_dyn] : 0u;
      for (int q = 0; q < wp.n_pieces; ++q) {
        const uint32_t piece = wp.pieces[q];
        const uint32_t py = (uint32_t)((int)((piece >> 8) & 0xffu) - r0), px = (uint32_t)((int)(piece & 0xffu) - c0);
        const uint32_t p = py * (uint32_t)wp.w + px;
        const uint32_t a = row0 + ((piece >> 16) & 0xffu) * (uint32_t)wp.hw + p;
        const uint32_t b = row0 + (piece >> 24) * (uint32_t)wp.hw + p;
        if (((shown >> q) & 1u) && py < (uint32_t)wp.h && px < (uint32_t)wp.w) {
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
      if (off < wp.total) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(win0 + j * 1024 + lane * 16);
        if (off + 16u > wp.total) {
          const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
          for (uint32_t i = 0; off + i < wp.total; ++i) dst[off + i] = (int8_t)(w4[i >> 2] >> ((i & 3u) * 8u));
        } else if (wp.nt) {
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
    for (int hh = 0; hh < 2 * kWin; ++hh) {
      const uint32_t elem = woff0 + (uint32_t)hh * 512u + (uint32_t)lane * 8u;
      if (elem < wp.total) {
        const uint2 b = *reinterpret_cast<const uint2*>(win0 + hh * 512 + lane * 8);
        u32x4 v;
        v.x = ((b.x & 0xffu) | ((b.x << 8) & 0x00ff0000u)) * kOne;
        v.y = (((b.x >> 16) & 0xffu) | ((b.x >> 8) & 0x00ff0000u)) * kOne;
        v.z = ((b.y & 0xffu) | ((b.y << 8) & 0x00ff0000u)) * kOne;
        v.w = (((b.y >> 16) & 0xffu) | ((b.y >> 8) & 0x00ff0000u)) * kOne;
        if (elem + 8u > wp.total) {
          const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
          for (uint32_t i = 0; elem + i < wp.total; ++i)
            dst16[elem + i] = (uint16_t)(w4[i >> 1] >> ((i & 1u) * 16u));
        } else if (wp.nt) {
          store16_streaming(reinterpret_cast<u32x4*>(dst16 + elem), v);
        } else {
          *reinterpret_cast<u32x4*>(dst16 + elem) = v;
        }
      }
    }
  }
}

// The twenty-seven instances, at [kScen][kSrc][kFmt]: the request's `source` and `obs_format` are
// the indices.
static_assert(CAMPX_WINDOWS_PAIRS == 0 && CAMPX_WINDOWS_TRACE == 1 && CAMPX_WINDOWS_STATES == 2 &&
                  CAMPX_OBS_INT8 == 0 && CAMPX_OBS_F16 == 1 && CAMPX_OBS_BF16 == 2,
              "kSrc is CampxWindows.source, kFmt is obs_format");
using WindowKernel = decltype(&window_kernel<0, 0, 0>);
static const WindowKernel kWindowKernels[3][3][3] = {
    {{window_kernel<0, 0, 0>, window_kernel<1, 0, 0>, window_kernel<2, 0, 0>},
     {window_kernel<0, 1, 0>, window_kernel<1, 1, 0>, window_kernel<2, 1, 0>},
     {window_kernel<0, 2, 0>, window_kernel<1, 2, 0>, window_kernel<2, 2, 0>}},
    {{window_kernel<0, 0, 1>, window_kernel<1, 0, 1>, window_kernel<2, 0, 1>},
     {window_kernel<0, 1, 1>, window_kernel<1, 1, 1>, window_kernel<2, 1, 1>},
     {window_kernel<0, 2, 1>, window_kernel<1, 2, 1>, window_kernel<2, 2, 1>}},
    {{window_kernel<0, 0, 2>, window_kernel<1, 0, 2>, window_kernel<2, 0, 2>},
     {window_kernel<0, 1, 2>, window_kernel<1, 1, 2>, window_kernel<2, 1, 2>},
     {window_kernel<0, 2, 2>, window_kernel<1, 2, 2>, window_kernel<2, 2, 2>}}};

// What campx_wide_render_windows_launch() asks of a request; before anything touches a device.
static int32_t windows_check(const CampxWideSpec* s, const void* tables, const void* loc,
                             const CampxWindows* q, int64_t B) {
  if (!s || !tables || !loc || !q || !q->obs) return CAMPX_EINVAL;
  const int32_t v = wide_validate_plain(s);
  if (v != CAMPX_OK) return v;
  if (q->source < CAMPX_WINDOWS_PAIRS || q->source > CAMPX_WINDOWS_STATES) return CAMPX_EINVAL;
  if ((reinterpret_cast<uintptr_t>(q->obs) & 15) || (reinterpret_cast<uintptr_t>(loc) & 15) ||
      (reinterpret_cast<uintptr_t>(tables) & 15) || (reinterpret_cast<uintptr_t>(q->bad_count) & 3) ||
      (reinterpret_cast<uintptr_t>(q->bad_flag) & 3))
    return CAMPX_EINVAL;
  if (q->obs_format < CAMPX_OBS_INT8 || q->obs_format > CAMPX_OBS_BF16) return CAMPX_EINVAL;
  if (q->N <= 0) return CAMPX_EINVAL;
  if (q->h < 1 || q->w < 1 || q->h > 2 * s->rows - 1 || q->w > 2 * s->cols - 1) return CAMPX_EINVAL;
  const int64_t Rw = (int64_t)s->n_layers * q->h * q->w;
  if (Rw < 16) return CAMPX_EINVAL;
  if (q->N > ((1ll << 32) - 65536 - 1) / Rw) return CAMPX_EINVAL;
  if (q->anchor == CAMPX_WINDOW_ON_THING) {
    if (q->thing < 0 || q->thing >= s->n_dyn) return CAMPX_EINVAL;
  } else if (q->anchor == CAMPX_WINDOW_FIXED) {
    if (q->r0 < -255 || q->r0 > 255 || q->c0 < -255 || q->c0 > 255) return CAMPX_EINVAL;
  } else {
    return CAMPX_EINVAL;
  }
  if (q->pad_layer < -1 || q->pad_layer >= s->n_layers) return CAMPX_EINVAL;
  const uintptr_t idx_align = q->idx64 ? 7 : 3;
  if (q->source == CAMPX_WINDOWS_STATES) {
    if (reinterpret_cast<uintptr_t>(q->state_ids) & idx_align) return CAMPX_EINVAL;
    return CAMPX_OK;
  }
  // the trace: what gather_check() imposes (the whole trace brings no index arrays)
  if (!q->trace || B <= 0 || q->T <= 0) return CAMPX_EINVAL;
  if (reinterpret_cast<uintptr_t>(q->trace) & 1) return CAMPX_EINVAL;
  if (q->source == CAMPX_WINDOWS_PAIRS) {
    if (!q->t_idx || !q->e_idx) return CAMPX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(q->t_idx) | reinterpret_cast<uintptr_t>(q->e_idx)) & idx_align)
      return CAMPX_EINVAL;
  }
  if (q->pitch < B) return CAMPX_EINVAL;
  if (q->n_planes != wide_layout(*s).n_planes) return CAMPX_EINVAL;
  if (q->T > (1ll << 40) / q->pitch) return CAMPX_EINVAL;
  if (q->n_planes > 1 && q->plane < q->T * q->pitch) return CAMPX_EINVAL;
  if (q->source == CAMPX_WINDOWS_TRACE && (B > (1ll << 32) / q->T || q->N != q->T * B)) return CAMPX_EINVAL;
  return CAMPX_OK;
}

}  // namespace campx_impl

using namespace campx_impl;

extern "C" {

int32_t campx_wide_render_windows_launch(const CampxWideSpec* s, const void* tables_dev,
                                         const void* layer_of_cell, const CampxWindows* q, int64_t B,
                                         void* stream) {
  const int32_t rc = windows_check(s, tables_dev, layer_of_cell, q, B);
  if (rc != CAMPX_OK) return rc;
  const WideTables t = wide_tables(*s, tables_dev);
  const WideLayout& lay = t.lay;
  const int HW = s->rows * s->cols;
  const int64_t Rw = (int64_t)s->n_layers * q->h * q->w;
  const GatherPlan plan = gather_plan(q->N, Rw, q->obs_format, reinterpret_cast<uintptr_t>(q->obs));
  WindowParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.R = (uint32_t)Rw;
  wp.m = plan.m;
  wp.sh1 = plan.sh1;
  wp.sh2 = plan.sh2;
  wp.total = plan.total;
  wp.shift = plan.shift;
  wp.n_rows = (uint32_t)q->N;
  wp.n_dyn = s->n_dyn;
  wp.n_planes = lay.n_planes;
  wp.n_variants = lay.n_variants;
  wp.n_pieces = s->n_pieces;
  wp.H = s->rows;
  wp.W = s->cols;
  wp.HW = HW;
  wp.L = s->n_layers;
  wp.h = q->h;
  wp.w = q->w;
  wp.hw = q->h * q->w;
  wp.mW = (uint32_t)(((1u << 20) + (uint32_t)s->cols - 1u) / (uint32_t)s->cols);
  wp.thing = q->anchor == CAMPX_WINDOW_ON_THING ? q->thing : -1;
  wp.r0 = q->r0;
  wp.c0 = q->c0;
  wp.pad = q->pad_layer < 0 ? 0xff : q->pad_layer;
  wp.idx64 = q->idx64 ? 1 : 0;
  wp.nt = q->streaming ? 1 : 0;
  wp.n_states = s->n_states;
  wp.B = B;
  wp.T = q->T;
  wp.pitch = q->pitch;
  wp.plane = q->plane;
  for (int d = 0; d < s->n_dyn; ++d) wp.dyn_layer[d] = s->dyn_layer[d];
  for (int p = 0; p < s->n_pieces; ++p) {
    const uint32_t cell = s->piece_cell[p];
    wp.pieces[p] = (cell % (uint32_t)s->cols) | ((cell / (uint32_t)s->cols) << 8) |
                   ((uint32_t)s->piece_layer[p] << 16) | ((uint32_t)s->static_top_layer[cell] << 24);
  }
  wp.loc = static_cast<const uint8_t*>(layer_of_cell);
  wp.trace = static_cast<const uint16_t*>(q->trace);
  wp.cells = t.cells;
  wp.t_idx = q->source == CAMPX_WINDOWS_STATES ? q->state_ids : q->t_idx;
  wp.e_idx = q->e_idx;
  wp.bad_count = q->bad_count;
  wp.bad_flag = q->bad_flag;
  const dim3 grid(plan.grid), block(kWindowWaves * kWave);
  int8_t* dst = static_cast<int8_t*>(q->obs);
  const int scen = lay.n_variants > 1 ? 1 : (s->n_pieces > 0 ? 2 : 0);
  hipLaunchKernelGGL(kWindowKernels[scen][q->source][q->obs_format], grid, block, 0,
                     static_cast<hipStream_t>(stream), wp, dst);
  return launch_status();
}

int32_t campx_wide_render_windows_plan(int64_t N, int32_t Rw, int32_t obs_format, uint64_t dst_addr,
                                       int64_t* plan_out) {
  if (!plan_out || N <= 0 || Rw < 16 || Rw > CAMPX_MAX_LAYERS * 253 * 253 ||
      obs_format < CAMPX_OBS_INT8 || obs_format > CAMPX_OBS_BF16 || (dst_addr & 15) ||
      N > ((1ll << 32) - 65536 - 1) / Rw)
    return CAMPX_EINVAL;
  const GatherPlan p = gather_plan(N, Rw, obs_format, dst_addr);
  plan_out[0] = p.m;
  plan_out[1] = p.sh1;
  plan_out[2] = p.sh2;
  plan_out[3] = p.total;
  plan_out[4] = p.shift;
  plan_out[5] = p.grid;
  plan_out[6] = obs_format ? 1024 : 2048;
  plan_out[7] = kWindowWaves;
  return CAMPX_OK;
}

}  // extern "C"
