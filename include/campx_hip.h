/*
 * campx_hip.h - C ABI of libcampx_hip.so, the MI355X (gfx950) batched grid-world
 * step/render engine.
 *
 * The reference (OpenMined/CampX) is pure Python and has no FFI; its hot path is
 * the per-frame call chain
 *
 *     Engine.play                      campx/engine.py:114-166
 *       Engine._update_and_render      campx/engine.py:168-208
 *         <entity>.update(...)         examples/boat_race.py:35-59, 69-91
 *         Engine._render               campx/engine.py:295-324
 *           BaseObservationRenderer.*  campx/rendering.py:104-219
 *       Engine._apply_and_clear_plot   campx/engine.py:211-293
 *
 * which produces, for ONE environment, `(Observation(board, layers,
 * layered_board), reward, discount)`.  The entry points below are what a binding
 * for that path binds instead: the same function for B environments at once,
 * for T consecutive frames per call, on device buffers the caller owns.
 * INTEGRATION.md shows the ctypes stub a CampX maintainer would add.
 *
 * Conventions
 *   - plain C, no exceptions: every function returns CAMPX_OK (0) or a negative
 *     CAMPX_E* code; campx_strerror() names it.
 *   - the library owns no memory between calls: all buffers are caller-allocated DEVICE
 *     memory unless a parameter says "host".  The only process-wide state: the settings
 *     (campx_config_set / _get / _string below: one table, no environment variable but
 *     CAMPX_CONFIG) and - read-only after first use - per device, its CU count and the
 *     dynamic-LDS limit already granted to a kernel.
 *   - launches are asynchronous on the hipStream_t passed as `void* stream`
 *     (NULL = the default stream); nothing in here synchronises.
 *   - re-entrant; calls on distinct state buffers may be issued concurrently.
 */
#ifndef CAMPX_HIP_H_
#define CAMPX_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAMPX_SPEC_MAGIC 0x58504d43u /* 'CMPX' */
#define CAMPX_SPEC_VERSION 1u

#define CAMPX_MAX_CELLS 128  /* rows * cols */
#define CAMPX_MAX_LAYERS 16  /* characters of a game = channels of layered_board */
#define CAMPX_MAX_DYN 4      /* one-cell things that move (agents, boxes) */
#define CAMPX_MAX_STATIC 16  /* drapes whose mask never changes */
#define CAMPX_MAX_RULES 16
#define CAMPX_N_ACTIONS 5    /* left, right, up, down, stay (examples/boat_race.py:26) */

enum {
  CAMPX_OK = 0,
  CAMPX_EINVAL = -1,   /* NULL / misaligned / out-of-range argument */
  CAMPX_ESPEC = -2,    /* GameSpec fails validation */
  CAMPX_ELAUNCH = -3,  /* HIP refused the launch (see campx_last_hip_error) */
  CAMPX_ENODEV = -4,   /* no gfx950 device */
  CAMPX_ENOMEM = -5    /* host scratch allocation failed (set-up calls only) */
};

enum { CAMPX_OBS_INT8 = 0, CAMPX_OBS_F16 = 1, CAMPX_OBS_BF16 = 2 };

/* Rule opcodes: the update() bodies of the reference's example entities. */
enum {
  /* Move dynamic thing `dyn` one cell by the action, cyclically; if the cell it
   * would enter SHOWED (at the latest repaint) a character in `block_layers`,
   * it returns to the cell it was painted at.  Optional reward: `base`
   * (+1 when the entered cell showed a character in `reward_layers`).
   * examples/boat_race.py:35-59; Demo 1/2/3 cell 3. */
  CAMPX_OP_AGENT = 1,
  /* reward = base + [the cell dynamic thing `dyn` is in now showed layer `aux`
   * at the latest repaint] * bonus[action].  examples/boat_race.py:69-91. */
  CAMPX_OP_DIR_HOVER = 2,
  /* Box `dyn` moves one cell by the action if agent `aux`'s painted position,
   * moved by the action, is the box's cell and the cell beyond showed no
   * character of `block_layers`.  campx_amd/rules.py BoxDrape. */
  CAMPX_OP_BOX = 3,
  /* reward = base + [dynamic thing `dyn` stands on static drape `aux`] *
   * bonus[0]; if it does, the episode terminates with discount 0.
   * campx_amd/rules.py GoalDrape. */
  CAMPX_OP_GOAL = 4
};

typedef struct CampxRule {
  int32_t op;
  int32_t end_group;      /* 1 = a repaint follows this rule (campx/engine.py:208) */
  int32_t dyn;
  int32_t aux;
  uint32_t block_layers;  /* bit l = layer l */
  uint32_t reward_layers;
  int32_t has_reward;     /* rule calls Plot.add_reward (campx/plot.py:186) */
  float base;
  float bonus[CAMPX_N_ACTIONS];
  int32_t reserved[3];
} CampxRule;              /* 64 bytes */

/* One entry of the (cell, action) transition table of a one-mover game. */
typedef struct CampxTransition {
  float reward;       /* summed reward of the frame (NaN = None) */
  uint8_t next_cell;  /* row * cols + col after the frame */
  uint8_t done;       /* bit 0: the episode terminated on the frame; bits 4-7: discount code c:
                         the frame reports spec.discount_list[c], or - c == 0 - the default,
                         0.0 when it terminated and 1.0 otherwise (campx/plot.py:161-184,
                         232-257) */
  int8_t perf;        /* hidden performance of the frame (perf_scale * code + perf_offset) */
  uint8_t paint;      /* how the mover paints at next_cell: bits 0-6 the scenery layer it
                         covers there, bit 7 set when the scenery hides it instead */
} CampxTransition;    /* 8 bytes */

/*
 * GameSpec: the immutable description of one game, produced once per game by the
 * host (campx_amd/gamespec.py from the ascii_art_to_game() arguments,
 * campx/ascii_art.py:60-309) and uploaded by the caller to device memory.
 * Plain data, no pointers, same bytes on host and device.
 */
typedef struct CampxSpec {
  uint32_t magic, version;
  int32_t rows, cols;
  int32_t n_layers;                     /* L; layer l shows character layer_char[l], ascending */
  int32_t n_dyn;                        /* K */
  int32_t n_static;
  int32_t n_rules;
  int32_t any_reward;                   /* 0: nobody ever calls add_reward -> reward is NaN (None) */
  int32_t table_valid;                  /* 1: `table` below is filled (campx_spec_compile) */
  int32_t render_valid;                 /* 1: `rot_obs` / `rot_board` below are filled */
  int32_t perf_dyn;                     /* moving thing whose hidden performance is scored, or -1 */
  int32_t perf_n;                       /* length n of the cycle of cell classes (>= 2) */
  int32_t table_only;                   /* 1: `rules` is empty and the update pass exists only as
                                           tables the HOST filled by running the game's own Python
                                           update() bodies over every reachable state
                                           (campx_amd/tabulate.py: `table` for one mover,
                                           campx_pair_table_pack() for two to four).  Calls that
                                           would interpret the rules return CAMPX_ESPEC. */
  int32_t reserved0[2];
  uint8_t layer_char[CAMPX_MAX_LAYERS];
  int32_t dyn_layer[CAMPX_MAX_DYN];     /* layer painted by dynamic thing d */
  int32_t dyn_z[CAMPX_MAX_DYN];         /* its z rank, 1 = rearmost thing (0 = backdrop).  A
                                           host-tabulated game (table_only) may give its LAST
                                           things rank 0: values the tables are indexed by that
                                           are never painted - the z-order in force of a game
                                           that calls Plot.change_z_order (campx/plot.py:121-159),
                                           whose effect on the screen is in the table entries'
                                           "is the character its cell shows" bits */
  int32_t dyn_row0[CAMPX_MAX_DYN];      /* position in the art */
  int32_t dyn_col0[CAMPX_MAX_DYN];
  CampxRule rules[CAMPX_MAX_RULES];     /* update-schedule order */
  /* Per cell, considering the backdrop and the static drapes only: */
  uint8_t static_top_layer[CAMPX_MAX_CELLS]; /* layer of the front-most one */
  uint8_t static_top_z[CAMPX_MAX_CELLS];     /* its z rank (0 = backdrop) */
  uint16_t static_cover[CAMPX_MAX_CELLS];    /* bit s = static drape s covers the cell */
  /* layered board of the static scenery alone, [L][rows*cols] 0/1 */
  int8_t obs_template[CAMPX_MAX_LAYERS * CAMPX_MAX_CELLS];
  /* Games with ONE moving thing: the whole update pass of a frame is a function of
   * (cell the thing is in, action).  campx_spec_compile() tabulates it by running
   * the rule interpreter kernel once over every (cell, action) pair; the frame
   * loop then does one lookup instead of interpreting the rules.
   * Index: cell * CAMPX_N_ACTIONS + action. */
  CampxTransition table[CAMPX_MAX_CELLS * CAMPX_N_ACTIONS];
  /* For the render kernel of the two-kernel path, filled by campx_spec_compile():
   * 16 byte-rotations of the scenery's row (the layered board, resp. the flat board,
   * of the static scenery), each continued cyclically, so that any 16 consecutive
   * bytes of back-to-back rows are one aligned 16-byte load:
   *   rot[r * pitch + j] = row[(j + r) mod R],  pitch = round_up(R, 16) + 16,
   * R = L*rows*cols (rot_obs) or rows*cols (rot_board).  16-byte aligned in the blob. */
  int8_t rot_obs[16 * (CAMPX_MAX_LAYERS * CAMPX_MAX_CELLS + 16)];
  int8_t rot_board[16 * (CAMPX_MAX_CELLS + 16)];
  /* Hidden performance (examples/boat_race.py:117-151): class 1..perf_n of each cell,
   * 0 = none.  A frame scores +1 when thing perf_dyn goes from class i to class i+1
   * (cyclically), -1 for the reverse, else 0. */
  uint8_t cell_class[CAMPX_MAX_CELLS];
  /* Two kinds of hidden performance, both a small code per frame that the state tables
   * carry in 3 bits; the value written to CampxOutputs.perf is perf_scale * code + perf_offset.
   *   perf_mode 0  progress round a cycle of cell classes (above): code = progress + 1,
   *                scale 1, offset -1.
   *   perf_mode 1  a penalty for where things stand: code = sum over the moving things in
   *                perf_mask (bit d = thing d) of cell_class[its cell], at most 7 - the
   *                side-effects penalty of sokoban (-5 for a box next to a
   *                wall, -10 for a box in a corner: classes 1 and 2, perf_scale -5).
   * perf_dyn >= 0 says that the game has a hidden performance at all (mode 1: any thing
   * of perf_mask). */
  int32_t perf_mode, perf_mask, perf_scale, perf_offset;
  /* Discounts other than the default (Plot.change_default_discount, terminate_episode(d):
   * campx/plot.py:161-184, 232-257): code -> value, codes 1..15; code 0 is the default.
   * Only host-tabulated games (table_only) produce them. */
  float discount_list[16];
} CampxSpec;

/* Dynamic state of B environments, struct-of-arrays, DEVICE pointers. */
typedef struct CampxState {
  int8_t* pos;     /* [2*K, B]: plane 2d = row of dynamic thing d, 2d+1 = its column */
  uint8_t* done;   /* [B] game-over latch (campx/engine.py:285); a latched environment is
                      rebuilt from the art before its next action is applied */
  float* ret;      /* [B] return accumulated since the last rebuild, or NULL */
  const void* pair_table; /* optional, games with two to four moving things: the device table
                      campx_pair_table_build() filled; lets the two-kernel path look the
                      update pass up instead of interpreting the rules.  NULL = interpret. */
} CampxState;

/* Per-frame outputs, DEVICE pointers; any of them except `obs` may be NULL.
 * Frame t of a call is written at  base + t * <t_stride>  (in elements); a stride
 * of 0 makes every frame overwrite the first slot, so only the last survives. */
/* Bits of *CampxOutputs.error_flag. */
#define CAMPX_ERR_FLOW_TIMEOUT 1

/* What the library remembers about a scratch block of one-launch rollouts - in the CALLER's
 * memory (CampxOutputs.flow_state), so that the library holds no state of its own. */
typedef struct CampxFlowState {
  int64_t tag;    /* 1..255, of the block's last launch; 0: none yet (the block is cleared first) */
  int64_t B, T;   /* what the block's entries were written for */
  int64_t pitch;  /* the row pitch they were written with */
  int64_t n_dyn;  /* how many movers' planes they were written for (a game with MORE movers on the
                     same block would find stale tags in the extra planes) */
  int64_t block;  /* the address of the block this state describes (a state handed over with
                     another block starts afresh) */
} CampxFlowState;

typedef struct CampxOutputs {
  int8_t* obs;        /* layered_board [*, B, L, rows, cols] 0/1 (campx/rendering.py:213-215);
                         16-byte aligned */
  int64_t obs_t_stride;
  int8_t* board;      /* flat board [*, B, rows, cols] of character codes (rendering.py:217) */
  int64_t board_t_stride;
  float* reward;      /* [T, B]; NaN where the reference returns None */
  float* discount;    /* [T, B] 1.0, or 0.0 on the frame the episode ended (plot.py:179-184) */
  uint8_t* done;      /* [T, B] game-over flag after the frame */
  int8_t* perf;       /* [T, B] hidden performance of the frame (-1, 0, +1), or NULL; needs
                         spec.perf_dyn >= 0 */
  uint8_t* trace;     /* optional [K, T, B]: for moving thing d at frame t in environment e,
                           bits 0-6  the cell (row*cols + col) it is in after the frame
                           bit  7    1 when it is the character that cell shows; when 0 it
                                     is hidden and changes nothing in the observation
                         A compact trajectory in its own right (1 byte per thing per frame
                         against L*rows*cols of observation); and when it is given, frames are
                         stored back to back (obs_t_stride == B*L*rows*cols; any batch size),
                         the library runs the update pass and the render as
                         two kernels, which streams the observations to HBM faster (DESIGN.md
                         "Kernels"); with strides of 0 (only the last frame survives) it
                         renders just that frame from the last row of the trace.  Written
                         only on that path. */
  int32_t obs_format; /* element type of `obs` (obs_t_stride counts elements):
                         CAMPX_OBS_INT8 0/1 bytes (the default, 0);
                         CAMPX_OBS_F16 / CAMPX_OBS_BF16: 0.0 / 1.0 in that format, the tensor
                         the reference's driver builds with `layered_board.view(-1).float()`
                         (examples/reinforce.py:123,149) handed over without a conversion
                         pass.  16-bit formats are produced by the render kernel (rollouts:
                         they need `trace` and back-to-back frames) and by the one-frame
                         kernels of games with their tables (T == 1);
                         anything else returns CAMPX_EINVAL. */
  int32_t* bad_count; /* optional device int32: += number of action ids outside 0..4 this call
                         consumed (the reference asserts sum(act) == 1 per step,
                         examples/boat_race.py:48; here the check rides in the kernel that
                         reads the actions anyway and the caller looks when it likes).  Never
                         reset by the library. */
  int32_t* bad_flag;  /* optional int32, device memory or host memory mapped into the device
                         (hipHostMalloc): set to 1, by a plain system-scope store, when the
                         call consumed any id outside 0..4.  Lets a host poll for bad
                         actions without a stream synchronisation. */
  int64_t scalar_pitch; /* elements from one frame's row to the next in reward, discount, done,
                         perf and trace (the planes of `trace` are then T * scalar_pitch
                         apart); 0 = B, rows back to back.  With a batch size that is not a
                         multiple of 16 a row of a [T, B] array starts at any byte, and the
                         update kernels' 16-byte stores are misaligned for most frames (legal,
                         but 4.3 instead of 7 TB/s: 47 instead of 16 us per 100 frames at
                         B = 65 535).  A caller can pad the arrays instead - [T, pitch] with
                         pitch = B rounded up to a multiple of 16, the first B elements of a
                         row used: every row then starts aligned and the kernels write whole
                         16-byte groups (the pad holds unspecified values).  `actions` and the
                         observation / board frames are never padded. */
  uint32_t* overlap_ctl; /* optional device scratch of campx_flow_scratch_bytes(B, T) bytes, 16-byte
                         aligned; NULL: two launches per rollout.  With it - AND `flow_state` AND
                         `error_flag` below - a rollout of a table game (one mover; two to four
                         with CampxState.pair_table) at a batch of at most 8 192 environments
                         (int8 observations of every frame, whole 16-byte chunks per frame) runs
                         as ONE launch whose update pass and render overlap: update workgroups
                         first, render workgroups behind them reading a tagged 16-bit copy of
                         each mover's trace kept in this block as the update role writes it
                         (csrc/k_update.hip, pipe_table_kernel<true>: 15 / 22 / 34 us against
                         20 / 27 / 38 at B = 1 024 / 4 096 / 8 192; pipe_multi_kernel<K, ., true>,
                         sokoban with one box: 23 / 30 / 44 against 28 / 35 / 46; the four-mover
                         level from 4 097 environments up).  Not while `stream` is being
                         captured into a graph.  Setting flow = 0 (campx_config_set): never.
                         Two launches that may run at the same time must not share a block.
                         campx_flow_shared() says whether a call will take this path. */
  int64_t overlap_ctl_bytes;
  struct CampxFlowState* flow_state; /* HOST memory, caller-owned, one per `overlap_ctl` block,
                         zero-initialised by the caller when the block is allocated and from then
                         on read and written only by the library, inside the launch call: the tag
                         of the block's last launch and the (B, T, row pitch, bytes) its entries
                         were written for (a launch with any of them changed first clears the
                         block, stream-ordered).  The library itself keeps NO state between
                         calls.  NULL: two launches per rollout. */
  int32_t* error_flag; /* int32, device memory or host memory mapped into the device: bits OR-ed in
                         (system scope) when a launch could not do what it was asked to, although
                         the call returned CAMPX_OK: CAMPX_ERR_FLOW_TIMEOUT - a render wave of a
                         one-launch rollout waited for trace entries of its own launch until it
                         gave up (seconds; two launches sharing one block at the same time is
                         the known way to get there) and wrote frames from stale entries: the
                         observations of that launch are WRONG.  Never cleared by the library.
                         Required for the one-launch path (NULL: two launches per rollout), so
                         that this failure cannot pass unseen. */
} CampxOutputs;

/* Size of CampxOutputs.overlap_ctl for rollouts of T frames of B environments (of any game: a
 * 16-byte header and, for each of up to CAMPX_MAX_DYN movers, T rows of B rounded up to 16 entries). */
int64_t campx_flow_scratch_bytes(int64_t B, int32_t T);

/* 1 when campx_rollout_launch() of T frames of B environments of this game, with a scratch
 * block, flow state and error flag supplied, int8 observations of every frame at a 16-byte
 * aligned address, rows of the per-frame streams `scalar_pitch` apart (0: B) and a stream that
 * is not being captured, runs as ONE launch (pipe_table_kernel<true>, pipe_multi_kernel<K, ., true>
 * - the latter given the game's pair / tuple table, which this query cannot see); 0 when it runs as an
 * update launch and a render launch.  The library's own bounds and environment knobs, for
 * callers that allocate the block only where it is used and for whoever reports which kernel
 * ran (bench.py). */
int32_t campx_flow_shared(const CampxSpec* spec_host, int64_t B, int32_t T, int64_t scalar_pitch);

/* sizeof(CampxSpec), for bindings that allocate the blob themselves. */
int32_t campx_spec_size(void);

/* Check a HOST GameSpec: magic/version, bounds, rule operands. */
int32_t campx_spec_validate(const CampxSpec* spec_host);

/*
 * Optional, once per game: derive the acceleration tables of a GameSpec.
 *   - rot_obs / rot_board (render_valid): host arithmetic on the scenery tables.
 *   - table (table_valid), only for n_dyn == 1: the rule interpreter kernel is run
 *     over all (cell, action) pairs on the current device.
 * Set-up time only: allocates and frees its own scratch device memory and
 * synchronises `stream`.  Upload the spec to the device AFTER this call.
 */
int32_t campx_spec_compile(CampxSpec* spec_host, void* stream);

/*
 * Games with TWO TO FOUR moving things: the update pass of a frame is a function of
 * (cell of thing 0, ..., cell of thing K-1, action).  campx_pair_table_bytes() is the
 * size of its table for this game (0 when n_dyn < 2, or the table would exceed 1 MiB for
 * two movers / 512 MiB for three and four); campx_pair_table_build() fills
 * caller-allocated DEVICE memory of that size by running the rule interpreter kernel over
 * every (cell, ..., cell, action) tuple, the same way campx_spec_compile() does for
 * one-mover games (set-up time only: scratch allocation + stream synchronisation inside;
 * about 19 bytes of host and of device scratch per tuple).  Returns CAMPX_ESPEC when a
 * frame of this game can pay more than 256 distinct rewards (the table indexes a reward
 * list).  Layout: 256 floats (reward list), then n = (rows*cols)^K * 5 entries, index
 * ((cell0 * rows*cols + cell1) * rows*cols + ...) * 5 + action.
 * Two movers, uint32 entries:
 *   bits 0-6 cell of thing 0 after the frame, 7-13 cell of thing 1, 14/15 whether
 *   thing 0 / 1 is the character its cell shows, 16 done, 17-18 and 31 the hidden-performance
 *   code (3 bits), 19-26 index into the reward list, 27-30 discount code.
 * Three and four movers, uint64 entries:
 *   bits 7d..7d+6 cell of thing d after the frame, 28+d whether it is the character its
 *   cell shows, 32 done, 33-34 and 43 the hidden-performance code, 35-42 index into the
 *   reward list, 44-47 discount code.
 */
int64_t campx_pair_table_bytes(const CampxSpec* spec_host);
int32_t campx_pair_table_build(const CampxSpec* spec_host, const CampxSpec* spec_dev,
                               void* table_dev, void* stream);

/*
 * The same table from HOST arrays instead of the rule interpreter: for games whose update()
 * bodies are arbitrary Python (the reference's own examples/boat_race.py:28-91 classes, a
 * user's Drapes), tabulated on the host by running them (campx_amd/tabulate.py).  With
 * n = (rows*cols)^K * 5 entries indexed as above:
 *   trace   [K][n]  thing d after the frame: cell | (it is the character its cell shows) << 7
 *   reward  [n]     summed reward of the frame, NaN = None (campx/plot.py:208-211)
 *   done    [n]     bit 0: the episode terminated on the frame; bits 4-7: discount code
 *                   (index into spec_host->discount_list; 0 = the default)
 *   perf    [n]     hidden performance (a value perf_scale * code + perf_offset), or NULL
 * Packs them into `table_dev` (campx_pair_table_bytes() bytes of device memory) and
 * synchronises `stream`.  CAMPX_ESPEC for more than 256 distinct rewards or a perf value
 * that is not one of the eight the spec's scale and offset give.
 */
int32_t campx_pair_table_pack(const CampxSpec* spec_host, const uint8_t* trace,
                              const float* reward, const uint8_t* done, const int8_t* perf,
                              void* table_dev, void* stream);

/*
 * Put B environments into the state its_showtime() leaves them in
 * (campx/engine.py:487-544: positions from the art, game-over clear, return 0)
 * and, if out->obs / out->board are non-NULL, write that first observation to
 * slot 0 of each.
 */
int32_t campx_reset_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev, CampxState state,
                           CampxOutputs out, int64_t B, void* stream);

/*
 * Advance B environments by T frames: T back-to-back Engine.play() calls for
 * each environment, with `actions[t*B + e]` (ids 0..4) the action of
 * environment e at frame t.  T = 1 is Engine.play().
 *
 * reset_first != 0 rebuilds every environment from the art before frame 0 (a
 * fresh make_game() per episode, examples/reinforce.py:122).
 * Action ids outside 0..4 are treated as 4 (stay) on the device; out.bad_count /
 * out.bad_flag (or campx_check_actions_launch()) detect them.  `actions` needs no padding:
 * nothing is read outside its T * B bytes.
 */
int32_t campx_rollout_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev,
                             CampxState state, const int8_t* actions, CampxOutputs out, int64_t B,
                             int32_t T, int32_t reset_first, void* stream);

/*
 * The two halves of campx_rollout_launch()'s two-kernel path, for callers that want to
 * overlap them across calls (the update pass of launch i+1 is a short, latency-bound
 * kernel that fits under the observation stream of launch i when issued on another
 * stream; campx_amd/fused.py `rollout(pipelined=True)`):
 *
 *   campx_update_launch   the update pass alone: reads state and actions, writes state,
 *                         out.trace (required) and the per-frame scalars out.reward /
 *                         discount / done / perf / bad_*; ignores out.obs / out.board.
 *   campx_render_launch   expands out.trace into out.obs (and out.board): frames back to
 *                         back (obs_t_stride == B*L*rows*cols) or only the last one
 *                         (strides 0), T <= 65535 (one grid row per frame), else
 *                         CAMPX_EINVAL.  Reads nothing but the trace and the spec.
 * update then render on one stream == campx_rollout_launch(), which in addition runs
 * launches whose trace planes (T*B bytes) exceed 28 MB as chunks of frames.
 */
int32_t campx_update_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev, CampxState state,
                            const int8_t* actions, CampxOutputs out, int64_t B, int32_t T,
                            int32_t reset_first, void* stream);
int32_t campx_render_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev, CampxOutputs out,
                            int64_t B, int32_t T, void* stream);

/*
 * Rollouts pipelined across calls: the update pass of one rollout (as campx_update_launch:
 * `actions`, `out`) together with the render pass of the rollout BEFORE it (as
 * campx_render_launch: `prev.trace` -> `prev.obs` / `prev.board`, same B and T), for callers
 * whose next actions do not depend on the observations they are waiting for (open-loop action
 * streams; the reference has no such call - it is Engine.play(), campx/engine.py:145-222,
 * T times for rollout i + 1 interleaved with the _render() calls, engine.py:286-324, of
 * rollout i).  For table games of ONE TO FOUR movers (one: the table in the spec; two to four:
 * the pair / tuple table in `state.pair_table`, round 5) with int8 observations of whole 16-byte
 * chunks per frame and no flat board, up to 32 768 environments and 2 GB of observations per
 * rollout, the two passes share ONE launch (update workgroups first, the others render);
 * otherwise they are issued one after the other on `stream`.  prev.trace == NULL: the update
 * pass alone.
 */
int32_t campx_update_render_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev,
                                   CampxState state, const int8_t* actions, CampxOutputs out,
                                   CampxOutputs prev, int64_t B, int32_t T, int32_t reset_first,
                                   void* stream);
/* 1 if campx_update_render_launch() puts the two passes of such rollouts (int8 observations of
 * every frame, no flat board) in one launch, 0 if it would issue them one after the other - in
 * which case a caller does better not to defer at all: campx_rollout_launch() renders a trace
 * that is still cached, a deferred render reads one that a whole launch has since evicted
 * (boat race, B = 200 000: 0.67 of peak against 0.83).  For a game of two to four movers the
 * answer assumes its table in CampxState.pair_table (without one: one after the other). */
int32_t campx_update_render_shared(const CampxSpec* spec_host, int64_t B, int32_t T);

/*
 * ---- Shape tier --------------------------------------------------------------------
 * Games made only of rigidly translated things that interact with nothing: the
 * reference's Hello World (examples/Hello World Example.ipynb cell 3: RollingDrape
 * `np.roll`s its whole mask, SlidingSprite moves diagonally, action 4 quits).  A thing
 * is a set of art cells plus a cyclic (row, col) offset that the action changes; things
 * may cover many cells and boards go up to CAMPX_SHAPE_MAX_CELLS cells, so these games
 * have their own spec and kernel (one wavefront per environment).
 *
 * Rendering follows campx/engine.py:295-324 and campx/rendering.py:104-219 including
 * the renderer's aliasing: paint_all_of() makes the canvas share the backdrop's storage
 * (rendering.py:128) until the first paint_drape rebinds it (rendering.py:178), so
 * sprites painted BEFORE the first drape in z-order are written into the backdrop for
 * good and leave trails.  The backdrop is therefore per-environment state here.
 */
#define CAMPX_SHAPE_SPEC_MAGIC 0x50485343u /* 'CSHP' */
#define CAMPX_SHAPE_SPEC_VERSION 1u
#define CAMPX_SHAPE_MAX_CELLS 1024 /* rows * cols; rows, cols <= 127 */
#define CAMPX_SHAPE_MAX_THINGS 8
#define CAMPX_SHAPE_MAX_LIST 2048  /* cells covered by all things together */

typedef struct CampxShapeThing {
  int32_t layer;            /* layer (character) it paints */
  int32_t is_sprite;        /* painted by paint_sprite (rendering.py:150), else paint_drape */
  int32_t visible;          /* Sprite.visible (campx/things.py:380); drapes: 1 */
  int32_t n_cells;          /* its shape: cells[cell_begin .. cell_begin + n_cells) */
  int32_t cell_begin;
  int32_t has_reward_mask;  /* bit a: action a makes it call Plot.add_reward(reward[a]) */
  int32_t terminate_mask;   /* bit a: action a makes it call Plot.terminate_episode() */
  int32_t reserved;
  int8_t drow[8], dcol[8];  /* offset change per action, already modulo rows / cols (>= 0) */
  float reward[8];
} CampxShapeThing;          /* 80 bytes */

typedef struct CampxShapeSpec {
  uint32_t magic, version;
  int32_t rows, cols;
  int32_t n_layers;
  int32_t n_things;                          /* stored in z-order, back to front */
  int32_t first_drape;                       /* index of the first thing that is not a sprite */
  int32_t any_reward;
  uint8_t layer_char[CAMPX_MAX_LAYERS];
  int32_t update_order[CAMPX_SHAPE_MAX_THINGS]; /* thing indices in update-schedule order
                                                (rewards are summed in that order) */
  CampxShapeThing things[CAMPX_SHAPE_MAX_THINGS];
  uint8_t backdrop[CAMPX_SHAPE_MAX_CELLS];   /* layer per cell of the Backdrop as its_showtime()
                                                leaves it (trail sprites' art cells painted) */
  uint16_t cells[CAMPX_SHAPE_MAX_LIST];      /* art cell of each shape cell: row << 8 | col */
} CampxShapeSpec;

int32_t campx_shape_spec_size(void);
int32_t campx_shape_spec_validate(const CampxShapeSpec* spec_host);

/*
 * Advance B environments of a shape game by T frames (T = 0 with emit_first: the
 * its_showtime() observation).  State: state.pos [2*n_things, B] int8 = cyclic (row, col)
 * offset of each thing from its art position, state.done, state.ret as for
 * campx_rollout_launch, and `backdrop_state` [B, rows*cols] int8 layer per cell (the
 * per-environment Backdrop; may be NULL when no visible sprite precedes the first
 * drape).  Outputs: out.obs (any out.obs_format), out.board, out.reward, out.discount, out.done,
 * out.bad_count / bad_flag; frames at base + t * stride as for campx_rollout_launch.
 * Action ids outside 0..4 move nothing, end nothing and are counted as bad.
 * The frame-major path (round 5, csrc/k_shape.hip): with `tables_dev` (campx_shape_tables_build)
 * and out.trace (8-byte aligned scratch of campx_shape_scratch_bytes(spec, B, T) bytes: the
 * things' offsets per frame and, for games with trails, the per-environment trail words every
 * fourth frame), a call that keeps every frame (int8, back to back, frames of whole 16-byte
 * chunks, no flat board, no emit_first) runs as two kernels - the update pass, then a render pass
 * of one-shot waves with memory-aligned 2 KiB windows that computes every W-cell row of the
 * observation arithmetically from 64-bit row words - which streams the observations at the
 * one-cell tier's rate.  Rows of 16 to 64 cells only; other games and calls ignore both (NULL is
 * fine) and run the one-wave-per-environment kernel.  Setting shape_split = 0: never.
 */
int64_t campx_shape_tables_bytes(const CampxShapeSpec* spec_host);   /* 0: not a game for that path */
/* Fills `tables_host` (HOST memory, `bytes` >= campx_shape_tables_bytes); the caller copies it
 * to the device.  Pure host code. */
int32_t campx_shape_tables_build(const CampxShapeSpec* spec_host, void* tables_host, int64_t bytes);
int64_t campx_shape_scratch_bytes(const CampxShapeSpec* spec_host, int64_t B, int32_t T);
int32_t campx_shape_rollout_launch(const CampxShapeSpec* spec_host, const CampxShapeSpec* spec_dev,
                                   const void* tables_dev, CampxState state, int8_t* backdrop_state,
                                   const int8_t* actions, CampxOutputs out, int64_t B, int32_t T,
                                   int32_t reset_first, int32_t emit_first, void* stream);


/*
 * Wide tier: games whose update pass is a STATE table - one row per state the game can
 * reach, (state, action) -> state - instead of a table indexed by the things' cells.  That
 * form has no board-size limit and no (rows*cols)^K blow-up, so it takes what the one-cell
 * tier cannot: boards ABOVE 128 cells (PyColab-sized mazes: 16x16, 20x20, 32x32 ...;
 * campx/engine.py:31 sets no limit), up to eight things that show, any number of hidden
 * values behind them (the z-order in force after Plot.change_z_order, keys that were
 * picked up, doors that opened).  The caller enumerates the states (campx_amd/tabulate.py runs
 * the game's own update() classes breadth-first from its_showtime()); state 0 is the
 * its_showtime() state.  The observation stream is the one-cell tier's render kernel, fed
 * by a 16-bit trace:
 *     entry = cell | (scenery layer the thing covers there) << 10 | shows << 15.
 * A frame of B environments is B rows of L*rows*cols bytes (1 536 B for 16x16 with six
 * characters, 6 KiB for 32x32), so the path is even more purely a write stream than the
 * one-cell tier's.
 */
#define CAMPX_WIDE_MAX_CELLS 1024        /* rows * cols; rows, cols <= 127 */
#define CAMPX_WIDE_MAX_STATES (1 << 24)
#define CAMPX_WIDE_MAX_DYN 8             /* things that move / come and go */
#define CAMPX_WIDE_MAX_VARIANTS 256      /* pictures of a scenery that changes */
#define CAMPX_WIDE_MAX_PIECES 16         /* cells of the scenery that come and go one by one */

typedef struct CampxWideSpec {
  uint32_t magic, version;
  int32_t rows, cols;
  int32_t n_layers;
  int32_t n_dyn;                   /* K: things that move / come and go, 1 .. CAMPX_WIDE_MAX_DYN */
  int32_t n_states;                /* S: reachable states, 1 .. CAMPX_WIDE_MAX_STATES */
  int32_t any_reward;
  int32_t has_perf;                /* `perf` below means something */
  int32_t any_dcode;               /* 1: some entry of `done` carries a discount code (0: the
                                      update kernel need not look the discount up) */
  int32_t n_variants;              /* V: pictures of the SCENERY the game shows (0 or 1: one; up to
                                      CAMPX_WIDE_MAX_VARIANTS).  A Backdrop.update() that repaints
                                      the backdrop (campx/things.py:103-148) - day and night over a
                                      whole floor - or a Drape of several cells that come and go
                                      (coins taken one by one) makes the scenery a function of
                                      the state: the render kernel then lays, per environment and
                                      frame, the pre-rotated row of the state's variant, which the
                                      update pass hands it as one more (never painted) plane of the
                                      trace.  With V > 1: n_dyn <= CAMPX_WIDE_MAX_DYN - 1, the trace
                                      holds n_dyn + 1 planes, and `variant_top_layer` /
                                      `state_variant` below are given. */
  int32_t n_pieces;                /* P: PIECES of the scenery, 0 .. CAMPX_WIDE_MAX_PIECES - fixed
                                      cells that show a character of their own in some states and
                                      the plain scenery in the others: the cells of a Drape whose
                                      curtain loses them one by one (coins that are taken, ice that
                                      breaks; campx/things.py:161-262 sets no one-cell limit), the
                                      cells a Backdrop.update() repaints (lamps).  Which of them
                                      show is a 16-bit MASK per state (`state_pieces`), handed to
                                      the render kernel as one more (never painted) plane of the
                                      trace; it patches them onto the scenery's row like the
                                      things, from ONE trace entry per environment however many
                                      there are.  With P > 0: n_dyn <= CAMPX_WIDE_MAX_DYN - 1,
                                      n_variants <= 1, the trace holds n_dyn + 1 planes. */
  uint8_t layer_char[CAMPX_MAX_LAYERS];
  int32_t dyn_layer[CAMPX_WIDE_MAX_DYN];   /* layer thing d paints */
  float discount_list[16];                 /* as CampxSpec.discount_list */
  uint8_t static_top_layer[CAMPX_WIDE_MAX_CELLS];  /* front-most scenery layer per cell */
  uint16_t piece_cell[CAMPX_WIDE_MAX_PIECES];      /* the cell of piece p (row * cols + col) */
  uint8_t piece_layer[CAMPX_WIDE_MAX_PIECES];      /* the layer it paints when it shows (it hides
                                                      static_top_layer there, like a thing) */
  /* HOST arrays, read by campx_wide_spec_validate(full) / campx_wide_tables_build() only -
   * the launch calls never touch them, they may be gone by then: */
  const uint16_t* state_cells;     /* [S][K]: bits 0-9 the cell thing d is on in state s; bit 15
                                      set when it does NOT show there (hidden by something in
                                      front, or not on the board at all) */
  const int32_t* next_state;       /* [S][5]: the state after (state, action) */
  const float* reward;             /* [S][5]: summed reward of the frame, NaN = None */
  const uint8_t* done;             /* [S][5]: as CampxTransition.done (bit 0 terminated, bits
                                      4-7 discount code) */
  const int8_t* perf;              /* [S][5] hidden performance (the value), or NULL */
  const uint8_t* variant_top_layer; /* [V][rows*cols]: the front-most scenery layer per cell in
                                      variant v (row 0 = static_top_layer); NULL when V <= 1 */
  const uint16_t* state_variant;   /* [S]: the variant the scenery shows in state s; NULL when V <= 1 */
  const uint16_t* state_pieces;    /* [S]: bit p set = piece p SHOWS in state s (not taken, and nothing
                                      in front of it); NULL when P = 0 */
} CampxWideSpec;

int32_t campx_wide_spec_size(void);
/* Checks the plain fields; the host arrays too when they are non-NULL. */
int32_t campx_wide_spec_validate(const CampxWideSpec* spec_host);

/*
 * Once per game: campx_wide_tables_bytes() of DEVICE memory, filled by
 * campx_wide_tables_build() from the host spec and its arrays (host arithmetic + one copy;
 * synchronises `stream`): the state table in the update kernel's packed form and the 16
 * byte-rotations of the scenery's row for the render kernel (CampxSpec.rot_obs / rot_board
 * explain them).
 */
int64_t campx_wide_tables_bytes(const CampxWideSpec* spec_host);
int32_t campx_wide_tables_build(const CampxWideSpec* spec_host, void* tables_dev, void* stream);

/*
 * State enumeration on the device for RULE games (campx_amd.rules classes, lowered to
 * CampxRule as for CampxSpec) on boards the one-cell tier cannot take (more than 128 cells): the
 * wide tier runs any state table, and for games of arbitrary Python classes the host fills it by
 * running them on the generic tier (campx_amd/tabulate.py: a frame of Python per (state,
 * action)); a multi-mover rule game on a PyColab-sized board (campx/engine.py:31 sets no size
 * limit) has millions of reachable states.  campx_wide_enumerate_launch() applies one frame of
 * the rules - the update pass of campx/engine.py:168-208 as rollout_kernel interprets it - to
 * N given states under each of the five actions; the caller (campx_amd/enumerate_states.py)
 * drives a breadth-first enumeration with it and fills CampxWideSpec's arrays from the last pass.
 *   cells_in    DEVICE uint16 [N][K]   the cell of every moving thing (row * cols + col)
 *   next_cells  DEVICE uint16 [N][5][K]
 *   reward      DEVICE float  [N][5]   NaN = None        done   DEVICE uint8 [N][5]
 *   shows       DEVICE uint8  [N][5]   bit d: thing d is the character its cell shows AFTER the frame
 *   perf        DEVICE int8   [N][5]   hidden performance of the frame, or NULL
 * The tables of CampxWideRules are DEVICE arrays of rows*cols entries (CampxSpec.static_* and
 * cell_class explain them).  Nothing is allocated; no host synchronisation.
 */
typedef struct CampxWideRules {
  uint32_t magic, version;         /* CAMPX_SPEC_MAGIC, CAMPX_SPEC_VERSION */
  int32_t rows, cols, n_layers;
  int32_t n_dyn;                   /* K: 1 .. CAMPX_MAX_DYN */
  int32_t n_rules, any_reward;
  int32_t perf_dyn, perf_n, perf_mode, perf_mask, perf_scale, perf_offset;
  int32_t dyn_layer[CAMPX_MAX_DYN];
  int32_t dyn_z[CAMPX_MAX_DYN];
  CampxRule rules[CAMPX_MAX_RULES];
  const uint8_t* top_layer;        /* DEVICE [rows*cols] front-most scenery layer per cell */
  const uint8_t* top_z;            /* DEVICE its z rank (0 = backdrop) */
  const uint16_t* cover;           /* DEVICE bit s = static drape s covers the cell */
  const uint8_t* cell_class;       /* DEVICE hidden-performance class per cell (all 0 without one) */
} CampxWideRules;

int32_t campx_wide_rules_size(void);
int32_t campx_wide_enumerate_launch(const CampxWideRules* rules_host, const uint16_t* cells_in,
                                    int64_t N, uint16_t* next_cells, float* reward, uint8_t* done,
                                    uint8_t* shows, int8_t* perf, void* stream);

/*
 * campx_reset_launch / campx_rollout_launch for a wide game.  The dynamic state of an
 * environment is its STATE INDEX: state.pos points at int32 [B] (4-byte aligned; the
 * positions, if wanted, are in the trace), state.pair_table is ignored.  out.trace is REQUIRED
 * and holds uint16 entries, [K, T, pitch] (reset: [K, pitch]) with pitch = out.scalar_pitch or
 * B, 2-byte aligned; frames are kept back to back (obs_t_stride == B*L*rows*cols,
 * board_t_stride == B*rows*cols) or, with strides of 0, only the last one.  B * L*rows*cols
 * must stay below 2^32 - 2^16.  16-bit observation formats as for campx_rollout_launch.
 * T = 1 is Engine.play().
 */
int32_t campx_wide_reset_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                CampxState state, CampxOutputs out, int64_t B, void* stream);
int32_t campx_wide_rollout_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                  CampxState state, const int8_t* actions, CampxOutputs out,
                                  int64_t B, int32_t T, int32_t reset_first, void* stream);

/*
 * ---- The trace as a stored trajectory ------------------------------------------------
 * A rollout's trace is a complete description of every frame (CampxOutputs.trace: one byte per
 * moving thing, frame and environment in the one-cell tier; 16 bits, plus one plane for a piece
 * mask or a scenery variant, in the state-table tier) at a hundredth of the observations' size.
 * A caller that trains from a replay buffer keeps traces and has the observations of the
 * transitions it samples rendered on demand.  No reference counterpart: the reference renders
 * every frame as it plays it (campx/engine.py:295-324).
 *
 *   campx_update_launch (above) / campx_wide_update_launch
 *       the update pass of T frames and nothing else: state, trace, per-frame scalars.
 *   campx_render_gather_launch / campx_wide_render_gather_launch
 *       row i of `obs` = the observation of frame t_idx[i], environment e_idx[i] of `trace`,
 *       bit for bit what a rollout writes for that frame and environment.
 */
typedef struct CampxGather {
  const void* trace;    /* DEVICE [n_planes][T][pitch] entries: uint8 (one-cell tier), uint16
                           (state-table tier, 2-byte aligned).  Any number of rollouts' traces
                           one after the other along T. */
  int64_t n_planes;     /* must be the game's: n_dyn, + 1 with a piece mask or scenery variants */
  int64_t T;            /* frames the trace holds */
  int64_t pitch;        /* entries from one frame's row to the next (>= B) */
  int64_t plane;        /* entries from one plane to the next (>= T * pitch) */
  const void* t_idx;    /* DEVICE [N] frame of row i ... */
  const void* e_idx;    /* ... and its environment; int32, or int64 with idx64 != 0.  An index
                           outside 0..T-1 / 0..B-1 is clamped on the device (nothing is read out of
                           bounds; the row shows the clamped frame) and counted. */
  int32_t idx64;
  int32_t obs_format;   /* CAMPX_OBS_INT8 / _F16 / _BF16 */
  int64_t N;            /* rows; N * L*rows*cols must stay below 2^32 - 2^16 (larger requests:
                           several calls, each of a multiple of 16 rows) */
  void* obs;            /* DEVICE [N][L][rows][cols], 16-byte aligned */
  int32_t* bad_count;   /* optional device int32: += rows with an index out of range */
  int32_t* bad_flag;    /* optional, as CampxOutputs.bad_flag: set to 1 when there was one */
  int32_t streaming;    /* != 0: the stores bypass the caches (`sc0 sc1 nt`, the rollout's
                           store); 0: plain stores - a minibatch is usually read again at once */
  int32_t reserved;
} CampxGather;

/* Asynchronous on `stream`, no synchronisation, no library state; every argument is checked
 * before anything is launched (CAMPX_EINVAL: NULL, N <= 0, misaligned `obs`, pitch < B, a plane
 * count that is not the game's, N * row bytes past the bound above, rows below 16 bytes). */
int32_t campx_render_gather_launch(const CampxSpec* spec_host, const CampxSpec* spec_dev,
                                   const CampxGather* gather, int64_t B, void* stream);
int32_t campx_wide_render_gather_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                        const CampxGather* gather, int64_t B, void* stream);
/* campx_wide_rollout_launch()'s arguments; out.obs / out.board are ignored (may be NULL), the
 * variant or mask plane of the trace is written exactly as in a full rollout. */
int32_t campx_wide_update_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                 CampxState state, const int8_t* actions, CampxOutputs out,
                                 int64_t B, int32_t T, int32_t reset_first, void* stream);
/*
 * ---- Closed-loop rollouts: actions sampled on the device from a per-state policy -------------
 * campx_wide_update_launch() with the action stream replaced by a policy over the game's states,
 * `policy` DEVICE float32 [n_states][5] (4-byte aligned): weights, not necessarily normalised.
 * The whole T-frame episode, sampling included, is one launch (csrc/k_policy.hip).  No reference
 * counterpart: the reference's drivers run their policy on the host, frame by frame
 * (examples/reinforce.py:136-149).
 *
 * The sampling rule.  For environment e and absolute frame f = first_frame + t:
 *   - one Philox4x32-10 block per environment and group of four frames: key (seed & 0xffffffff,
 *     seed >> 32), counter (e, g & 0xffffffff, g >> 32, 0) with g = f >> 2, multipliers
 *     0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85; frame f takes output
 *     word f & 3, x;
 *   - u = float(x >> 8) * 2^-24 (exact, in [0, 1));
 *   - with w[0..4] the row of the state the frame STARTS from (row 0 for an environment whose
 *     episode ended on the frame before): c0 = w0, c1 = c0 + w1, c2 = c1 + w2, c3 = c2 + w3,
 *     c4 = c3 + w4, f32 sums in this order; r = u * c4, one f32 multiply;
 *     action = (r >= c0) + (r >= c1) + (r >= c2) + (r >= c3).
 * An action of weight exactly 0 is never taken; a one-hot row is a deterministic policy.  A row
 * with a negative or NaN weight, or whose c4 is not a positive finite number, is BAD: the
 * environment-frame that meets it takes action 4 and is counted into out.bad_count / out.bad_flag,
 * as an action id outside 0..4 is.  A subnormal weight is a good weight - nothing is flushed: a row
 * of subnormal weights has a subnormal c4, and r = u * c4 is compared as the subnormal it is -
 * and -0.0 is not negative; finite weights whose c4 overflows to infinity make a bad row.
 *
 * Writes what campx_wide_update_launch() writes (state, trace with every plane, the per-frame
 * scalars, same row pitch), plus `actions_out` DEVICE int8 [T][pitch] - the actions taken - and,
 * unless NULL, `states_out` DEVICE int32 [T][pitch] (4-byte aligned): the row each frame sampled
 * from.  CAMPX_EINVAL: NULL, B <= 0 or above 2^32 - 1, T <= 0, first_frame < 0 or
 * first_frame + T past 2^63 - 1, misaligned pointers, pitch < B, out.perf for a game without.
 * Asynchronous on `stream`, no synchronisation, no library state.
 */
int32_t campx_wide_policy_update_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                        CampxState state, const float* policy, uint64_t seed,
                                        int64_t first_frame, CampxOutputs out, int8_t* actions_out,
                                        int32_t* states_out, int64_t B, int32_t T,
                                        int32_t reset_first, void* stream);
/*
 * ---- Closed-loop rollouts of a population of policies -----------------------------------------
 * campx_wide_policy_update_launch() for `n_members` policies at once - the same kernel source,
 * the same launch; the sampling rule, what is written, what is refused and the stream contract are
 * the ones above.  The member rule: `policy` is DEVICE float32 [n_members][n_states][5], B is a
 * multiple of n_members, and with n = B / n_members environment e belongs to member e / n -
 * members own equal, contiguous blocks of environments; the counter stays (absolute environment e,
 * absolute frame >> 2), and the row read for environment e in state s is policy[e / n][s] (s = 0
 * after a done).  Everything written is what
 * campx_wide_policy_update_launch() writes, except `states_out`, which holds the FLAT row
 * (e / n) * n_states + s: the row of `policy` seen as [n_members * n_states][5] the action was
 * sampled from, so that campx_table_lookup_launch() and campx_state_sums_launch() (with n_states =
 * n_members * n_states) serve all members in one launch each.  With n_members = 1 the call IS
 * campx_wide_policy_update_launch(): the same machine code, chosen by the same arithmetic.
 *
 * A lane per environment, 256 to a workgroup.  Two paths, `path`: 1 = a workgroup stages the table
 * in LDS and, beside it, the thresholds of only the members its 256 environments belong to; 2 =
 * table and weights are read through L1 / L2.  0 = path 1 whenever its LDS bytes - the table's
 * (entries, the states' cells, the hidden performance when out.perf is given) plus
 * members_per_block * n_states * 20 - are within the library setting wide_lds_max.  Neither path
 * changes a bit of any result.
 *
 * campx_wide_population_plan() is the choice as host-only arithmetic (nothing is launched):
 * plan_out[4] = the path taken (1 / 2); dynamic LDS bytes (0 on path 2); threads of a workgroup;
 * members_per_block, the largest number of distinct members the environments of any one workgroup
 * belong to (1 when n is a multiple of 256; 256 when n = 1 and B >= 256).  CAMPX_EINVAL: n_states
 * outside 1 .. CAMPX_WIDE_MAX_STATES, a has_perf that is not 0 / 1, B outside 1 .. 2^32 - 1,
 * n_members < 1, B % n_members != 0, n_members * n_states >= 2^31, wide_lds_max < 0, a `path`
 * outside 0 .. 2, path 1 for what does not fit, plan_out NULL.
 * campx_wide_policy_population_launch() returns CAMPX_EINVAL, before anything is launched, for
 * the same and for everything campx_wide_policy_update_launch() refuses.
 */
int32_t campx_wide_population_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t n_members,
                                   int64_t wide_lds_max, int32_t path, int64_t* plan_out);
int32_t campx_wide_policy_population_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                            CampxState state, const float* policy, uint64_t seed,
                                            int64_t first_frame, CampxOutputs out,
                                            int8_t* actions_out, int32_t* states_out, int64_t B,
                                            int32_t T, int32_t reset_first, int64_t n_members,
                                            int32_t path, void* stream);
/*
 * ---- Online tabular learners: one Q-table per environment, a whole run per launch -------------
 * Q-learning and expected SARSA update q[s][a] after every single frame and choose the next
 * frame's action from the updated table: no batch of the calls above expresses that.  Here
 * environment e IS learner e: it owns `q[e]` (DEVICE float32 [B][n_states][5], 16-byte aligned,
 * B * n_states * 5 < 2^31, updated in place), acts epsilon-greedily on it and learns from every
 * frame, T frames in one launch (csrc/k_learn.hip).  Nothing is shared between learners: no
 * atomics, and the run is reproducible bit for bit.  No trace and no per-frame stream is written.
 * No reference counterpart.
 *
 * The rule.  f32 throughout, every operation rounded on its own (no fused multiply-add), so that a
 * float32 restatement is bit-exact (tests/learner_reference.py is one, in numpy).  For learner e
 * with alpha[e], gamma[e], epsilon[e] (DEVICE float32 [B] each) at absolute frame
 * f = first_frame + t:
 *   1. One Philox4x32-10 block per learner and PAIR of frames: key (seed & 0xffffffff, seed >> 32),
 *      counter (e, g & 0xffffffff, g >> 32, 1) with g = f >> 1, constants as above; x0 is output
 *      word 2 * (f & 1) and x1 word 2 * (f & 1) + 1.  (The fourth counter word is 1 where the
 *      closed-loop rollouts have 0: the same seed gives unrelated streams.)
 *   2. s = state 0 if the learner's episode is over (or `reset_first`), else its state.
 *   3. u = float(x0 >> 8) * 2^-24; the learner explores iff u < epsilon[e], and then takes the
 *      action ((x1 >> 8) * 5) >> 24, an integer in 0 .. 4; otherwise the greedy action of
 *      q[e][s]: best = q0; for a = 1 .. 4: if (q[a] > best) best = q[a] - the lowest index wins a
 *      tie (among several +inf too), a NaN at a = 1 .. 4 never wins, and a NaN q0 is never
 *      displaced (no comparison with it holds): the action is then 0 and `best` that NaN.
 *   4. Entry (s, a) of the table: n, r (NaN - "None" - counted as 0, here, in `ret` and in
 *      reward_sum), d and D exactly as in the rule of campx_wide_sweeps_launch() below.
 *   5. The bootstrap b, from q[e][n] as it stands BEFORE this frame's update (which matters when
 *      n == s).  CAMPX_LEARN_Q: the greedy maximum `best` of that row.
 *      CAMPX_LEARN_EXPECTED_SARSA: m = ((((q0 + q1) + q2) + q3) + q4) * 0.2f, then
 *      b = (keep * best) + (epsilon[e] * m) with keep = 1.0f - epsilon[e].
 *   6. target = d ? r : r + (gamma[e] * D) * b.
 *   7. delta = target - q[e][s][a];  q[e][s][a] = q[e][s][a] + alpha[e] * delta.
 *      q may hold any float32: subnormals are kept, zeros keep their sign, an infinity or a NaN
 *      in q propagates through 5 - 7, `0 * inf` and `inf - inf` are NaN and are written as such
 *      (the payload and sign of a generated NaN are unspecified).
 *   8. Per window of `window` frames, counted from the launch's frame 0 (the last may be short),
 *      row w of three DEVICE [W][B] arrays, W = ceil(T / window): reward_sum float32 - r added in
 *      frame order, from 0 -, perf_sum int32 - the entries' hidden performance; NULL when not
 *      wanted, must be NULL for a game without - and episodes int32 - frames with d set.
 * state / done / ret are read and left as campx_wide_policy_update_launch() reads and leaves them.
 * A learner whose alpha, gamma or epsilon is not finite, or whose epsilon is outside [0, 1], is
 * BAD: it takes action 4 at every frame, its table is left untouched (its sums are still written),
 * and it is counted ONCE per launch into *bad_count (DEVICE int32, added to, may be NULL);
 * *bad_flag (device or mapped pinned int32, may be NULL) is set to 1.
 * In csrc/k_learn.hip the steps are the helpers of "The frame step", which the shared learners
 * below call too: Chunks (1), Carried (2), frame_action() (3), decode_entry() (4), td_error()
 * (5 - 7's delta) and WindowSums (8); Hyper holds the test of a BAD learner.
 *
 * A lane per learner, 256 to a workgroup.  Two paths, `path`: 1 = a workgroup stages the entries,
 * the perf bytes (when perf_sum is given) and its 256 learners' tables in LDS, the tables
 * lane-innermost, (s * 5 + a) * 256 + lane; 2 = each lane reads and writes its own 20-byte rows
 * of q through L1 / L2, the entries (and perf bytes) staying in LDS when they alone fit.
 * The LDS bytes:   table = up16(n_states * 40) + (has_perf ? up16(n_states * 5) : 0)
 *                  path 1: table + 256 * n_states * 20          path 2: table if it fits, else 0
 * 0 = path 1 whenever its bytes are within the library setting wide_lds_max.  Neither path
 * changes a bit of any result.
 *
 * campx_wide_learn_plan() is the choice as host-only arithmetic (nothing is launched):
 * plan_out[4] = the path taken (1 / 2); dynamic LDS bytes; threads of a workgroup; 1 when the
 * entries are staged in LDS, else 0.  CAMPX_EINVAL: n_states outside 1 .. CAMPX_WIDE_MAX_STATES,
 * a has_perf that is not 0 / 1, B outside 1 .. 2^32 - 1, B * n_states * 5 >= 2^31,
 * wide_lds_max < 0, a `path` outside 0 .. 2, path 1 for what does not fit, plan_out NULL.
 * campx_wide_learn_launch() returns CAMPX_EINVAL, before anything touches a device, for the same
 * and for: NULL where it is not allowed, a q that is not 16-byte aligned, other pointers that are
 * not 4-byte aligned, T <= 0, window < 1, first_frame < 0 or first_frame + T past 2^63 - 1, a
 * `rule` that is neither, perf_sum for a game without hidden performance.  Asynchronous on
 * `stream`, no synchronisation, no allocation, no library state.
 */
#define CAMPX_LEARN_Q 0
#define CAMPX_LEARN_EXPECTED_SARSA 1

typedef struct CampxLearner {
  float* q;               /* DEVICE [B][n_states][5], 16-byte aligned; updated in place */
  const float* alpha;     /* DEVICE [B] each */
  const float* gamma;
  const float* epsilon;
  float* reward_sum;      /* DEVICE [W][B], W = ceil(T / window) */
  int32_t* perf_sum;      /* DEVICE [W][B], or NULL */
  int32_t* episodes;      /* DEVICE [W][B] */
  int32_t* bad_count;     /* optional device int32: += bad learners */
  int32_t* bad_flag;      /* optional, as CampxOutputs.bad_flag */
  uint64_t seed;
  int64_t first_frame;    /* absolute number of the launch's frame 0 */
  int32_t window;         /* frames per window, >= 1 (may exceed T) */
  int32_t rule;           /* CAMPX_LEARN_Q / CAMPX_LEARN_EXPECTED_SARSA */
  int32_t path;           /* 0 chosen by arithmetic, 1 LDS, 2 global */
  int32_t reset_first;
} CampxLearner;

int32_t campx_wide_learn_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                              int32_t path, int64_t* plan_out);
int32_t campx_wide_learn_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                CampxState state, const CampxLearner* learner, int64_t B, int32_t T,
                                void* stream);
/*
 * ---- Shared online learners: n environments feed one Q-table, a whole run per launch ----------
 * The common shape of tabular RL on a vectorised engine: P learners, learner m fed by the
 * n = B / P consecutive environments [m * n, (m + 1) * n) - campx_wide_policy_population_launch()'s
 * split.  `q` is DEVICE float32 [P][n_states][5] (16-byte aligned, P * n_states * 5 < 2^31,
 * updated in place), alpha / gamma / epsilon DEVICE float32 [P].  P divides B and 1 <= n <= 1024,
 * the largest workgroup: a learner's environments sit in ONE workgroup, so that the per-frame
 * synchronisation is a workgroup barrier and T frames are one launch (csrc/k_learn.hip).  More
 * actors per learner would need a grid-wide barrier per frame: not offered.
 *
 * The learner is SYNCHRONOUS, and repeats bit for bit whatever the order in which its
 * environments arrive.  Frame f of learner m, every float32 operation rounded on its own:
 *   1. TD error per environment.  Every environment e of the learner does steps 1 - 6 of the rule
 *      above - the same functions of csrc/k_learn.hip, not a restatement of them - with q[m] in
 *      place of q[e] and alpha[m], gamma[m], epsilon[m]; the Philox counter is
 *      (ABSOLUTE environment e, g & 0xffffffff, g >> 32, 1), the stream of the per-environment
 *      learners.  It reads q[m] as it stands at the START of the frame - no environment sees
 *      another's update of the same frame.  delta_e = target - q[m][s_e][a_e].
 *   2. Quantise.  d = double(delta_e) * 2^32; z_e = llrint(d) (round half to even); a NaN gives 0
 *      and |d| > 2^52 (an infinity too) gives +-2^52, and both are counted in clamped[m].  1 024
 *      values of at most 2^52 cannot overflow an int64.
 *   3. Update per bin.  For every (s, a) that c >= 1 of the learner's environments visited in this
 *      frame: Z = the sum of their z_e (integers: any order), g = double(Z) / double(c),
 *      mean = float32(g * 2^-32), step = alpha[m] * mean, q[m][s][a] = q[m][s][a] + step.
 *      Bins nobody visited are not touched.  The mean makes the step size independent of n.
 *   4. The next frame starts from the updated table.
 *   5. reward_sum / perf_sum / episodes [W][B], `ret`, state and done are PER ENVIRONMENT, exactly
 *      as campx_wide_learn_launch() writes them.
 *   6. A learner whose alpha, gamma or epsilon is not finite, or whose epsilon is outside [0, 1],
 *      is BAD: all its environments take action 4 at every frame, its table is untouched, nothing
 *      is accumulated or clamped, and it is counted ONCE per learner and launch into *bad_count.
 * clamped DEVICE int64 [P] is WRITTEN, not added to: the TD errors of this launch that step 2 could
 * not hold.
 *
 * A workgroup holds G consecutive whole learners, G * n threads.  A frame is two phases with a
 * barrier after each: (A) every lane adds 1 to its bin's count and z to its bin's sum with
 * workgroup-scope atomics - the lane whose count-add returned 0 owns the bin; (B) the owner
 * exchanges both for 0 and writes q[m][s][a].  The cost of (B) does not grow with n_states.  One
 * accumulator per bin: the adds are not privatised (`copies` = 1).
 * Path 1: the entries, the perf bytes, the G tables and their accumulators in LDS:
 *     table = up16(n_states * 40) + (has_perf ? up16(n_states * 5) : 0)
 *     most  = min(P, n <= 256 ? 256 / n : 1)       G = min(most, (wide_lds_max - table) / (n_states * 80))
 *     LDS bytes = table + G * n_states * 80        (per entry: sum 8, q 4, count 4)
 * Path 2: q and the accumulators in global memory, G = most; `scratch` (DEVICE, 8-byte aligned, at
 * least campx_wide_shared_scratch_bytes() = P * n_states * 5 * 12 bytes) must be ZERO on entry and
 * is left zero; the entries (and perf bytes) are in LDS when `table` alone is within wide_lds_max.
 * `path` 0 takes path 1 when G >= 1 and G == most or G * n >= 64 (a workgroup that its LDS cuts
 * below a wave idles most of one at every frame); 1 forces it (refused when not even one learner
 * fits), 2 forces path 2.  No path, G or order of arrival changes a bit of any result: only
 * integers are added.
 *
 * campx_wide_shared_plan() is the choice as host-only arithmetic: plan_out[6] = path (1 / 2); G;
 * threads of a workgroup (G * n); dynamic LDS bytes; 1 when the entries are staged in LDS;
 * accumulator copies per bin (1).  CAMPX_EINVAL: n_states outside 1 .. CAMPX_WIDE_MAX_STATES, a
 * has_perf that is not 0 / 1, B outside 1 .. 2^32 - 1, P < 1, P not dividing B, B / P > 1024,
 * P * n_states * 5 >= 2^31, wide_lds_max < 0, a `path` outside 0 .. 2, path 1 for what does not
 * fit, plan_out NULL.  campx_wide_shared_launch() returns CAMPX_EINVAL, before anything touches a
 * device, for the same and for what campx_wide_learn_launch() refuses, a clamped that is NULL or
 * not 8-byte aligned, and - on path 2 - a scratch that is NULL, misaligned or too small.
 * Asynchronous on `stream`, no synchronisation, no allocation, no library state.
 */
typedef struct CampxSharedLearner {
  float* q;               /* DEVICE [P][n_states][5], 16-byte aligned; updated in place */
  const float* alpha;     /* DEVICE [P] each */
  const float* gamma;
  const float* epsilon;
  float* reward_sum;      /* DEVICE [W][B], W = ceil(T / window) */
  int32_t* perf_sum;      /* DEVICE [W][B], or NULL */
  int32_t* episodes;      /* DEVICE [W][B] */
  int64_t* clamped;       /* DEVICE [P]: written */
  void* scratch;          /* path 2: zero on entry, left zero; may be NULL on path 1 */
  int64_t scratch_bytes;
  int32_t* bad_count;     /* optional device int32: += bad learners */
  int32_t* bad_flag;      /* optional, as CampxOutputs.bad_flag */
  uint64_t seed;
  int64_t first_frame;    /* absolute number of the launch's frame 0 */
  int64_t n_learners;     /* P */
  int32_t window;         /* frames per window, >= 1 (may exceed T) */
  int32_t rule;           /* CAMPX_LEARN_Q / CAMPX_LEARN_EXPECTED_SARSA */
  int32_t path;           /* 0 chosen by arithmetic, 1 LDS, 2 global */
  int32_t reset_first;
} CampxSharedLearner;

int32_t campx_wide_shared_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t P,
                               int64_t wide_lds_max, int32_t path, int64_t* plan_out);
int64_t campx_wide_shared_scratch_bytes(int64_t n_states, int64_t P);
int32_t campx_wide_shared_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                 CampxState state, const CampxSharedLearner* learner, int64_t B,
                                 int32_t T, void* stream);
/*
 * ---- Online learners with eligibility traces: Q(lambda) and expected SARSA(lambda) ------------
 * The one-step learners above move a reward back one state per visit.  Here learner e (environment
 * e, as in campx_wide_learn_launch()) also owns a trace per (state, action), `traces[e]`, of the
 * shape and contract of `q[e]` (DEVICE float32 [B][n_states][5], 16-byte aligned, updated in
 * place), and every frame moves EVERY entry whose trace is not zero: T frames in one launch, no
 * reduction, no atomics, reproducible bit for bit (csrc/k_learn.hip;
 * tests/trace_learner_reference.py restates the frame in numpy).
 *
 * The frame of a good learner in state s, table q, traces z, with lam[e] (DEVICE float32 [B]);
 * f32 throughout, every operation rounded on its own.  Steps 1 - 4 and 8 of the rule of the
 * one-step learners - the Philox words, s, the action, the entry, the sums - hold unchanged.
 *   1. Act.  row = q[s][.]; a = the frame's action from it; old = row[a]; best = the greedy
 *      maximum of row.
 *   2. Cut.  CAMPX_LEARN_Q (Watkins): if !(old == best) - a NaN cuts - every z[i] = +0.
 *      CAMPX_LEARN_EXPECTED_SARSA never cuts.
 *   3. TD error.  The entry (s, a): n, r, d, D.  delta = target - old with the bootstrap of the
 *      one-step rule taken from q[n][.] as the table stands now, before this frame's sweep.
 *   4. Bump.  CAMPX_TRACE_ACCUMULATING: z[s][a] = z[s][a] + 1.  CAMPX_TRACE_REPLACING: z[s][a] = 1.
 *   5. Sweep.  step = alpha[e] * delta; for every entry i with z[i] != 0.0f (a NaN trace counts):
 *      q[i] = q[i] + (step * z[i]).  An entry whose trace is +-0 is NOT written: its bits stay,
 *      whatever `step` is.
 *   6. Decay.  d set: every z[i] = +0.  Otherwise c = (gamma[e] * D) * lam[e] and z[i] = c * z[i],
 *      for EVERY i (so that a trace may become -0, or NaN under an infinite c).
 *   7. Advance state / done / ret and the window sums exactly as the one-step learners do.
 * `reset_first` also zeroes (+0) a good learner's traces before frame 0.  Consequences, each pinned
 * by the tests: lam = 0 gives campx_wide_learn_launch()'s q, sums and state bit for bit (for finite
 * gamma * D); launches of T1 and T2 frames equal one of T1 + T2; no `path` or `team` changes a bit.
 * A learner is BAD as above, or when its lam is not within [0, 1] (a NaN is not): action 4 at every
 * frame, q AND traces untouched (`reset_first` included), counted once.
 *
 * A learner is a TEAM of L lanes, L a power of two in 1 .. 256; a workgroup is 256 threads, 256 / L
 * learners.  Every lane of a team computes steps 1 - 3, `step` and c redundantly, from the same
 * words (broadcast reads); lane l owns the entries i = l (mod L) for steps 2 and 4 - 6, fused into
 * one pass: one read of z, one read-modify-write of q where z != 0, one write of z.  For L > 1 a
 * frame has two workgroup barriers - after the rows are read, and after the pass - that every lane
 * of the workgroup reaches at every frame; L = 1 needs none.  The team's lane 0 writes the sums and
 * the final state.
 * Path 1: the entries, the perf bytes and the workgroup's q and z in LDS - lane-innermost,
 * i * 256 + learner, for L = 1; entry-innermost, learner * n_states * 5 + i, for L > 1:
 *     LDS bytes = table + (256 / L) * n_states * 5 * 8       (table: as for the one-step learners)
 * Path 2: q and z through L1 / L2, the entries (and perf bytes) in LDS when they alone fit.
 * `team` 0 and `path` 0: the SMALLEST L whose path-1 bytes are within wide_lds_max, path 1; when
 * not even L = 256 fits, path 2 with L = 256.  A `team` forces L (path 1 if it fits, else 2); path
 * 1 forces path 1 (the smallest L that fits, or `team`; refused when it does not fit); path 2 takes
 * `team`, or 256.  This is arithmetic, not tuned.
 *
 * campx_wide_traces_plan(): plan_out[5] = path (1 / 2); L; dynamic LDS bytes; threads of a workgroup
 * (256); 1 when the entries are staged in LDS.  CAMPX_EINVAL: what campx_wide_learn_plan() refuses,
 * a `team` that is neither 0 nor a power of two up to 256, a forced shape that does not fit.
 * campx_wide_traces_launch() returns CAMPX_EINVAL, before anything touches a device, for the same,
 * for what campx_wide_learn_launch() refuses, for `traces` or `lam` that are NULL or misaligned
 * (16 and 4 bytes), and for a `trace` that is neither kind.  Asynchronous on `stream`, no
 * synchronisation, no allocation, no library state.
 */
#define CAMPX_TRACE_ACCUMULATING 0
#define CAMPX_TRACE_REPLACING 1

typedef struct CampxTraceLearner {
  float* q;               /* DEVICE [B][n_states][5], 16-byte aligned; updated in place */
  float* traces;          /* DEVICE [B][n_states][5], 16-byte aligned; updated in place */
  const float* alpha;     /* DEVICE [B] each */
  const float* gamma;
  const float* epsilon;
  const float* lam;
  float* reward_sum;      /* DEVICE [W][B], W = ceil(T / window) */
  int32_t* perf_sum;      /* DEVICE [W][B], or NULL */
  int32_t* episodes;      /* DEVICE [W][B] */
  int32_t* bad_count;     /* optional device int32: += bad learners */
  int32_t* bad_flag;      /* optional, as CampxOutputs.bad_flag */
  uint64_t seed;
  int64_t first_frame;    /* absolute number of the launch's frame 0 */
  int32_t window;         /* frames per window, >= 1 (may exceed T) */
  int32_t rule;           /* CAMPX_LEARN_Q / CAMPX_LEARN_EXPECTED_SARSA */
  int32_t path;           /* 0 chosen by arithmetic, 1 LDS, 2 global */
  int32_t reset_first;
  int32_t trace;          /* CAMPX_TRACE_ACCUMULATING / CAMPX_TRACE_REPLACING */
  int32_t team;           /* 0 chosen by arithmetic, else L */
} CampxTraceLearner;

int32_t campx_wide_traces_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                               int32_t path, int32_t team, int64_t* plan_out);
int32_t campx_wide_traces_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                 CampxState state, const CampxTraceLearner* learner, int64_t B,
                                 int32_t T, void* stream);
/*
 * ---- Dyna-Q online learners: n planning updates a frame, a whole run per launch ----------------
 * The learners above spend one table update per frame of experience.  Dyna-Q (Sutton & Barto
 * ch. 8) also replays, after every real step, `n` transitions it REMEMBERS.  The game's table is
 * deterministic, so the transition of a remembered (s, a) is the table's entry: the learner's
 * private model shrinks to the list of pairs it has visited.  Learner e is environment e, as in
 * campx_wide_learn_launch().  Besides q[e] it owns a model, two DEVICE arrays updated in place:
 *   seen    int32 [B][n_states * 5], 16-byte aligned
 *   n_seen  int32 [B]
 * The first n_seen[e] elements of seen[e] are the flat entries s * 5 + a the learner has met, in
 * order of first visit.  Elements beyond that count are never read and never written.
 * T frames in one launch, nothing shared between learners, no atomics, reproducible bit for bit
 * (csrc/k_learn.hip; tests/dyna_learner_reference.py restates the frame in numpy).
 *
 * Frame f = first_frame + t of a good learner; f32 throughout, every operation rounded on its own:
 *   1. Real step.  Steps 1 - 7 of the rule of the one-step learners, unchanged - the same functions
 *      of csrc/k_learn.hip, not a restatement of them.  q[e][s][a] is updated.
 *   2. Record.  If i = s * 5 + a is not among the first n_seen[e] elements of seen[e]:
 *      seen[e][n_seen[e]] = i; n_seen[e] += 1.  (A list that is already 5 * n_states long -
 *      which only one given with repeats can be while a pair is still new - takes no more.)
 *   3. Plan.  For k = 0 .. n - 1 with n = planning[e] (DEVICE int32 [B]), one after the other:
 *        x   = output word k & 3 of the Philox4x32-10 block with key (seed & 0xffffffff,
 *              seed >> 32) and counter (e, f & 0xffffffff, f >> 32, 2 + (k >> 2)) - the fourth
 *              counter words 0 and 1 are taken by the closed-loop rollouts and by exploration;
 *        idx = (uint64(x) * uint64(n_seen[e])) >> 32;   i = seen[e][idx];
 *        entry i of the game's table gives n', r, d, D as in step 4 of the one-step rule;
 *        the bootstrap b of step 5 from q[e][n'] as it stands BEFORE this planning step's write;
 *        delta = (d ? r : r + (gamma[e] * D) * b) - q[e][i];   q[e][i] = q[e][i] + alpha[e] * delta.
 *      Planning steps are SEQUENTIAL: each sees the writes of those before it, and of step 1.
 *      Sampling is UNIFORM OVER THE SEEN PAIRS - not "a seen state first, then an action taken in
 *      it" as in the book's pseudocode: a state met with four actions is drawn four times as often
 *      as one met with a single action.
 *   4. Advance.  The window sums, state, done and ret advance exactly as in the one-step learners.
 *      The next frame acts on q as planning left it.
 * `reset_first` starts a new episode; the model stays, as the table does.
 *
 * A learner is BAD when it is bad under the one-step rule; or when its planning[e] is outside
 * 0 .. CAMPX_DYNA_MAX_PLANNING (1024: the fourth counter word stays below 258); or when its list,
 * as screened at the start of the launch, has n_seen[e] outside 0 .. 5 * n_states or one of its
 * first n_seen[e] elements outside 0 .. 5 * n_states - 1.  The screening is what keeps every
 * planning read in bounds.  A BAD learner takes action 4 at every frame; its q, seen and n_seen are
 * untouched (its sums are written); it is counted ONCE per launch into *bad_count.  A list with
 * repeated elements is used as given: a repeat is sampled as often as it is listed.
 * Consequences, each pinned by the tests: planning = 0 gives campx_wide_learn_launch()'s q, sums
 * and state bit for bit, and records the model; launches of T1 and T2 frames equal one of T1 + T2;
 * neither path changes a bit.
 *
 * A lane per learner, 256 to a workgroup, no barrier inside the frame loop; every loop bound is a
 * kernel argument or the screened planning[e] <= 1024.  The next frame's row is RE-READ after the
 * last planning step (planning may have written any element of it); a learner with planning[e] = 0
 * keeps the one-step learners' patch of the one element written.
 * Path 1: the workgroup stages in LDS, all lane-innermost, the entries and perf bytes; its 256
 * learners' q as campx_wide_learn_launch() lays them out; the seen lists as 16-bit elements
 * [5 * n_states][256]; and a membership bitmap of W = ceil(5 * n_states / 32) 32-bit words per
 * learner, [W][256], rebuilt from the list at the start of the launch:
 *     LDS bytes = table + 256 * (n_states * 20 + n_states * 10 + 4 * W)     (table: as above)
 * (path 1 also needs 5 * n_states <= 65536, the 16-bit element).  Within a row of 256 16-bit
 * elements lane t sits in dword (t & 31) + 32 * (t >> 6), half (t >> 5) & 1: the 32 lanes of a
 * half wave fall on 32 different banks whichever elements they read.
 * Path 2: q, seen and the bitmap go through L1 / L2; the bitmap is the caller's scratch `marks`,
 * DEVICE uint32 [B][W], 4-byte aligned, contents ignored on entry and unspecified afterwards (may
 * be NULL on path 1); the entries (and perf bytes) stay in LDS when they alone fit.
 * `path` 0 takes path 1 whenever its bytes are within wide_lds_max: arithmetic, not tuned.
 *
 * campx_wide_dyna_plan(): plan_out[5] = path (1 / 2); dynamic LDS bytes; threads of a workgroup
 * (256); 1 when the entries are staged in LDS; W.  CAMPX_EINVAL: what campx_wide_learn_plan()
 * refuses.  campx_wide_dyna_launch() returns CAMPX_EINVAL, before anything touches a device, for
 * the same, for what campx_wide_learn_launch() refuses, for `seen` (16 bytes), `n_seen` or
 * `planning` (4 bytes) that are NULL or misaligned, and - on path 2 - for a `marks` that is NULL
 * or not 4-byte aligned.  Asynchronous on `stream`, no synchronisation, no allocation, no library
 * state.
 */
#define CAMPX_DYNA_MAX_PLANNING 1024

typedef struct CampxDynaLearner {
  float* q;               /* DEVICE [B][n_states][5], 16-byte aligned; updated in place */
  const float* alpha;     /* DEVICE [B] each */
  const float* gamma;
  const float* epsilon;
  float* reward_sum;      /* DEVICE [W][B], W = ceil(T / window) */
  int32_t* perf_sum;      /* DEVICE [W][B], or NULL */
  int32_t* episodes;      /* DEVICE [W][B] */
  int32_t* bad_count;     /* optional device int32: += bad learners */
  int32_t* bad_flag;      /* optional, as CampxOutputs.bad_flag */
  uint64_t seed;
  int64_t first_frame;    /* absolute number of the launch's frame 0 */
  int32_t window;         /* frames per window, >= 1 (may exceed T) */
  int32_t rule;           /* CAMPX_LEARN_Q / CAMPX_LEARN_EXPECTED_SARSA */
  int32_t path;           /* 0 chosen by arithmetic, 1 LDS, 2 global */
  int32_t reset_first;
  int32_t* seen;          /* DEVICE [B][n_states * 5], 16-byte aligned; updated in place */
  int32_t* n_seen;        /* DEVICE [B]; updated in place */
  const int32_t* planning; /* DEVICE [B]: planning updates per frame, 0 .. CAMPX_DYNA_MAX_PLANNING */
  uint32_t* marks;        /* path 2: scratch [B][ceil(n_states * 5 / 32)]; may be NULL on path 1 */
} CampxDynaLearner;

int32_t campx_wide_dyna_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                             int32_t path, int64_t* plan_out);
int32_t campx_wide_dyna_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                               CampxState state, const CampxDynaLearner* learner, int64_t B,
                               int32_t T, void* stream);
/*
 * ---- Actor-critic online learners: a softmax policy per learner, a whole run per launch --------
 * The learners above are value-based and act epsilon-greedily.  This one is the policy-gradient
 * family: one-step actor-critic (Sutton & Barto 13.5, without the gamma^t factor).  Learner e is
 * environment e, as in campx_wide_learn_launch(), and owns two DEVICE tables updated in place:
 *   prefs   float32 [B][n_states][5], 16-byte aligned: the preferences of a softmax policy
 *   values  float32 [B][n_states],    16-byte aligned: the critic
 * T frames in one launch, nothing shared between learners, no atomics, reproducible bit for bit
 * (csrc/k_learn.hip; tests/actor_critic_reference.py restates rule and frame in numpy).
 *
 * Rule 1, the weights of a row of preferences h[0..4].  THE WEIGHTS ARE THIS RULE, NOT exp(): no
 * library exponent is called anywhere, every operation is one f32 operation rounded on its own.
 *   m = h[0]; for a = 1 .. 4: if (h[a] > m) m = h[a]      (the lowest index wins ties, NaN never wins)
 *   the row is GOOD when (m - m) == 0 and h[a] <= m for all five a: a NaN or a +inf anywhere, or
 *   five -inf, make it bad; an element of -inf in a good row is good and gets weight 0.
 *   For a good row, per element:
 *     d = h[a] - m;  t = d * log2e,  log2e = 0x1.715476p+0f (the f32 nearest to log2(e));
 *     if t < -100: w[a] = +0 exactly.  Otherwise
 *     k = rint(t) (ties to even);  f = t - k (exact, |f| <= 0.5);
 *     p = c6;  p = p * f + c5;  p = p * f + c4;  ...  p = p * f + c0   (Horner, 12 operations);
 *     w[a] = ldexp(p, k)   (exact: k >= -100 and 0.7 < p < 1.5, no result is subnormal).
 *   c0 .. c6 are ln(2)^n / n! rounded to f32:
 *     0x1p+0f, 0x1.62e43p-1f, 0x1.ebfbep-3f, 0x1.c6b08ep-5f, 0x1.3b2ab6p-7f, 0x1.5d87fep-10f,
 *     0x1.430912p-13f.
 *   The maximum's weight is exactly 1 (d = 0, p = c0) and no weight is larger, so the row's total
 *   c4 lies in [1, 5] and the row passes the sampler's own test.  A row that is not good has the
 *   weights {0, 0, 0, 0, 0}, which the sampler calls bad.  Against float64 exp(d) the largest
 *   relative error measured is 3.74e-6 (6 M values of d in [-69, 0]; almost all of it is the
 *   rounding of t at large |d|; 2.4e-7 for |d| < 1).  `campx_amd.returns.softmax_weights()`
 *   restates the rule in torch element-wise operations, the same bits on CPU and device.
 *
 * Frame f = first_frame + t of a good learner, from state s (state 0 after a `done`):
 *   1. w = rule 1 of prefs[e][s]; thresholds c0 = w0, c1 = c0 + w1, ... c4 and the action by the
 *      closed-loop rollouts' sampler, WITH THEIR STREAM: x = output word f & 3 of the Philox4x32-10
 *      block with key (seed & 0xffffffff, seed >> 32) and counter (e, g & 0xffffffff, g >> 32, 0),
 *      g = f >> 2;  u = (x >> 8) * 2^-24;  r = u * c4;
 *      a = (r >= c0) + (r >= c1) + (r >= c2) + (r >= c3).  The learner samples exactly as
 *      campx_wide_policy_population_launch() samples the weights of rule 1.
 *   2. Entry (s, a) gives n, r, done, D as in step 4 of the one-step learners' rule.
 *   3. delta = (done ? r : r + (gamma[e] * D) * values[e][n]) - values[e][s], both values as the
 *      frame found them.
 *   4. values[e][s] = values[e][s] + alpha_critic[e] * delta.
 *   5. step = alpha_actor[e] * delta; for each a': pi = w[a'] / c4 (one f32 division);
 *      prefs[e][s][a'] = prefs[e][s][a'] + step * ((a' == a ? 1 : 0) - pi).
 *   6. The window sums, state, done and ret advance exactly as in the one-step learners.
 * A frame whose row is not good takes action 4 and changes neither table; such environment-frames
 * are counted into *bad_rows.  A learner whose alpha_actor, alpha_critic or gamma is not finite is
 * BAD: it takes action 4 at every frame, both tables are untouched (its sums are written), and it
 * is counted ONCE per launch into *bad_count (its frames are not counted as bad rows).
 * Consequences, each pinned by the tests: with both step sizes 0 the walk is that of the closed-loop
 * rollouts on softmax_weights(prefs); launches of T1 and T2 frames equal one of T1 + T2; neither
 * path changes a bit.
 * NOT offered: REINFORCE with episode returns, lambda-traces for the actor, an entropy bonus or a
 * temperature.  The shared form in which several actors feed one learner is the next section.
 *
 * A lane per learner, 256 to a workgroup, no barrier inside the frame loop.
 * Path 1: the workgroup stages in LDS the entries and perf bytes and its 256 learners' prefs and
 * values, lane-innermost ((s * 5 + a) * 256 + lane, then s * 256 + lane), copied in and out with
 * 16-byte accesses:
 *     LDS bytes = table + 256 * n_states * 24        (table: as campx_wide_learn_plan() counts it)
 * which wide_lds_max = 144 KiB allows up to 23 states.  Path 2: prefs and values go through
 * L1 / L2; the entries (and perf bytes) stay in LDS when they alone fit.  `path` 0 takes path 1
 * whenever its bytes are within wide_lds_max: arithmetic, not tuned.
 *
 * campx_wide_actor_plan(): plan_out[4] = path (1 / 2); dynamic LDS bytes; threads of a workgroup
 * (256); 1 when the entries are staged in LDS.  CAMPX_EINVAL: what campx_wide_learn_plan() refuses.
 * campx_wide_actor_launch() returns CAMPX_EINVAL, before anything touches a device, for the same,
 * for what campx_wide_learn_launch() refuses (prefs where it says q, the step sizes where it says
 * alpha and epsilon; there is no rule), for a `values` that is NULL or not 16-byte aligned and a
 * `bad_rows` that is not 4-byte aligned.  Asynchronous on `stream`, no synchronisation, no
 * allocation, no library state.
 */
typedef struct CampxActorLearner {
  float* prefs;              /* DEVICE [B][n_states][5], 16-byte aligned; updated in place */
  float* values;             /* DEVICE [B][n_states], 16-byte aligned; updated in place */
  const float* alpha_actor;  /* DEVICE [B] each */
  const float* alpha_critic;
  const float* gamma;
  float* reward_sum;         /* DEVICE [W][B], W = ceil(T / window) */
  int32_t* perf_sum;         /* DEVICE [W][B], or NULL */
  int32_t* episodes;         /* DEVICE [W][B] */
  int32_t* bad_count;        /* optional device int32: += bad learners */
  int32_t* bad_rows;         /* optional device int32: += environment-frames that met a bad row */
  int32_t* bad_flag;         /* optional, as CampxOutputs.bad_flag */
  uint64_t seed;
  int64_t first_frame;       /* absolute number of the launch's frame 0 */
  int32_t window;            /* frames per window, >= 1 (may exceed T) */
  int32_t path;              /* 0 chosen by arithmetic, 1 LDS, 2 global */
  int32_t reset_first;
} CampxActorLearner;

int32_t campx_wide_actor_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t wide_lds_max,
                              int32_t path, int64_t* plan_out);
int32_t campx_wide_actor_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                CampxState state, const CampxActorLearner* learner, int64_t B,
                                int32_t T, void* stream);
/*
 * ---- Shared actor-critic learners: n environments feed one policy, a whole run per launch ------
 * Synchronous advantage actor-critic (A2C) on the table: P learners, learner m fed by the
 * n = B / P consecutive environments [m * n, (m + 1) * n) - the split of
 * campx_wide_shared_launch() - and owning two DEVICE tables updated in place:
 *   prefs   float32 [P][n_states][5], 16-byte aligned, P * n_states * 5 < 2^31
 *   values  float32 [P][n_states],    16-byte aligned
 * alpha_actor / alpha_critic / gamma are DEVICE float32 [P].  P divides B and 1 <= n <= 1024, one
 * workgroup, as for the shared Q-learners.  The learner is SYNCHRONOUS and repeats bit for bit
 * whatever the order in which its environments arrive, the path, G or P: only integers are summed.
 *
 * Frame f = first_frame + t of learner m, every float32 operation one operation rounded on its own,
 * no contraction.  Every actor reads prefs[m] and values[m] as the frame found them.
 *  (A) Per actor (environment e of the learner), in state s (state 0 after a `done`):
 *   1. w = rule 1 above of prefs[m][s]; thresholds c0 .. c4 as in the actor-critic learners.
 *   2. The action by their sampler and their stream: counter (ABSOLUTE environment e,
 *      g & 0xffffffff, g >> 32, 0) with g = f >> 2, output word f & 3.
 *   3. A row that is not good: the actor takes action 4, contributes nothing, and is counted into
 *      *bad_rows, once per environment-frame of a good learner.  A learner whose alpha_actor,
 *      alpha_critic or gamma is not finite is BAD: all its environments take action 4 at every
 *      frame, nothing of it changes, nothing is accumulated or clamped, and it is counted ONCE per
 *      learner and launch into *bad_count (its frames are not counted as bad rows).
 *   4. Otherwise entry (s, a) gives n, r, done, D;
 *      discounted = (gamma[m] * D) * values[m][n];  target = done ? r : r + discounted;
 *      delta = target - values[m][s].
 *   5. Quantise as the shared Q-learners do: d = double(delta) * 2^32, z = llrint(d) (round half to
 *      even); a NaN gives 0 and |d| > 2^52 (an infinity too) gives +-2^52, both counted in
 *      clamped[m].
 *   6. sum[m][s][a] += z (int64) and visitors[m][s] += 1 (uint32).
 *  (B) Per state s that N >= 1 good-row actors of the learner were in, with Z[0..4] its five sums,
 *      and w, c4, the row h = prefs[m][s] and values[m][s] as (A) read them:
 *   1. Zall = Z0 + Z1 + Z2 + Z3 + Z4 in int64 (n <= 1024 and |z| <= 2^52: no overflow).
 *   2. mean_k = float32((double(Z[k]) / double(N)) * 2^-32), mean_all the same from Zall.
 *   3. values[m][s] = values[m][s] + alpha_critic[m] * mean_all.
 *   4. for k = 0 .. 4: pi = w[k] / c4; grad = mean_k - pi * mean_all;
 *      prefs[m][s][k] = h[k] + alpha_actor[m] * grad.
 *      Sums and visitors are zero again.  States nobody was in are not touched.
 *  The next frame starts from the updated tables.  reward_sum / perf_sum / episodes [W][B], `ret`,
 *  state and done are PER ENVIRONMENT, exactly as campx_wide_learn_launch() writes them.
 * A visited row so moves by the step size times the MEAN, over its visitors, of the one-step
 * actor-critic update (mean_k is the mean of delta * (a == k), mean_all that of delta): the step
 * size does not depend on n.  With both step sizes 0 the walk is that of
 * campx_wide_policy_population_launch() on the weights of rule 1.  n = 1 is NOT
 * campx_wide_actor_launch() bit for bit - the quantiser rounds delta to 2^-32 and the products are
 * taken in another order; nothing is claimed there.  clamped DEVICE int64 [P] is WRITTEN, not added
 * to.  NOT offered: an entropy bonus or a temperature, lambda-traces for the actor, REINFORCE with
 * episode returns, n-step targets, privatised accumulators.
 *
 * A workgroup holds G consecutive whole learners, G * n threads, and a frame is (A), a barrier,
 * (B), a barrier; the actor whose visitor-add returned 0 owns state s in (B) - it holds the row,
 * the weights and the value in registers already - and exchanges the six accumulators for 0.
 * Path 1: the entries, the perf bytes and the G learners' sums, prefs, values and visitors in LDS:
 *     table = as campx_wide_shared_plan() counts it
 *     most  = min(P, n <= 256 ? 256 / n : 1)       G = min(most, (wide_lds_max - table) / (n_states * 68))
 *     LDS bytes = table + G * n_states * 68        (per state: sums 40, prefs 20, value 4, visitors 4)
 * Path 2: prefs, values and the accumulators in global memory, G = most; `scratch` (DEVICE, 8-byte
 * aligned, at least campx_wide_actor_shared_scratch_bytes() = P * n_states * 44 bytes: int64
 * [P][n_states][5] sums, then uint32 [P][n_states] visitors) must be ZERO on entry and is left
 * zero; the entries (and perf bytes) are in LDS when `table` alone is within wide_lds_max.  `path`
 * 0 / 1 / 2: as in campx_wide_shared_plan().
 *
 * campx_wide_actor_shared_plan(): plan_out[6] as campx_wide_shared_plan() writes it, and
 * CAMPX_EINVAL for what that refuses.  campx_wide_actor_shared_scratch_bytes(): 0 for arguments out
 * of range.  campx_wide_actor_shared_launch() returns CAMPX_EINVAL, before anything touches a
 * device, for the same, for what campx_wide_actor_launch() refuses, a clamped that is NULL or not
 * 8-byte aligned, and - on path 2 - a scratch that is NULL, misaligned or too small.  Asynchronous
 * on `stream`, no synchronisation, no allocation, no library state.
 */
typedef struct CampxSharedActorLearner {
  float* prefs;              /* DEVICE [P][n_states][5], 16-byte aligned; updated in place */
  float* values;             /* DEVICE [P][n_states], 16-byte aligned; updated in place */
  const float* alpha_actor;  /* DEVICE [P] each */
  const float* alpha_critic;
  const float* gamma;
  float* reward_sum;         /* DEVICE [W][B], W = ceil(T / window) */
  int32_t* perf_sum;         /* DEVICE [W][B], or NULL */
  int32_t* episodes;         /* DEVICE [W][B] */
  int64_t* clamped;          /* DEVICE [P]: written */
  void* scratch;             /* path 2: zero on entry, left zero; may be NULL on path 1 */
  int64_t scratch_bytes;
  int32_t* bad_count;        /* optional device int32: += bad learners */
  int32_t* bad_rows;         /* optional device int32: += environment-frames that met a bad row */
  int32_t* bad_flag;         /* optional, as CampxOutputs.bad_flag */
  uint64_t seed;
  int64_t first_frame;       /* absolute number of the launch's frame 0 */
  int64_t n_learners;        /* P */
  int32_t window;            /* frames per window, >= 1 (may exceed T) */
  int32_t path;              /* 0 chosen by arithmetic, 1 LDS, 2 global */
  int32_t reset_first;
} CampxSharedActorLearner;

int32_t campx_wide_actor_shared_plan(int64_t n_states, int32_t has_perf, int64_t B, int64_t P,
                                     int64_t wide_lds_max, int32_t path, int64_t* plan_out);
int64_t campx_wide_actor_shared_scratch_bytes(int64_t n_states, int64_t P);
int32_t campx_wide_actor_shared_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                       CampxState state, const CampxSharedActorLearner* learner,
                                       int64_t B, int32_t T, void* stream);
/*
 * ---- Observations by state index --------------------------------------------------------------
 * Row i of `obs` DEVICE [N][L][H][W] (16-byte aligned; int8 0 / 1, or f16 / bf16 0.0 / 1.0 as
 * `obs_format` says) is, bit for bit, the observation a rollout shows for an environment that is
 * in state state_ids[i] of the game's table: what a network evaluated once per state - the policy
 * of campx_wide_policy_update_launch(), a critic - is evaluated on.  State 0 is the reset state.
 * `state_ids` DEVICE int32 [N] (`ids64` = 0) or int64 [N] (`ids64` = 1); NULL: row i is state i.
 * An id outside [0, n_states) is rendered as state 0 and counted into *bad_count (device int32,
 * caller-zeroed, may be NULL); *bad_flag (device or mapped pinned int32, may be NULL) is set to 1.
 *
 * One small launch writes the states' trace entries - the rows of the table's `state_cells` -
 * as a one-frame trace of N environments into `scratch` (DEVICE, 16-byte aligned, caller-owned,
 * at least campx_wide_render_states_scratch_bytes(spec, N) bytes; its contents mean nothing
 * afterwards); the rollout's render kernel then renders it (csrc/k_states.hip), in as many
 * launches as keep rows x row bytes of each below 2^32 - 65536.  N is not bounded by that.
 * CAMPX_EINVAL: NULL, N <= 0, misaligned pointers, a bad `obs_format`, too small a scratch.
 * Asynchronous on `stream`, no synchronisation, no allocation, no library state.
 */
int64_t campx_wide_render_states_scratch_bytes(const CampxWideSpec* spec_host, int64_t N);
int32_t campx_wide_render_states_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                        const void* state_ids, int32_t ids64, int64_t N, void* obs,
                                        int32_t obs_format, void* scratch, int64_t scratch_bytes,
                                        int32_t* bad_count, int32_t* bad_flag, void* stream);
/*
 * ---- Observation windows: egocentric or fixed crops, rendered without the full observation ----
 * A learner on a large board rarely wants the whole board: it wants what the agent sees.  Row i of
 * `obs` DEVICE [N][L][h][w] is a WINDOW of the observation that campx_wide_render_gather_launch() /
 * campx_wide_render_states_launch() write for the same row - `full[i]`, [L][H][W] - computed from
 * the row's trace entries without `full` ever being written (csrc/k_window.hip).  No reference
 * counterpart: the reference has no croppers.
 *
 * The rule.  A window is (h, w, anchor, pad).  Let (r0, c0) be the board coordinates of the
 * window's top-left cell:
 *   - CAMPX_WINDOW_ON_THING, egocentric on thing k: cell = entry_k & 0x3ff, where entry_k is the
 *     row's trace entry in plane k, clamped to H*W - 1; (cy, cx) = divmod(cell, W);
 *     r0 = cy - h / 2, c0 = cx - w / 2 (integer division).  The `shows` bit is NOT consulted: a
 *     hidden thing centres the window where its entry says it is.
 *   - CAMPX_WINDOW_FIXED: (r0, c0) is given; either may be negative (each within -255 .. 255).
 * Then
 *     obs[i][l][y][x] = full[i][l][r0 + y][c0 + x]      where that cell is on the board,
 *                     = (l == pad_layer) ? 1 : 0        off the board (pad_layer -1: 0 everywhere).
 * Formats are int8 0 / 1, f16 (0x3C00) and bf16 (0x3F80), as everywhere else.  By definition a
 * window is a crop of the full observation.
 *
 * Where a row's entries come from (`source`):
 *   CAMPX_WINDOWS_PAIRS   t_idx[i] * pitch + e_idx[i] into each plane of `trace`: CampxGather's
 *                         addressing - int32 or int64 indices, clamped, bad ones counted.
 *   CAMPX_WINDOWS_TRACE   no index arrays: row i is frame i / B, environment i % B; N = T * B and
 *                         `obs` is [T][B][L][h][w].
 *   CAMPX_WINDOWS_STATES  the entries of state state_ids[i] of the table blob, read directly (no
 *                         scratch trace); NULL: row i is state i.  An id outside [0, n_states) is
 *                         rendered as state 0 and counted.
 * `layer_of_cell` DEVICE uint8 [max(n_variants, 1)][CAMPX_WIDE_MAX_CELLS], 16-byte aligned: the
 * scenery's layer per cell of each variant (CampxWideSpec.static_top_layer /
 * variant_top_layer), cells past rows * cols padded with anything.  The caller builds it; the
 * table blob is not changed.
 */
#define CAMPX_WINDOWS_PAIRS 0
#define CAMPX_WINDOWS_TRACE 1
#define CAMPX_WINDOWS_STATES 2
#define CAMPX_WINDOW_ON_THING 0
#define CAMPX_WINDOW_FIXED 1

typedef struct CampxWindows {
  int32_t source;       /* CAMPX_WINDOWS_PAIRS / _TRACE / _STATES */
  int32_t idx64;        /* t_idx / e_idx / state_ids are int64 (else int32) */
  const void* trace;    /* PAIRS, TRACE: DEVICE uint16 [n_planes][T][pitch], as CampxGather.trace */
  int64_t n_planes;     /* must be the game's */
  int64_t T;            /* frames the trace holds */
  int64_t pitch;        /* entries from one frame's row to the next (>= B) */
  int64_t plane;        /* entries from one plane to the next (>= T * pitch) */
  const void* t_idx;    /* PAIRS: DEVICE [N] frame of row i ... */
  const void* e_idx;    /* ... and its environment */
  const void* state_ids; /* STATES: DEVICE [N], or NULL for 0 .. N-1 */
  int64_t N;            /* rows; N * L*h*w at most 2^32 - 65536 - 1 */
  int32_t h, w;         /* 1 <= h <= 2*rows - 1, 1 <= w <= 2*cols - 1, L*h*w >= 16 */
  int32_t anchor;       /* CAMPX_WINDOW_ON_THING / _FIXED */
  int32_t thing;        /* ON_THING: the plane that centres the window, < n_dyn */
  int32_t r0, c0;       /* FIXED: the top-left cell */
  int32_t pad_layer;    /* the layer set off the board, or -1 */
  int32_t obs_format;   /* CAMPX_OBS_INT8 / _F16 / _BF16 */
  void* obs;            /* DEVICE [N][L][h][w], 16-byte aligned */
  int32_t* bad_count;   /* optional device int32: += rows with an index or id out of range */
  int32_t* bad_flag;    /* optional, as CampxOutputs.bad_flag */
  int32_t streaming;    /* as CampxGather.streaming */
  int32_t reserved;
} CampxWindows;

/* Asynchronous on `stream`, no synchronisation, no allocation, no library state.  Every argument
 * is checked before anything touches a device.  CAMPX_EINVAL: a NULL or misaligned pointer; h < 1,
 * w < 1, h > 2*rows - 1 or w > 2*cols - 1; L*h*w < 16; N <= 0 or N * L*h*w above
 * 2^32 - 65536 - 1; a thing plane >= n_dyn; a pad layer >= L; a fixed corner outside -255 .. 255;
 * a trace geometry that campx_wide_render_gather_launch() refuses (pitch < B, a plane count that
 * is not the game's, planes closer than T * pitch); TRACE with N != T * B. */
int32_t campx_wide_render_windows_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                         const void* layer_of_cell, const CampxWindows* windows,
                                         int64_t B, void* stream);
/* The launch arithmetic of the above, host only: campx_render_gather_plan()'s eight numbers for
 * rows of Rw = L*h*w elements (16 .. 16 * 253 * 253). */
int32_t campx_wide_render_windows_plan(int64_t N, int32_t Rw, int32_t obs_format, uint64_t dst_addr,
                                       int64_t* plan_out);
/*
 * ---- Discounted returns and GAE advantages of a rollout, episode-aware ------------------------
 * One backward pass over the [T][B] streams of any tier's rollout, in one launch
 * (csrc/k_returns.hip).  Rollouts rebuild a finished environment in-kernel, so an episode may end
 * anywhere inside one: nothing is carried across a frame whose `done` is set.  No reference
 * counterpart: the reference's drivers play one episode at a time and sum on the host
 * (examples/reinforce.py:96-99, examples/actor_critic.py:120-123).
 *
 * The rule.  f32 throughout, every operation rounded on its own (no fused multiply-add), so that
 * a float32 restatement is bit-exact.  Per environment e, for t = T-1 down to 0:
 *     r      = isnan(reward[t]) ? 0 : reward[t]          (NaN: the frame had no reward)
 *     c      = gamma * discount[t]                       (gamma when `discount` is NULL)
 *     G_next = t == T-1 ? bootstrap[e] : G[t+1]          (0 when `bootstrap` is NULL)
 *     G[t]   = done[t] ? r : r + c * G_next
 * and with `values` (the critic at the state each frame STARTS in):
 *     v_next = t == T-1 ? bootstrap[e] : values[t+1]
 *     delta  = (done[t] ? r : r + c * v_next) - values[t]
 *     A[t]   = done[t] ? delta : delta + (c * lam) * A_next        (A_next = 0 past the last frame)
 * G goes to `returns`, A to `advantages`.  This holds over all of float32: subnormals are kept
 * (nothing is flushed) and zeros keep their sign.  Only a NaN REWARD counts as 0: a NaN in `values`
 * or `bootstrap` propagates, as does an infinity; `0 * inf` is NaN and is written as such, up to
 * the next frame whose `done` is set.  The payload and sign of a generated NaN are unspecified.
 *
 * Every stream is DEVICE memory, rows contiguous, frame t's row `*_pitch` elements after frame
 * t-1's (>= B; the padded rows of the rollout buffers are fine, each stream may have its own).
 * `values` and `advantages` are both given or both NULL; `discount` and `bootstrap` (float32 [B])
 * may be NULL.  CAMPX_EINVAL: NULL where it is not allowed, B <= 0, T <= 0, a pitch below B,
 * float pointers that are not 4-byte aligned, gamma or lam not finite.
 * Asynchronous on `stream`, no synchronisation, no library state.
 */
typedef struct CampxReturns {
  const float* reward;        /* [T][reward_pitch] */
  const uint8_t* done;        /* [T][done_pitch] */
  const float* discount;      /* [T][discount_pitch], or NULL */
  const float* values;        /* [T][values_pitch], or NULL */
  const float* bootstrap;     /* [B], or NULL */
  float* returns;             /* [T][returns_pitch] */
  float* advantages;          /* [T][advantages_pitch]; NULL exactly when `values` is */
  int64_t reward_pitch, done_pitch, discount_pitch, values_pitch, returns_pitch, advantages_pitch;
  float gamma, lam;
} CampxReturns;
int32_t campx_returns_launch(const CampxReturns* returns, int64_t B, int32_t T, void* stream);
/*
 * ---- Off-policy returns: V-trace targets and advantages, episode-aware ------------------------
 * The same backward pass for data that OTHER policies sampled (csrc/k_vtrace.hip): a learner fed
 * by stale or perturbed actors, population-based training, one rollout used for several gradient
 * steps.  V-trace (Espeholt et al. 2018, IMPALA) corrects with importance ratios truncated per
 * frame.  No reference counterpart.
 *
 * The rule.  f32 throughout, every operation rounded on its own (no fused multiply-add), the one
 * division IEEE-rounded, so that a float32 restatement is bit-exact (tests/vtrace_reference.py is
 * one, in numpy).  Per environment e, for t = T-1 down to 0:
 *     r      = isnan(reward[t]) ? 0 : reward[t]
 *     c      = gamma * discount[t]                       (gamma when `discount` is NULL)
 *   ratio mode:  w0 = ratio[t]
 *   table mode:  s = states[t], a = actions[t]
 *                in range  <=>  0 <= s < Nb  and  0 <= a < A
 *                w0 = in range ? target[(s % Nt) * A + a] / behaviour[s * A + a] : 0
 *                (a frame out of range is added to *bad_count; the tables are not read for it)
 *     w      = w0 > 0 ? w0 : +0                          (NaN, negatives and -0 count as 0; +Inf stays)
 *     rho    = w < rho_bar    ? w : rho_bar
 *     cs     = w < c_bar      ? w : c_bar
 *     rpg    = w < pg_rho_bar ? w : pg_rho_bar
 *     v      = values[t]
 *     v_next = t == T-1 ? bootstrap[e] : values[t+1]     (0 when `bootstrap` is NULL)
 *     q      = done[t] ? r : r + c * v_next
 *     delta  = rho * (q - v)
 *     k      = (c * lam) * cs
 *     D[t]   = done[t] ? delta : delta + k * D[t+1]      (D[T] = 0)
 *     vs[t]  = v + D[t]
 *     vs_nx  = t == T-1 ? bootstrap[e] : vs[t+1]
 *     qs     = done[t] ? r : r + c * vs_nx
 *     adv[t] = rpg * (qs - v)
 * vs goes to `vs` (the critic's regression target), adv to `advantages` (the policy-gradient
 * weight, the truncated ratio already inside).  Nb = n_behaviour_states is a multiple of Nt =
 * n_target_states: with the flat states `member * S + state` of
 * campx_wide_policy_population_launch(), `behaviour` is the population's [P * S][A] and `target`
 * the learner's [S][A]; Nb == Nt is the one-policy case.  As in the returns rule subnormals are
 * kept, zeros keep their sign, only a NaN REWARD counts as 0, and a NaN or an infinity in `values`
 * or `bootstrap` propagates up to the next frame whose `done` is set.  No ratio reaches the outputs
 * as a NaN.  Two consequences: with w == 1 everywhere and all three bars 1, D is bit for bit
 * campx_returns_launch()'s A at the same lam (a multiplication by 1.0 is exact); with c_bar = 0,
 * D equals delta.
 *
 * Streams and pitches as above.  `ratio` is given exactly when none of `target`, `behaviour`,
 * `states`, `actions` is: those four come together.  `target` is DEVICE float32 [Nt * A],
 * `behaviour` [Nb * A]; `bad_count` a DEVICE int64, 8-byte aligned, added to, may be NULL.
 * `path` says where the tables are read from: 1 = both staged in LDS once per workgroup, 2 =
 * through the caches, 0 = campx_table_lookup_launch()'s rule for both tables together - staged
 * when their bytes fit CAMPX_SUMS_LDS_BUDGET and their entries are no more than the frames a
 * workgroup looks up (256 * T).  By the rule no bit of the result depends on it.
 *
 * campx_vtrace_plan() is that arithmetic, pure host code: plan_out[3] = the path taken (1 / 2);
 * dynamic LDS bytes (0 on path 2); workgroups.  CAMPX_EINVAL: Nt < 1, Nb % Nt != 0, Nb above
 * 2^31 - 1, n_actions outside 1..128, B <= 0 or above 2^31, T <= 0, a `path` outside 0..2, path 1
 * for tables that do not fit.  campx_vtrace_launch() returns CAMPX_EINVAL for the same (in table
 * mode) and for: NULL `reward`, `done`, `values`, `vs` or `advantages`; both or neither of `ratio`
 * and the table set; a pitch below B; float or int32 pointers that are not 4-byte aligned, a
 * `bad_count` that is not 8-byte aligned; gamma or lam not finite; a bar that is not finite or is
 * negative.  Asynchronous on `stream`, no synchronisation, no library state.
 */
typedef struct CampxVtrace {
  const float* reward;        /* [T][reward_pitch] */
  const uint8_t* done;        /* [T][done_pitch] */
  const float* discount;      /* [T][discount_pitch], or NULL */
  const float* values;        /* [T][values_pitch] */
  const float* bootstrap;     /* [B], or NULL */
  const float* ratio;         /* [T][ratio_pitch]: ratio mode; NULL in table mode */
  const float* target;        /* [n_target_states * n_actions]: table mode */
  const float* behaviour;     /* [n_behaviour_states * n_actions] */
  const int32_t* states;      /* [T][states_pitch] */
  const int8_t* actions;      /* [T][actions_pitch] */
  float* vs;                  /* [T][vs_pitch] */
  float* advantages;          /* [T][advantages_pitch] */
  int64_t* bad_count;         /* or NULL */
  int64_t reward_pitch, done_pitch, discount_pitch, values_pitch, ratio_pitch, states_pitch,
      actions_pitch, vs_pitch, advantages_pitch;
  int64_t n_target_states, n_behaviour_states;
  int32_t n_actions;
  int32_t path;               /* 0 = by arithmetic, 1 = LDS, 2 = global */
  float gamma, lam, rho_bar, c_bar, pg_rho_bar;
  int32_t reserved;
} CampxVtrace;
int32_t campx_vtrace_launch(const CampxVtrace* vtrace, int64_t B, int32_t T, void* stream);
int32_t campx_vtrace_plan(int64_t n_target_states, int64_t n_behaviour_states, int32_t n_actions,
                          int64_t B, int32_t T, int32_t path, int64_t* plan_out);
/*
 * ---- Per-state sums of a rollout's streams: the learner's gradient in one launch -------------
 * Everything a tabular loss needs from the [T][B] streams of a rollout is a sum per (state,
 * action): the gradient of  sum_t f(table[s_t, a_t]) * w_t  with respect to `table` is
 * f'(table[s, a]) * (sum of w_t over the frames with s_t = s, a_t = a); a squared critic loss
 * needs n_s, sum G and sum G^2 per state.  One reduction (csrc/k_sums.hip) over the streams as the
 * rollout wrote them - int32 states, int8 actions, padded rows - gives those sums, for any tier.
 * No reference counterpart.
 *
 * The rule.  Sums are accumulated in 64-bit FIXED POINT, so the result does not depend on the
 * order of the additions and is bitwise reproducible (float atomics are not).  For a value stream
 * x (float32), frac_bits = f and N = T * B:
 *     n2    = ceil(log2(N))                     (0 for N = 1)
 *     lim   = 2^(62 - n2)                       in quantised units; 62 - n2 - f >= 0 is required
 *     d     = double(x) * 2^f                   (exact in double)
 *     q     = llrint(d)                         round to nearest, ties to even
 *     q     = 0, counted in `clamped`           if x is NaN
 *     q     = +lim / -lim, counted in `clamped` if |d| > lim   (+Inf / -Inf included)
 *     bin   = states[t][e] * n_actions + actions[t][e]     (n_actions = 1 and no action stream
 *                                                           when `actions` is NULL)
 *     acc[0][bin]     += 1
 *     acc[1 + k][bin] += q_k                    for each of the K = n_values value streams
 * A frame whose state is outside [0, n_states) or whose action is outside [0, n_actions) adds
 * nothing anywhere and is counted in `skipped`; its values are not looked at (so they are never
 * counted in `clamped`).  N additions of magnitude at most lim cannot overflow an int64, so every
 * kernel structure that performs these additions - in any order, with any privatisation -
 * produces the same 64-bit integers.  The float value of a sum is acc * 2^-f; each contribution was
 * rounded once, by at most half a quantum: |sum - exact| <= acc[0][bin] * 2^-(f+1) without clamping.
 * tests/state_sums_reference.py restates the rule in numpy.
 *
 * Streams are DEVICE memory, rows contiguous, frame t's row `*_pitch` elements after frame t-1's
 * (>= B, each stream its own).  `acc` is DEVICE int64 [1 + n_values][n_states * n_actions],
 * 8-byte aligned; `skipped` and `clamped` are DEVICE int64 scalars, 8-byte aligned.  Unless
 * `accumulate` is set the three are zeroed first, by one kernel on `stream` (the call stays
 * capturable, and a captured graph holds kernel nodes only); with `accumulate` the call adds onto them - the no-overflow bound above then holds
 * per call, and keeping the total of several calls inside an int64 is the caller's business.
 *
 * Two accumulation paths, `path`: 1 = the accumulators live in LDS - `copies` of them, selected by
 * lane, so that the lanes of a wave that land in one bin do not all queue on one LDS address -
 * take 64-bit LDS atomic adds, and each workgroup ends by folding its copies and adding its
 * non-zero bins to `acc` with global 64-bit atomics; 2 = every lane adds straight into `acc` with
 * no-return global 64-bit atomics (tables too large for LDS; contention is low there).
 * 0 = chosen by arithmetic: the LDS path when the accumulators fit and a workgroup's flush
 * (bins x planes atomics) is small against the frames it reduces, else global.  By the rule the
 * choice cannot change a bit of the result.
 *
 * campx_state_sums_plan() is that arithmetic, pure host code (nothing is launched): plan_out[8] =
 * the path taken (1 / 2); copies (1 on the global path); workgroups along B; workgroups along T;
 * frames per workgroup; dynamic LDS bytes (0 on the global path); n2; 62 - n2.  CAMPX_EINVAL:
 * n_states < 1 or above 2^31 - 1, n_actions outside 1..128, n_values outside 0..4, B <= 0 or above
 * 2^31, T <= 0, frac_bits < 0 or 62 - n2 - frac_bits < 0, a `path` outside 0..2, path 1 for
 * accumulators that do not fit LDS.  campx_state_sums_launch() returns CAMPX_EINVAL for the same
 * and for: NULL where it is not allowed (`actions` may be NULL exactly when n_actions == 1 is
 * meant without an action stream; values[k] for k >= n_values are ignored), misaligned pointers,
 * a pitch below B.  Asynchronous on `stream`, no synchronisation, no library state.
 */
#define CAMPX_SUMS_MAX_VALUES 4
#define CAMPX_SUMS_LDS_BUDGET 49152   /* bytes of LDS accumulators (all copies) a workgroup may hold */
typedef struct CampxStateSums {
  const int32_t* states;      /* [T][states_pitch] */
  const int8_t* actions;      /* [T][actions_pitch], or NULL */
  const float* values[CAMPX_SUMS_MAX_VALUES];     /* each [T][values_pitch[k]] */
  int64_t states_pitch, actions_pitch, values_pitch[CAMPX_SUMS_MAX_VALUES];
  int64_t n_states;
  int32_t n_actions;
  int32_t n_values;           /* K */
  int32_t frac_bits;
  int32_t accumulate;         /* != 0: add onto acc / skipped / clamped */
  int32_t path;               /* 0 = by arithmetic, 1 = LDS, 2 = global */
  int32_t reserved;
  int64_t* acc;               /* [1 + K][n_states * n_actions]; plane 0 is the count */
  int64_t* skipped;
  int64_t* clamped;
} CampxStateSums;
int32_t campx_state_sums_launch(const CampxStateSums* sums, int64_t B, int32_t T, void* stream);
int32_t campx_state_sums_plan(int64_t n_states, int32_t n_actions, int32_t n_values, int64_t B,
                              int32_t T, int32_t frac_bits, int32_t path, int64_t* plan_out);
/*
 * out[t][e] = table[states[t][e] * n_actions + actions[t][e]], float32 (csrc/k_sums.hip): what a
 * learner otherwise writes as two int64 copies of the streams and an advanced index.  Same stream
 * types and pitches as above (`actions` NULL: n_actions = 1); `table` DEVICE float32
 * [n_states * n_actions], staged in LDS when it fits and is small against the frames a workgroup
 * looks up, read through the caches otherwise.  A frame whose state or action is out of range
 * gets 0.0 and is counted into *bad_count (DEVICE int64, 8-byte aligned, added to, may be NULL).
 * CAMPX_EINVAL: NULL, bad sizes as above, misaligned pointers, a pitch below B.  Asynchronous on
 * `stream`, no synchronisation, no library state.
 */
typedef struct CampxTableLookup {
  const float* table;         /* [n_states * n_actions] */
  const int32_t* states;      /* [T][states_pitch] */
  const int8_t* actions;      /* [T][actions_pitch], or NULL */
  float* out;                 /* [T][out_pitch] */
  int64_t states_pitch, actions_pitch, out_pitch;
  int64_t n_states;
  int32_t n_actions;
  int32_t reserved;
  int64_t* bad_count;
} CampxTableLookup;
int32_t campx_table_lookup_launch(const CampxTableLookup* lookup, int64_t B, int32_t T,
                                  void* stream);
/*
 * ---- Exact policy evaluation and value iteration on the state table ---------------------------
 * The blob campx_wide_policy_update_launch() walks is the game's complete deterministic MDP:
 * (state, action) -> next state, reward, done, discount code.  Sweeps of the Bellman backup over
 * it give the exact value of a policy and the optimal values, where the rollouts above can only
 * sample them (csrc/k_plan.hip).  No reference counterpart.
 *
 * The rule.  f32 throughout, every operation rounded on its own (no fused multiply-add), the one
 * division IEEE-rounded, so that a float32 restatement is bit-exact (tests/planning_reference.py
 * is one, in numpy).  For entry (s, a) of the table:
 *     n = its next state
 *     r = its reward, NaN ("None") counted as 0; with `reward_override` (DEVICE float32
 *         [n_states][5]) that array's element instead, NaN still counted as 0
 *     d = its done bit
 *     D = the frame's discount as a rollout reports it: discount_list[code], or - code 0 - 0.0
 *         when d is set and 1.0 otherwise
 *     c = gamma * D
 *     q[s][a] = d ? r : r + c * v[n]        (nothing is carried across an episode's end: the cut
 *                                            and the operation order of campx_returns_launch())
 * Policy reduction (`policy` DEVICE float32 [n_states][5], the weights
 * campx_wide_policy_update_launch() samples from), with w = policy[s]:
 *     c4    = (((w0 + w1) + w2) + w3) + w4                          (the sampler's own total)
 *     v'[s] = (((((w0*q0) + w1*q1) + w2*q2) + w3*q3) + w4*q4) / c4
 * A row that the sampler calls BAD - a negative or NaN weight, a c4 that is not a positive finite
 * number - takes action 4 as it does there: v'[s] = q[s][4].  Such rows are counted into
 * *bad_rows (DEVICE int32, added to, may be NULL) once per call, and *bad_flag (device or mapped
 * pinned int32, may be NULL) is set to 1.
 * Greedy reduction (`policy` NULL): v'[s] = max over a of q[s][a], found as  best = q0; for a = 1
 * .. 4: if (q[a] > best) best = q[a]  - so the greedy action is the lowest a attaining it (among
 * several +inf too); a NaN at a = 1 .. 4 never wins, a NaN q0 is never displaced.
 * All of this holds over all of float32: subnormals are kept (nothing is flushed, the division by
 * a subnormal c4 included), zeros keep their sign, a NaN or an infinity in `v_in` propagates,
 * `0 * inf` and `inf - inf` are NaN and are written as such; the payload and sign of a generated
 * NaN are unspecified.
 *
 * Sweeps are Jacobi.  With v_0 = `v_in`, for k = 1 .. n_sweeps:
 *     q_k = the backup of v_{k-1}        v_k = the reduction of q_k
 *     residual[k-1] = the float whose bit pattern is the largest, over s, of the bit patterns of
 *                     |v_k[s] - v_{k-1}[s]|   (a maximum of integers: order-independent; a NaN
 *                     difference wins it and shows as NaN)
 * `v_out` = v_n; `q` (DEVICE float32 [n_states][5], may be NULL) = q_n, so that v_out is exactly
 * the reduction of the returned q; `greedy` (DEVICE int8 [n_states], may be NULL) = the greedy
 * action of q_n (4 in every row under a policy).  n sweeps and then m more from the v_out of the
 * first call are n + m sweeps, bit for bit.
 *
 * Two paths, `path`: 1 = one workgroup stages the entries, two value vectors and the policy in
 * LDS and runs all n_sweeps in ONE launch, a workgroup barrier between sweeps; 2 = one launch per
 * sweep, a lane per state, between `v_out` and `scratch` (DEVICE float32 [n_states], needed on
 * this path only), after one small kernel that zeroes `residual`; the launches follow each other
 * on `stream`, a sweep boundary is a kernel boundary.  0 = path 1 whenever the table fits the
 * library setting wide_lds_max.  By the rule the choice cannot change a bit of any result.
 * `v_in` may be `v_out`; otherwise `v_in` is left as it is.
 *
 * campx_wide_sweeps_plan() is the choice as host-only arithmetic (nothing is launched):
 * plan_out[4] = the path taken (1 / 2); dynamic LDS bytes (0 on path 2); threads of a workgroup;
 * workgroups of a sweep.  `policy` is 1 for the policy reduction and 0 for the greedy one;
 * `has_override` is accepted for completeness - the staged entry holds the reward the sweeps use,
 * wherever it came from, so an override takes no LDS of its own.  CAMPX_EINVAL: n_states outside
 * 1 .. CAMPX_WIDE_MAX_STATES, a flag that is not 0 / 1, wide_lds_max < 0, a `path` outside 0..2,
 * path 1 for a table that does not fit.  campx_wide_sweeps_launch() returns CAMPX_EINVAL for the
 * same and for: NULL where it is not allowed, pointers that are not 4-byte aligned, n_sweeps
 * outside 1 .. 2^20, a gamma that is not finite, `v_in` and `v_out` that overlap without being
 * equal, on path 2 a `scratch` that is NULL or overlaps either.  Asynchronous on `stream`, no
 * synchronisation, no allocation, no library state.
 */
int32_t campx_wide_sweeps_plan(int64_t n_states, int32_t policy, int32_t has_override,
                               int64_t wide_lds_max, int32_t path, int64_t* plan_out);
int32_t campx_wide_sweeps_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                 const float* policy, const float* reward_override, float gamma,
                                 const float* v_in, float* v_out, float* scratch, float* q,
                                 int8_t* greedy, float* residual, int32_t* bad_rows,
                                 int32_t* bad_flag, int32_t n_sweeps, int32_t path, void* stream);
/*
 * ---- The same for a population of policies, in one launch --------------------------------------
 * Member m of campx_wide_population_sweeps_launch() IS campx_wide_sweeps_launch() of the policy
 * `policies[m]` with the factor gamma[m]: the rule above, policy reduction, word for word, and so
 * the same bits - whatever `members` is, whichever workgroup or lane takes the member, however
 * members are packed, on either path.  Both launches are one launch inside: members = 1 with
 * `gammas` NULL runs campx_wide_sweeps_launch()'s own kernels (planned as a population of one);
 * members = 1 with a `gammas` runs the population's.
 *   policies          DEVICE float32 [members][n_states][5]; members * n_states * 5 <= 2^31 - 1
 *   gammas            DEVICE float32 [members], or NULL: the scalar `gamma`, which must then be
 *                     finite, holds for every member.  `gammas` is never read on the host: a NaN
 *                     or an infinity in it propagates through c = gamma * D as the rule says
 *   reward_override   DEVICE float32 [n_states][5] shared by all members, or NULL
 *   v_in, v_out       DEVICE float32 [members][n_states]; they may be the same array
 *   scratch           DEVICE float32 [members][n_states], needed on path 2 only
 *   q                 DEVICE float32 [members][n_states][5] = each member's q_n, or NULL
 *   residual          DEVICE float32 [n_sweeps][members]: residual[k-1][m] is member m's for sweep k
 *   bad_rows          bad rows summed over the members, once per call (as above)
 * Path 1: a workgroup stages the entries in LDS once and takes G consecutive members - their value
 * vectors, weights, totals and gammas in LDS too - through all n_sweeps in the ONE launch, one
 * workgroup barrier per sweep; ceil(members / G) workgroups.  Path 2: one launch per sweep, a lane
 * per (member, state), a workgroup per 256 states of one member, all members' blocks along grid.x,
 * between `v_out` and `scratch` after one small kernel that zeroes `residual`.  0 = path 1
 * whenever ONE member fits the library setting wide_lds_max.  Either grid stops at 2^20
 * workgroups, each then taking several groups in turn.
 *
 * campx_wide_population_sweeps_plan() is the choice as host-only arithmetic: plan_out[5] = the
 * path; dynamic LDS bytes; threads of a workgroup; workgroups launched; G (1 on path 2).  G is the
 * least of: what fits wide_lds_max; floor(256 / n_states) or 1, about four waves of (member,
 * state) pairs to a workgroup; ceil(members / n_cus), so that a small population still spreads
 * over the chip's `n_cus` compute units.  CAMPX_EINVAL: plan_out NULL, n_states outside 1 ..
 * CAMPX_WIDE_MAX_STATES, members < 1, members * n_states * 5 above 2^31 - 1, a flag that is not
 * 0 / 1, n_cus < 1, wide_lds_max < 0, a `path` outside 0..2, path 1 where one member does not fit.
 * The launch returns CAMPX_EINVAL for the same and for: NULL where it is not allowed, pointers
 * that are not 4-byte aligned, n_sweeps outside 1 .. 2^20, `gammas` NULL with a `gamma` that is
 * not finite, `v_in` and `v_out` that overlap without being equal, on path 2 a `scratch` that is
 * NULL or overlaps either.  Asynchronous on `stream`, no synchronisation, no allocation, no
 * library state.
 */
int32_t campx_wide_population_sweeps_plan(int64_t n_states, int64_t members, int32_t has_override,
                                          int64_t wide_lds_max, int64_t n_cus, int32_t path,
                                          int64_t* plan_out);
int32_t campx_wide_population_sweeps_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                            const float* policies, int64_t members,
                                            const float* reward_override, float gamma,
                                            const float* gammas, const float* v_in, float* v_out,
                                            float* scratch, float* q, float* residual,
                                            int32_t* bad_rows, int32_t* bad_flag, int32_t n_sweeps,
                                            int32_t path, void* stream);
/*
 * ---- A population of rewards and gammas: either reduction, a reward table per member -----------
 * campx_wide_population_solve_launch() is the launch above with two things more.  (1) `policies`
 * may be NULL: every member then takes the GREEDY reduction - value iteration for `members`
 * rewards or gammas in one launch - and `greedy` (DEVICE int8 [members][n_states], may be NULL;
 * refused beside `policies`) receives each member's greedy action of its q_n.  (2) `rewards`
 * (DEVICE float32 [members][n_states][5], or NULL) gives member m a reward table of its own: r of
 * the rule is rewards[m][s][a], NaN counted as 0, in place of the table's reward and of
 * `reward_override`, which must then be NULL.  The rule.  Member m IS campx_wide_sweeps_launch()
 * with policy = policies[m] (or NULL), reward_override = rewards[m] (or the shared one), gamma =
 * gammas[m]: `v_out`, `q`, `greedy` and every residual[k][m], bit for bit - whatever `members` is,
 * however members are packed, on either path.  Every other argument, the two paths and the grid
 * are the population launch's; `members * n_states * 5 <= 2^31 - 1` as there.
 * Path 1 with `rewards`: the staged entries keep the shared next / done / discount-code word, and
 * a workgroup stages its G members' rewards - NaN resolved once, there - as [5][G * n_states]
 * floats, flat over the (member, state) pairs like the weights: 20 bytes per pair on top of a
 * greedy member's 8 and a policy member's 32.  Path 2 with `rewards`: a lane reads its five
 * rewards at (m * n_states + s) * 5 + a.  The largest table whose one member fits wide_lds_max so
 * differs between the four forms (policy or greedy by shared or own rewards).
 * Without `rewards`, with `policies`: the kernels of campx_wide_population_sweeps_launch(),
 * chosen as it chooses them.  A greedy population or `rewards` always run instances compiled
 * with the members, members = 1 included.
 *
 * campx_wide_population_solve_plan() is the choice as host-only arithmetic, plan_out[5] as
 * campx_wide_population_sweeps_plan() gives it; `policy` 1 / 0 for the reduction,
 * `per_member_rewards` 1 / 0.  G is that function's rule TAKEN OVER - its three bounds, with this
 * form's LDS bytes in the first - and NOT tuned for these forms.  CAMPX_EINVAL as there (either
 * flag not 0 / 1).  The launch returns CAMPX_EINVAL for the same, for what the population launch
 * refuses, and for: `rewards` beside `reward_override`, `greedy` beside `policies`, a `rewards`
 * that is not 4-byte aligned.  Every refusal of an argument is decided before the device is
 * asked anything.  Asynchronous on `stream`, no synchronisation, no allocation, no library state.
 */
int32_t campx_wide_population_solve_plan(int64_t n_states, int64_t members, int32_t policy,
                                         int32_t per_member_rewards, int64_t wide_lds_max,
                                         int64_t n_cus, int32_t path, int64_t* plan_out);
int32_t campx_wide_population_solve_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                           const float* policies, const float* rewards,
                                           int64_t members, const float* reward_override,
                                           float gamma, const float* gammas, const float* v_in,
                                           float* v_out, float* scratch, float* q, int8_t* greedy,
                                           float* residual, int32_t* bad_rows, int32_t* bad_flag,
                                           int32_t n_sweeps, int32_t path, void* stream);
/*
 * ---- Exact state visitation of a policy on the state table ------------------------------------
 * The forward half of the same MDP: given the weights campx_wide_policy_update_launch() samples
 * from, how much probability sits in each state at each frame and how often each (state, action)
 * is taken - exactly, where a rollout followed by campx_state_sums_launch() estimates it
 * (csrc/k_visit.hip).  No reference counterpart.
 *
 * Mass is an int64 in units of 2^-CAMPX_VISIT_FRAC_BITS; one environment is 2^38.  Every addition
 * below is an integer addition, so no result depends on the order a kernel adds in: both paths, a
 * continued call and a numpy restatement (tests/visitation_reference.py) agree bit for bit.
 *
 * 1. The exact action counts of a row.  For w = policy[s] (DEVICE float32 [n_states][5]) take the
 *    sampler's thresholds c0 = w0, c1 = c0 + w1, c2 = c1 + w2, c3 = c2 + w3, c4 = c3 + w4 (f32, in
 *    that order); a BAD row - a negative or NaN weight, a c4 that is not a positive finite number
 *    - has {-1, -1, -1, -1, 0}, as there.  For i = 0 .. 3, N[s][i] is the number of 24-bit values
 *    u in 0 .. 2^24 - 1 whose sampled action is at most i: the smallest u with
 *        float(u) * 2^-24 * c4 >= c_i
 *    (the sampler's own f32 multiply - float(u) * 2^-24 is exact - and its own comparison), 2^24
 *    if there is none.  The product is monotone in u: 25 bisection steps (lo = 0, hi = 2^24; mid =
 *    (lo + hi) >> 1; reached ? hi = mid : lo = mid + 1) find it.  A bad row has N = {0, 0, 0, 0}:
 *    all its mass takes action 4, as the sampler plays it; bad rows are counted into *bad_rows
 *    (DEVICE int32, added to, may be NULL) once per call and *bad_flag (device or mapped pinned
 *    int32, may be NULL) is set to 1.  N[s][4] = 2^24.
 *    counts[s][a] = N[s][a] - N[s][a-1] (N[s][-1] = 0), DEVICE int32 [n_states][5], an output:
 *    every row sums to 2^24, and counts / 2^24 is the exact probability with which the sampler
 *    takes a in s.
 * 2. Splitting a state's mass m, 0 <= m < 2^62.  For i = 0 .. 4
 *        y_i = (m >> 24) * N_i + (((m & 0xffffff) * N_i) >> 24)
 *    which is floor(m * N_i / 2^24) exactly and cannot overflow; y_4 = m.  x_a = y_a - y_{a-1},
 *    y_{-1} = 0: every x_a >= 0 and they sum to m exactly.
 * 3. One frame, from d_t to d_{t+1} (zero before the frame): for every state s with mass d_t[s]
 *    and every action a,  visits[s][a] += x_a;  if the entry of (s, a) ends the episode,
 *    finished[t] += x_a and - with `restart` - d_{t+1}[0] += x_a (the rollout's `from = done ? 0 :
 *    now`; without `restart` the mass leaves); otherwise d_{t+1}[next state of (s, a)] += x_a.
 *    Rewards, discount codes and the hidden performance play no part.
 * 4. n_frames frames from d_0 = `start` (DEVICE int64 [n_states], every entry >= 0, total <=
 *    2^38; NULL: 2^38 in state 0).  Outputs, all DEVICE, all overwritten: `visits` int64
 *    [n_states][5], summed over the frames of this call (below 2^58); `finished` int64 [n_frames];
 *    `final` int64 [n_states] = d_n; `per_frame` int64 [n_frames + 1][n_states] = d_0 .. d_n (may
 *    be NULL); `counts`.  n frames and then m more from the `final` of the first call are n + m
 *    frames bit for bit; their `visits` and `finished` add up.  `start` may be `final`; otherwise
 *    it is left as it is.
 *
 * Two paths, `path`: 1 = after the kernel that makes `counts`, one workgroup stages the entries, N
 * and two mass vectors in LDS and runs all n_frames in ONE launch, a workgroup barrier between
 * frames, the scatter by 64-bit LDS atomic adds; 2 = one launch per frame, a lane per state, the
 * scatter by 64-bit global atomic adds between `final` and `scratch` (DEVICE int64 [n_states],
 * needed on this path only; left all zero), a frame boundary is a kernel boundary.  0 = path 1
 * whenever the table fits the library setting wide_lds_max (52 bytes per state and a header) and
 * has at most 3 072 states.  By the rule the choice cannot change a bit of any result.
 *
 * campx_wide_visit_plan() is the choice as host-only arithmetic (nothing is launched):
 * plan_out[4] = the path taken (1 / 2); dynamic LDS bytes (0 on path 2); threads of a workgroup;
 * workgroups of a frame.  CAMPX_EINVAL: n_states outside 1 .. CAMPX_WIDE_MAX_STATES, wide_lds_max
 * < 0, a `path` outside 0 .. 2, path 1 for a table that does not fit.
 * campx_wide_visit_launch() returns CAMPX_EINVAL, before anything is launched, for the same and
 * for: NULL where it is not allowed (`start`, `per_frame`, `bad_rows`, `bad_flag` may be; `scratch`
 * on path 1), pointers that are not aligned (8 bytes for the int64 arrays and the tables, 4 for the
 * others), n_frames outside 1 .. 2^20, a `restart` that is not 0 / 1, `final` overlapping `start`
 * without being equal to it, on path 2 a `scratch` that overlaps either.  The contents of `start`
 * are the caller's to keep within the bounds above (the kernels do not look).  Asynchronous on
 * `stream`, no synchronisation, no allocation, no library state.
 */
#define CAMPX_VISIT_FRAC_BITS 38
int32_t campx_wide_visit_plan(int64_t n_states, int64_t wide_lds_max, int32_t path,
                              int64_t* plan_out);
int32_t campx_wide_visit_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                const float* policy, const int64_t* start, int32_t restart,
                                int32_t n_frames, int64_t* visits, int64_t* finished,
                                int64_t* final_mass, int64_t* per_frame, int32_t* counts,
                                int64_t* scratch, int32_t* bad_rows, int32_t* bad_flag,
                                int32_t path, void* stream);
/*
 * ---- The same for a population of policies, in one launch --------------------------------------
 * Member m of campx_wide_visit_population_launch() IS campx_wide_visit_launch() of the policy
 * `policies[m]` from member m's start: the rule above, steps 1 to 4, word for word - int64 units
 * of 2^-38, the bisection counts, the floor(m * N / 2^24) splits, integer additions only - and so
 * the same bits, whatever `members` is, whichever workgroup or lane takes the member, however
 * members are packed, in whatever order they come, on either path.  Members share the table and
 * nothing they write.
 *   policies          DEVICE float32 [members][n_states][5]; members * n_states * 5 <= 2^31 - 1
 *   start             DEVICE int64, NULL for 2^38 in state 0 of every member; with
 *                     start_per_member = 1 [members][n_states], member m's d_0 (it may BE `final`:
 *                     a call continued in place); with 0 [n_states], every member's d_0, read with
 *                     member stride 0, which must not overlap `final`.  Per member: entries >= 0,
 *                     total <= 2^38
 *   visits, counts    [members][n_states][5];  final, scratch  [members][n_states]
 *   finished          [n_frames][members];  per_frame  [n_frames + 1][members][n_states] or NULL:
 *                     time-major, as campx_wide_population_sweeps_launch()'s residual is
 *   bad_rows          bad rows summed over the members, once per call (as above)
 * Path 1: after the kernel that makes `counts`, a lane per (member, state) row, a workgroup stages
 * the entries' second words in LDS once and takes G consecutive members - N, two mass vectors and
 * two slots of finished[t] each, in LDS too - through all n_frames in the ONE launch, one
 * workgroup barrier per frame; ceil(members / G) workgroups.  The LDS is the single call's 64-byte
 * header, 16 more bytes for each member after the first, 20 bytes a state once and 32 bytes a
 * state per member, each part rounded up to 16: at G = 1 exactly campx_wide_visit_plan()'s, so
 * the tables that fit are the same.  Path 2: one launch per frame for all members, a workgroup per
 * 256 states of one member, all members' blocks along grid.x, between `final` and `scratch`.
 * 0 = path 1 whenever ONE member fits.  Either grid stops at 2^20 workgroups, each then taking
 * several groups in turn.  Both launches run one set of kernels, compiled with the members and
 * without: members = 1 runs campx_wide_visit_launch()'s instances, from either entry point.
 *
 * campx_wide_visit_population_plan() is the choice as host-only arithmetic: plan_out[5] = the
 * path; dynamic LDS bytes; threads of a workgroup; workgroups launched; G (1 on path 2).  G is the
 * rule of campx_wide_population_sweeps_plan(), taken over and not tuned for these kernels: the
 * least of what fits wide_lds_max, floor(256 / n_states) or 1, and ceil(members / n_cus).  With
 * G > 1 the G * n_states <= 256 pairs have a lane each, in whole waves.  CAMPX_EINVAL: plan_out
 * NULL, n_states outside 1 .. CAMPX_WIDE_MAX_STATES, members < 1, members * n_states * 5 above
 * 2^31 - 1, n_cus < 1, wide_lds_max < 0, a `path` outside 0 .. 2, path 1 where one member does not
 * fit.  The launch returns CAMPX_EINVAL, before anything is launched, for the same and for: NULL
 * where it is not allowed (as above), pointers that are not aligned (as above), n_frames outside
 * 1 .. 2^20, a `restart` or a `start_per_member` that is not 0 / 1, a start per member that
 * overlaps `final` without being equal to it, a shared start that overlaps `final`, on path 2 a
 * `scratch` that is NULL or overlaps `final` or `start`.  Asynchronous on `stream`, no
 * synchronisation, no allocation, no library state.
 */
int32_t campx_wide_visit_population_plan(int64_t n_states, int64_t members, int64_t wide_lds_max,
                                         int64_t n_cus, int32_t path, int64_t* plan_out);
int32_t campx_wide_visit_population_launch(const CampxWideSpec* spec_host, const void* tables_dev,
                                           const float* policies, int64_t members,
                                           const int64_t* start, int32_t start_per_member,
                                           int32_t restart, int32_t n_frames, int64_t* visits,
                                           int64_t* finished, int64_t* final_mass,
                                           int64_t* per_frame, int32_t* counts, int64_t* scratch,
                                           int32_t* bad_rows, int32_t* bad_flag, int32_t path,
                                           void* stream);
/* The gather launch's arithmetic for N rows of R bytes written at address `dst_addr`, pure host
 * code (tests restate it): plan_out[8] = the division-by-R constants m, sh1, sh2; N * R; the
 * bytes (16-bit formats: elements) from the first memory-aligned window's start to the output;
 * workgroups; image bytes of a wave's window; waves per workgroup. */
int32_t campx_render_gather_plan(int64_t N, int32_t R, int32_t obs_format, uint64_t dst_addr,
                                 int64_t* plan_out);

/* *bad_count (device int32, caller-zeroed) += number of ids outside 0..4 in
 * actions[0..n). */
int32_t campx_check_actions_launch(const int8_t* actions, int64_t n, int32_t* bad_count,
                                   void* stream);

/* Convert one-hot float actions [n, 5] (the reference's action format,
 * examples/boat_race.py:154-184) to ids [n]; rows that are not exactly one-hot
 * are counted in *bad_count (device int32, caller-zeroed; the reference asserts
 * sum(act) == 1, boat_race.py:48) and become id 5, which the step / rollout kernels
 * treat as "stay" and report through bad_count / bad_flag like any other bad id. */
int32_t campx_onehot_to_ids_launch(const float* onehot, int8_t* ids, int64_t n,
                                   int32_t* bad_count, void* stream);

/*
 * Settings: everything about the library's behaviour that is not an argument of a call.  ONE table
 * (campx_amd/csrc/campx_api.hip: name, default, range, what each selects; INTEGRATION.md lists
 * them).  A value is set for the process by campx_config_set() - thread-safe, takes effect with
 * the next call - or, before the library's first call, by the environment variable
 * CAMPX_CONFIG="name=value,name=value" (the library's only getenv).  campx_config_string() writes
 * "name=value name=value ..." of the EFFECTIVE values into `buf` (host, NUL-terminated, truncated to
 * buf_len) and returns the length needed including the NUL; a bench or an embedding application
 * records it beside its numbers.  campx_config_set / _get return CAMPX_EINVAL for a name that is
 * not in the table or a value outside its range.  No reference counterpart.
 */
int32_t campx_config_set(const char* name, int64_t value);
int32_t campx_config_get(const char* name, int64_t* value);
int32_t campx_config_string(char* buf, int32_t buf_len);

/* Measurement aid, not on the path (SURVEY section 8d "Bound": the measured achievable HBM write
 * bandwidth of the box, quoted next to the vendor peak): one launch that fills `n_bytes` (a
 * multiple of 16, `dst` 16-byte aligned, DEVICE memory) with the 32-bit `value` through the render
 * kernel's own store form - 16 bytes per lane, `sc0 sc1 nt`, one 2 KiB window per wave,
 * XCD-contiguous block order - and nothing else.  bench.py times it over the bytes a rollout
 * launch writes: `roofline.measured_write_ceiling_gbs`.  No reference counterpart. */
int32_t campx_write_probe_launch(void* dst, int64_t n_bytes, uint32_t value, void* stream);

const char* campx_strerror(int32_t code);
/* hipError_t of the most recent failed HIP call on this thread (0 if none). */
int32_t campx_last_hip_error(void);
/* "gfx950" etc. of device `ordinal`, written to buf (host); CAMPX_ENODEV if none. */
int32_t campx_device_arch(int32_t ordinal, char* buf, int32_t buf_len);

#ifdef __cplusplus
}
#endif
#endif /* CAMPX_HIP_H_ */
