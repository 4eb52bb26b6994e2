// campx_torch.cpp - the torch custom-op face of libcampx_hip.so.
//
// `Engine.play()` / `Engine.rollout()` / `Engine.its_showtime()` of a batched engine
// lower to these ops (campx_amd/fused.py); they are what replaces the reference's
// per-frame Python path  Engine.play -> _update_and_render -> <entity>.update ->
// _render -> renderer.render  (campx/engine.py:114-324, campx/rendering.py:104-219).
//
//   campx::reset    its_showtime(): state from the art + the first observation
//   campx::step     one Engine.play() frame for B environments
//   campx::rollout  T consecutive frames in one launch
//   campx::update / campx::render   the two kernels of a rollout as separate ops
//   campx::rollout_pipelined        the two of them over two streams, in one dispatch
//   campx::update_render            update of one rollout + render of the one before it
//   campx::shape_rollout            the shape tier (Hello World): reset / step / rollout
//   campx::wide_rollout             the wide tier (boards above 128 cells): reset / step / rollout
//   campx::wide_update              the wide tier's update pass alone (trace-only rollouts)
//   campx::wide_policy_update       the same with every frame's action sampled on the device from a
//                                   policy over the game's states (closed-loop rollouts)
//   campx::wide_policy_population   wide_policy_update for P policies, each over its block of environments
//   campx::wide_learn               online tabular learners: a Q-table per environment, T frames per launch
//   campx::wide_learn_shared        shared learners: n environments feed one Q-table, T frames per launch
//   campx::wide_learn_traces        learners with eligibility traces: Q(lambda), expected SARSA(lambda)
//   campx::wide_learn_dyna          Dyna-Q learners: n planning updates of remembered pairs a frame
//   campx::wide_learn_actor         actor-critic learners: a softmax policy and a critic per environment
//   campx::wide_learn_actor_shared  shared actor-critic learners: n environments feed one policy and critic
//   campx::render_gather / campx::wide_render_gather   sampled frames of a stored trace -> a minibatch
//   campx::wide_render_states       the observations of given states of a state-table game
//   campx::wide_render_windows      egocentric / fixed windows of them, from a trace or state ids
//   campx::returns                  discounted returns / GAE advantages of a rollout's streams
//   campx::vtrace                   V-trace targets / advantages of off-policy streams
//   campx::state_sums               per-(state, action) fixed-point sums of a rollout's streams
//   campx::table_lookup             table[states, actions] of a rollout's streams
//   campx::wide_sweeps              policy evaluation / value iteration sweeps over the state table
//   campx::wide_population_sweeps   the policy-evaluation sweeps for a population of policies
//   campx::wide_population_solve    either reduction for a population, a reward table per member
//   campx::wide_visit               exact state visitation of a policy over the state table
//   campx::wide_visit_population    the same for a population of policies
//   campx::onehot_to_ids / campx::check_actions   action-format helpers
//
// Contract: every tensor is caller-owned and contiguous; outputs are written in
// place (declared mutable in the schema, so functionalization and torch.compile see
// the writes); the work is enqueued on torch's CURRENT HIP stream of the tensors'
// device and nothing synchronises.  Registered for the CUDA dispatch key (= HIP on
// ROCm) and Meta (one boxed no-op for every op, which is also the fake-tensor implementation).
// There is deliberately no CPU kernel: calling these with CPU state raises.
// An ADInplaceOrView kernel (one boxed function, registered for every op) bumps the version
// counter of every tensor an op writes, so that autograd refuses a backward pass through a
// tensor that a later play() / rollout() has overwritten (the engine's frame buffers are
// reused) instead of silently differentiating stale data.
// (ROCm builds of torch present HIP devices as device type "cuda"; the guard and stream
// types below are torch's own names for that arrangement.)
//
// The ops only unpack tensors into the C ABI of include/campx_hip.h; all kernels
// live in csrc/k_*.hip.  Each contract a tensor has to meet is one helper in the first part of
// this file; the ops below them say which of their arguments meets which.

#include <ATen/core/Tensor.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <ATen/core/stack.h>
#include <ATen/ops/empty.h>
#include <c10/core/impl/LocalDispatchKeySet.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>
#include <torch/library.h>

#include <map>
#include <mutex>
#include <optional>
#include <string>
#include <unordered_map>

#include "campx_hip.h"

namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

const OptTensor kNone;

// torch's current stream of the current device (ask under the op's DeviceGuard)
hipStream_t current_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

void check_ok(int32_t rc, const char* what) {
  TORCH_CHECK(rc == CAMPX_OK, what, " failed: ", campx_strerror(rc), " (code ", rc, ", hipError ",
              campx_last_hip_error(), ")");
}

const CampxSpec* host_spec(const Tensor& spec_host) {
  TORCH_CHECK(spec_host.device().is_cpu() && spec_host.scalar_type() == at::kByte &&
                  spec_host.is_contiguous() && spec_host.numel() == (int64_t)sizeof(CampxSpec),
              "campx: spec_host must be a contiguous CPU uint8 tensor of ", sizeof(CampxSpec),
              " bytes (the CampxSpec blob)");
  return reinterpret_cast<const CampxSpec*>(spec_host.data_ptr());
}

// The spec struct `type` of the other tiers in host memory ...
const void* host_blob(const Tensor& spec_host, size_t bytes, const char* type) {
  TORCH_CHECK(spec_host.device().is_cpu() && spec_host.scalar_type() == at::kByte &&
                  spec_host.is_contiguous() && spec_host.numel() == (int64_t)bytes,
              "campx: spec_host must be the ", type, " blob as a CPU uint8 tensor");
  return spec_host.data_ptr();
}

const CampxWideSpec* wide_spec(const Tensor& spec_host) {
  return static_cast<const CampxWideSpec*>(host_blob(spec_host, sizeof(CampxWideSpec), "CampxWideSpec"));
}

// ... and a spec struct's copy on the device.
const void* dev_blob(const Tensor& spec_dev, size_t bytes, const char* type, const c10::Device& dev) {
  TORCH_CHECK(spec_dev.device() == dev && spec_dev.scalar_type() == at::kByte &&
                  spec_dev.is_contiguous() && spec_dev.numel() == (int64_t)bytes,
              "campx: spec_dev must be the ", type, " blob as a uint8 tensor on ", dev);
  return spec_dev.data_ptr();
}

const CampxSpec* dev_spec(const Tensor& spec_dev, const c10::Device& dev) {
  return static_cast<const CampxSpec*>(dev_blob(spec_dev, sizeof(CampxSpec), "CampxSpec", dev));
}

// The device blob campx_wide_tables_build() filled for the state-table game `hs`.
void want_wide_tables(const Tensor& tables, const CampxWideSpec* hs, const c10::Device& dev) {
  TORCH_CHECK(tables.device() == dev && tables.scalar_type() == at::kByte && tables.is_contiguous() &&
                  tables.numel() == campx_wide_tables_bytes(hs),
              "campx: tables must be the campx_wide_tables_build() blob as a uint8 tensor on ", dev);
}

// Planes of a state-table game's trace: the things, plus the scenery's variant when it has
// several - or the mask of its pieces that show (the library's rule, csrc/k_wide.hip).
inline int64_t wide_planes(const CampxWideSpec* hs) {
  return hs->n_dyn + ((hs->n_variants > 1 || hs->n_pieces > 0) ? 1 : 0);
}

void want_on(const Tensor& t, const char* name, at::ScalarType dtype, const c10::Device& dev) {
  TORCH_CHECK(t.device() == dev, "campx: ", name, " must be on ", dev, ", it is on ", t.device());
  TORCH_CHECK(t.scalar_type() == dtype, "campx: ", name, " must be ", dtype, ", it is ",
              t.scalar_type());
}

void want(const Tensor& t, const char* name, at::ScalarType dtype, const c10::Device& dev,
          c10::IntArrayRef shape) {
  want_on(t, name, dtype, dev);
  TORCH_CHECK(t.is_contiguous(), "campx: ", name, " must be contiguous");
  TORCH_CHECK(t.sizes() == shape, "campx: ", name, " must have shape ", shape, ", it has ",
              t.sizes());
}

// A [T, B] stream: contiguous within a row, its rows as far apart as stride(0) says.
void want_row_stream(const Tensor& t, const char* name, at::ScalarType dtype, const c10::Device& dev,
                     int64_t T, int64_t B) {
  want_on(t, name, dtype, dev);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == T && t.size(1) == B, "campx: ", name,
              " must have shape [", T, ", ", B, "], it has ", t.sizes());
  TORCH_CHECK(B == 1 || t.stride(1) == 1, "campx: ", name, " must be contiguous within a row");
}

// ... of a rollout.  The per-frame scalar streams [T, B] and the trace [K, T, B] may be PADDED:
// contiguous within a row, rows `pitch` >= B elements apart, the same pitch for every stream of a
// call (the planes of the trace then T * pitch apart).  rollout_buffers() pads to a multiple of
// 16 when the batch size is not one, so that every row starts aligned
// (CampxOutputs.scalar_pitch).  `pitch` is 0 until the first stream has been seen.
void want_rows(const Tensor& t, const char* name, at::ScalarType dtype, const c10::Device& dev,
               int64_t T, int64_t B, int64_t& pitch) {
  want_row_stream(t, name, dtype, dev, T, B);
  if (T == 1) {
    // One row: its own pitch is never used, but the call's pitch (taken from the planes of the
    // trace, want_trace() runs first) decides whether the update kernels store the row's last
    // 16-element group whole (row_extent()): the row must then reach that far.
    const int64_t up = (B + 15) / 16 * 16;
    if (pitch >= up) {
      const int64_t room = static_cast<int64_t>(t.storage().nbytes() / t.element_size()) -
                           t.storage_offset();
      TORCH_CHECK(room >= up, "campx: ", name, " is a [1, ", B, "] row with room for ", room,
                  " elements, but the call's trace has a padded row pitch (", pitch,
                  "): the row must reach ", up, " elements (take every buffer from rollout_buffers())");
    }
    return;
  }
  const int64_t p = t.stride(0);
  TORCH_CHECK(p >= B && (pitch == 0 || p == pitch), "campx: ", name, " has row pitch ", p,
              "; every per-frame stream of a call must have the same pitch >= B");
  pitch = p;
}

const char* entry_name(at::ScalarType entry) { return entry == at::kByte ? "uint8" : "int16"; }

// The trace a rollout writes: `entry` uint8 (one-cell tiers) or int16 (state-table tier),
// [K, T, B] - or, `frames` false, the one frame [K, B] - padded like the streams above.
// (call it before want_rows: with one frame only the planes of the trace tell the pitch)
void want_trace(const Tensor& t, at::ScalarType entry, const c10::Device& dev, int64_t K, int64_t T,
                int64_t B, int64_t& pitch, bool frames = true) {
  const bool shaped = frames ? t.dim() == 3 && t.size(0) == K && t.size(1) == T && t.size(2) == B
                             : t.dim() == 2 && t.size(0) == K && t.size(1) == B;
  TORCH_CHECK(t.device() == dev && t.scalar_type() == entry && shaped, "campx: trace must be ",
              entry_name(entry), " [", K, ", ", frames ? c10::str(T, ", ") : std::string(), B,
              "] on ", dev);
  TORCH_CHECK(B == 1 || t.stride(frames ? 2 : 1) == 1, "campx: trace must be contiguous within a row");
  int64_t p = pitch;
  if (frames && T > 1) p = t.stride(1);
  else if (K > 1) p = t.stride(0);
  if (p == 0) return;            // one frame, one plane: nothing to tell
  TORCH_CHECK(p >= B && (pitch == 0 || p == pitch) && (K == 1 || !frames || t.stride(0) == T * p),
              "campx: trace must have the row pitch of the other per-frame streams and planes "
              "T * pitch apart");
  pitch = p;
}

// A STORED trace, as the gather and window ops read it: [planes, T', B] of any T', rows and
// planes as far apart as the strides say (a view of a padded buffer, a ring of several rollouts).
struct StoredTrace {
  int64_t T, B, pitch, plane;
};

StoredTrace want_stored_trace(const char* what, const Tensor& t, at::ScalarType entry,
                              const c10::Device& dev, int64_t planes) {
  TORCH_CHECK(t.device() == dev && t.scalar_type() == entry && t.dim() == 3 && t.size(0) == planes &&
                  t.size(1) >= 1 && t.size(2) >= 1 && (t.size(2) == 1 || t.stride(2) == 1),
              what, ": trace must be ", entry_name(entry), " [", planes, ", T, B] on ", dev,
              ", contiguous within a row");
  StoredTrace s{t.size(1), t.size(2), 0, 0};
  s.pitch = s.T > 1 ? t.stride(1) : s.B;
  s.plane = planes > 1 ? t.stride(0) : s.T * s.pitch;
  TORCH_CHECK(s.pitch >= s.B && s.plane >= s.T * s.pitch, what, ": trace rows must be >= B apart and its "
              "planes >= T * pitch apart");
  return s;
}

// The sampled (frame, environment) pairs of those ops: two index tensors [N] of one integer
// type; returns N.
int64_t want_pairs(const char* what, const Tensor& t_idx, const Tensor& e_idx, const c10::Device& dev) {
  TORCH_CHECK(t_idx.dim() == 1 && t_idx.size(0) >= 1 && t_idx.device() == dev && t_idx.is_contiguous() &&
                  (t_idx.scalar_type() == at::kLong || t_idx.scalar_type() == at::kInt),
              what, ": t_idx must be a contiguous int64 or int32 [N] tensor on ", dev);
  want(e_idx, "e_idx", t_idx.scalar_type(), dev, {t_idx.size(0)});
  return t_idx.size(0);
}

template <typename T>
T* opt_ptr(const OptTensor& t) {
  return t.has_value() ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

// Device-visible address of the bad-action flag: device memory, or pinned host memory
// (so that the host can poll it without a stream synchronisation).
int32_t* flag_ptr(const OptTensor& t, const c10::Device& dev) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kInt && t->numel() >= 1 && t->is_contiguous(),
              "campx: bad_flag must be a contiguous int32 tensor");
  if (t->device() == dev) return reinterpret_cast<int32_t*>(t->data_ptr());
  TORCH_CHECK(t->device().is_cpu() && t->is_pinned(),
              "campx: bad_flag must live on the state's device or in pinned host memory");
  void* mapped = nullptr;
  const hipError_t e = hipHostGetDevicePointer(&mapped, t->data_ptr(), 0);
  TORCH_CHECK(e == hipSuccess, "campx: hipHostGetDevicePointer(bad_flag) failed: ",
              hipGetErrorString(e));
  return static_cast<int32_t*>(mapped);
}

// The stream half of CampxOutputs: the optional per-frame streams of a call - [T, B] of the
// call's row pitch (want_trace() comes first) or, `frames` false, [B] of its one frame - and the
// bad-action counter and flag.  (`out.trace` is the caller's.)
void want_streams(CampxOutputs& out, const c10::Device& dev, int64_t T, int64_t B, int64_t pitch,
                  bool frames, const OptTensor& reward, const OptTensor& discount,
                  const OptTensor& step_done, const OptTensor& perf, const OptTensor& bad_count,
                  const OptTensor& bad_flag) {
  const struct { const OptTensor& t; const char* name; at::ScalarType dtype; } streams[] = {
      {reward, "reward", at::kFloat}, {discount, "discount", at::kFloat},
      {step_done, "step_done", at::kByte}, {perf, "perf", at::kChar}};
  for (const auto& s : streams) {
    if (!s.t.has_value()) continue;
    if (frames) want_rows(*s.t, s.name, s.dtype, dev, T, B, pitch);
    else want(*s.t, s.name, s.dtype, dev, {B});
  }
  if (bad_count.has_value()) want(*bad_count, "bad_count", at::kInt, dev, {1});
  out.scalar_pitch = pitch;
  out.reward = opt_ptr<float>(reward);
  out.discount = opt_ptr<float>(discount);
  out.done = opt_ptr<uint8_t>(step_done);
  out.perf = opt_ptr<int8_t>(perf);
  out.bad_count = opt_ptr<int32_t>(bad_count);
  out.bad_flag = flag_ptr(bad_flag, dev);
}

int32_t obs_format_of(const Tensor& obs) {
  switch (obs.scalar_type()) {
    case at::kChar: return CAMPX_OBS_INT8;
    case at::kHalf: return CAMPX_OBS_F16;
    case at::kBFloat16: return CAMPX_OBS_BF16;
    default: TORCH_CHECK(false, "campx: obs must be int8, float16 or bfloat16, it is ", obs.scalar_type());
  }
  return 0;
}

// The observation half of CampxOutputs: `obs` (int8, or f16 / bf16 for a policy network) and the
// optional int8 `board`, each [T, B, ...] - every frame kept - or [B, ...] - one frame buffer,
// overwritten: the last frame.  kOne: the op has one frame; kEvery: it keeps them all; kAsGiven:
// each tensor's rank says which - `alike`, the wide tier's rule, the same for both (names the op).
enum class Frames { kOne, kEvery, kAsGiven };

void want_frames(CampxOutputs& out, const c10::Device& dev, Frames frames, int64_t T, int64_t B,
                 int64_t L, int64_t H, int64_t W, const Tensor& obs, const OptTensor& board,
                 const char* obs_name = "obs", const char* alike = nullptr) {
  out.obs_format = obs_format_of(obs);
  const bool keep = frames == Frames::kEvery || (frames == Frames::kAsGiven && obs.dim() == 5);
  if (keep) want(obs, obs_name, obs.scalar_type(), dev, {T, B, L, H, W});
  else want(obs, obs_name, obs.scalar_type(), dev, {B, L, H, W});
  out.obs = reinterpret_cast<int8_t*>(obs.data_ptr());
  out.obs_t_stride = keep ? B * L * H * W : 0;
  if (!board.has_value()) return;
  const bool bkeep = frames == Frames::kEvery || (frames == Frames::kAsGiven && board->dim() == 4);
  TORCH_CHECK(!alike || bkeep == keep, alike,
              ": obs and board must both keep every frame or both the last");
  if (bkeep) want(*board, "board", at::kChar, dev, {T, B, H, W});
  else want(*board, "board", at::kChar, dev, {B, H, W});
  out.board = reinterpret_cast<int8_t*>(board->data_ptr());
  out.board_t_stride = bkeep ? B * H * W : 0;
}

// An action stream int8 [T, B]; returns T.
int64_t want_actions(const char* what, const Tensor& actions, const c10::Device& dev, int64_t B) {
  TORCH_CHECK(actions.dim() == 2, what, ": actions must be int8 [T, B]");
  want(actions, "actions", at::kChar, dev, {actions.size(0), B});
  return actions.size(0);
}

const int8_t* ids(const Tensor& actions) { return reinterpret_cast<const int8_t*>(actions.data_ptr()); }

struct Game {
  const CampxSpec* spec_host;
  const CampxSpec* spec_dev;
  CampxState state;
  c10::Device dev;
  int64_t B, K, L, H, W;
};

Game unpack_game(const Tensor& spec_host, const Tensor& spec_dev, const Tensor& pos,
                 const Tensor& done, const OptTensor& ret, const OptTensor& pair_table) {
  const CampxSpec* hs = host_spec(spec_host);
  TORCH_CHECK(pos.device().is_cuda(), "campx: the fused tier runs on a HIP device only; state is on ",
              pos.device(), " (there is no CPU implementation of these ops)");
  const c10::Device dev = pos.device();
  TORCH_CHECK(pos.dim() == 2, "campx: pos must be [2*K, B]");
  const int64_t K = hs->n_dyn, B = pos.size(1);
  want(pos, "pos", at::kChar, dev, {2 * K, B});
  want(done, "done", at::kByte, dev, {B});
  if (ret.has_value()) want(*ret, "ret", at::kFloat, dev, {B});
  const CampxSpec* ds = dev_spec(spec_dev, dev);
  if (pair_table.has_value())
    TORCH_CHECK(pair_table->device() == dev && pair_table->is_contiguous() &&
                    pair_table->nbytes() == (size_t)campx_pair_table_bytes(hs),
                "campx: pair_table has the wrong size or device");
  return Game{hs,
              ds,
              CampxState{reinterpret_cast<int8_t*>(pos.data_ptr()),
                         reinterpret_cast<uint8_t*>(done.data_ptr()), opt_ptr<float>(ret),
                         pair_table.has_value() ? pair_table->data_ptr() : nullptr},
              dev,
              B,
              K,
              hs->n_layers,
              hs->rows,
              hs->cols};
}

// The same for a state-table game (wide tier): `tables` the device blob campx_wide_tables_build()
// filled, `state` int32 [B] the environments' state indices, K the planes of its trace.
struct WideGame {
  const CampxWideSpec* hs;
  const void* tables;
  CampxState state;
  c10::Device dev;
  int64_t B, K, L, H, W;
};

WideGame unpack_wide(const char* what, const Tensor& spec_host, const Tensor& tables,
                     const Tensor& state, const Tensor& done, const OptTensor& ret) {
  const CampxWideSpec* hs = wide_spec(spec_host);
  TORCH_CHECK(state.device().is_cuda() && state.dim() == 1, what,
              ": state must be on a HIP device (no CPU implementation)");
  const c10::Device dev = state.device();
  const int64_t B = state.size(0);
  want(state, "state", at::kInt, dev, {B});
  want(done, "done", at::kByte, dev, {B});
  if (ret.has_value()) want(*ret, "ret", at::kFloat, dev, {B});
  want_wide_tables(tables, hs, dev);
  return WideGame{hs,
                  tables.data_ptr(),
                  CampxState{reinterpret_cast<int8_t*>(state.data_ptr()),
                             reinterpret_cast<uint8_t*>(done.data_ptr()), opt_ptr<float>(ret), nullptr},
                  dev,
                  B,
                  wide_planes(hs),
                  hs->n_layers,
                  hs->rows,
                  hs->cols};
}

void reset(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
           const OptTensor& ret, const OptTensor& pair_table, Tensor& obs, const OptTensor& board) {
  const Game g = unpack_game(spec_host, spec_dev, pos, done, ret, pair_table);
  want(obs, "obs", at::kChar, g.dev, {g.B, g.L, g.H, g.W});
  if (board.has_value()) want(*board, "board", at::kChar, g.dev, {g.B, g.H, g.W});
  CampxOutputs out{};
  out.obs = reinterpret_cast<int8_t*>(obs.data_ptr());
  out.board = opt_ptr<int8_t>(board);
  const DeviceGuard guard(g.dev);
  check_ok(campx_reset_launch(g.spec_host, g.spec_dev, g.state, out, g.B, current_stream()),
           "campx_reset_launch");
}

void rollout(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
             const OptTensor& ret, const OptTensor& pair_table, const Tensor& actions, Tensor& obs,
             const OptTensor& board, const OptTensor& reward, const OptTensor& discount,
             const OptTensor& step_done, const OptTensor& perf, const OptTensor& trace,
             const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first,
             const OptTensor& scratch, const OptTensor& scratch_state, const OptTensor& error_flag) {
  const Game g = unpack_game(spec_host, spec_dev, pos, done, ret, pair_table);
  const int64_t T = want_actions("campx::rollout", actions, g.dev, g.B);
  TORCH_CHECK(T <= 0x7fffffff, "campx::rollout: too many frames");
  CampxOutputs out{};
  want_frames(out, g.dev, Frames::kAsGiven, T, g.B, g.L, g.H, g.W, obs, board);
  int64_t pitch = 0;
  if (trace.has_value()) want_trace(*trace, at::kByte, g.dev, g.K, T, g.B, pitch);
  want_streams(out, g.dev, T, g.B, pitch, true, reward, discount, step_done, perf, bad_count, bad_flag);
  out.trace = opt_ptr<uint8_t>(trace);
  if (scratch.has_value()) {   // CampxOutputs.overlap_ctl: zeroed once by its owner
    // (how many bytes each user of it needs is the library's check: too small a block only
    // means the launch takes another path)
    TORCH_CHECK(scratch->device() == g.dev && scratch->scalar_type() == at::kInt &&
                    scratch->is_contiguous() && scratch->numel() >= 4,
                "campx::rollout: scratch must be a contiguous int32 tensor on ", g.dev);
    out.overlap_ctl = reinterpret_cast<uint32_t*>(scratch->data_ptr());
    out.overlap_ctl_bytes = scratch->numel() * 4;
    // the block's CampxFlowState lives with its owner, in host memory: six int64 (zeroed when
    // the block was allocated); without it, or without an error word, the library runs two launches
    if (scratch_state.has_value()) {
      TORCH_CHECK(scratch_state->device().is_cpu() && scratch_state->scalar_type() == at::kLong &&
                      scratch_state->is_contiguous() &&
                      scratch_state->numel() * 8 == (int64_t)sizeof(CampxFlowState),
                  "campx::rollout: scratch_state must be a contiguous CPU int64 tensor of ",
                  sizeof(CampxFlowState) / 8, " elements");
      out.flow_state = reinterpret_cast<CampxFlowState*>(scratch_state->data_ptr());
    }
  }
  out.error_flag = flag_ptr(error_flag, g.dev);
  const DeviceGuard guard(g.dev);
  check_ok(campx_rollout_launch(g.spec_host, g.spec_dev, g.state, ids(actions), out, g.B, (int32_t)T,
                                reset_first ? 1 : 0, current_stream()),
           "campx_rollout_launch");
}

// The two halves of the two-kernel rollout path as ops of their own, so that a caller
// can issue them on different streams (fused.py rollout(pipelined=True)).
void update(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
            const OptTensor& ret, const OptTensor& pair_table, const Tensor& actions,
            const OptTensor& reward, const OptTensor& discount, const OptTensor& step_done,
            const OptTensor& perf, Tensor& trace, const OptTensor& bad_count,
            const OptTensor& bad_flag, bool reset_first) {
  const Game g = unpack_game(spec_host, spec_dev, pos, done, ret, pair_table);
  const int64_t T = want_actions("campx::update", actions, g.dev, g.B);
  TORCH_CHECK(T >= 1 && T <= 0x7fffffff, "campx::update: bad frame count");
  int64_t pitch = 0;
  want_trace(trace, at::kByte, g.dev, g.K, T, g.B, pitch);
  CampxOutputs out{};
  want_streams(out, g.dev, T, g.B, pitch, true, reward, discount, step_done, perf, bad_count, bad_flag);
  out.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  const DeviceGuard guard(g.dev);
  check_ok(campx_update_launch(g.spec_host, g.spec_dev, g.state, ids(actions), out, g.B, (int32_t)T,
                               reset_first ? 1 : 0, current_stream()),
           "campx_update_launch");
}

void render(const Tensor& spec_host, const Tensor& spec_dev, const Tensor& trace, Tensor& obs,
            const OptTensor& board) {
  const CampxSpec* hs = host_spec(spec_host);
  TORCH_CHECK(trace.device().is_cuda() && trace.dim() == 3, "campx::render: trace must be a HIP uint8 [K, T, B] tensor");
  const c10::Device dev = trace.device();
  const int64_t K = hs->n_dyn, T = trace.size(1), B = trace.size(2);
  CampxOutputs out{};
  want_trace(trace, at::kByte, dev, K, T, B, out.scalar_pitch);
  const CampxSpec* ds = dev_spec(spec_dev, dev);
  want_frames(out, dev, Frames::kEvery, T, B, hs->n_layers, hs->rows, hs->cols, obs, board);
  out.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  const DeviceGuard guard(dev);
  check_ok(campx_render_launch(hs, ds, out, B, (int32_t)T, current_stream()), "campx_render_launch");
}

// A rollout over TWO streams (fused.py rollout(pipelined=True), in C++ since round 5): the update
// pass on a HIGH-priority side stream, the render on the caller's stream behind it - so that the
// update pass of the NEXT call runs under this call's render.  What makes it pay is the host: as
// two op dispatches and five stream / event calls from Python it cost 36-46 us per call, more
// than a middle-sized rollout takes (sokoban B = 16 384: 62 us in order); here it is one dispatch.
// The side stream and the events live in this binding layer, per device (the C library below it
// holds no state); `resync`: work has been issued on the caller's stream since the last
// pipelined call that the update pass must come after (state set up by other calls).
struct PipeStreams {
  // held for the whole body of rollout_pipelined: the op releases the GIL, so two actor threads
  // on one device would otherwise interleave their event records / waits and rehash `readers`
  // under each other (round 5 advice).  One pipelined rollout per device at a time is issued.
  std::mutex busy;
  hipStream_t side = nullptr;
  hipEvent_t updated = nullptr, synced = nullptr;
  std::unordered_map<const void*, hipEvent_t> readers;   // trace buffer -> its last render
};

void hip_ok(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "campx: ", what, " failed: ", hipGetErrorString(e));
}

PipeStreams& pipe_streams(int device) {
  static std::mutex lock;
  static std::map<int, PipeStreams> all;
  std::lock_guard<std::mutex> hold(lock);
  PipeStreams& p = all[device];
  if (!p.side) {
    int least = 0, greatest = 0;
    hip_ok(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
    hip_ok(hipStreamCreateWithPriority(&p.side, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority");
    hip_ok(hipEventCreateWithFlags(&p.updated, hipEventDisableTiming), "hipEventCreateWithFlags");
    hip_ok(hipEventCreateWithFlags(&p.synced, hipEventDisableTiming), "hipEventCreateWithFlags");
  }
  return p;
}

void rollout_pipelined(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
                       const OptTensor& ret, const OptTensor& pair_table, const Tensor& actions,
                       Tensor& obs, const OptTensor& board, const OptTensor& reward,
                       const OptTensor& discount, const OptTensor& step_done, const OptTensor& perf,
                       Tensor& trace, const OptTensor& bad_count, const OptTensor& bad_flag,
                       bool reset_first, bool resync) {
  const Game g = unpack_game(spec_host, spec_dev, pos, done, ret, pair_table);
  const int64_t T = want_actions("campx::rollout_pipelined", actions, g.dev, g.B);
  TORCH_CHECK(T >= 1 && T <= 65535, "campx::rollout_pipelined: 1 to 65535 frames");
  int64_t pitch = 0;
  want_trace(trace, at::kByte, g.dev, g.K, T, g.B, pitch);
  CampxOutputs upd{};
  want_streams(upd, g.dev, T, g.B, pitch, true, reward, discount, step_done, perf, bad_count, bad_flag);
  upd.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  CampxOutputs ren{};
  ren.scalar_pitch = pitch;
  want_frames(ren, g.dev, Frames::kEvery, T, g.B, g.L, g.H, g.W, obs, board);
  ren.trace = upd.trace;
  const DeviceGuard guard(g.dev);
  hipStream_t main = current_stream();
  PipeStreams& p = pipe_streams(g.dev.index());
  std::lock_guard<std::mutex> one_at_a_time(p.busy);
  if (resync) {       // everything issued on the caller's stream so far, renders included
    hip_ok(hipEventRecord(p.synced, main), "hipEventRecord");
    hip_ok(hipStreamWaitEvent(p.side, p.synced, 0), "hipStreamWaitEvent");
    // (events of trace buffers last rendered before this point are covered by it)
  }
  // the side stream runs ahead of the caller's without bound; what it may not do is overwrite a
  // trace buffer whose last render is still running
  if (p.readers.size() >= 64 && !p.readers.count(upd.trace)) {
    // (a caller that allocates new buffers for every rollout: the events of buffers long gone are
    // let go - behind one wait for everything the caller's stream holds, which covers them all)
    hip_ok(hipEventRecord(p.synced, main), "hipEventRecord");
    hip_ok(hipStreamWaitEvent(p.side, p.synced, 0), "hipStreamWaitEvent");
    for (auto& kept : p.readers) (void)hipEventDestroy(kept.second);
    p.readers.clear();
  }
  hipEvent_t reader = p.readers[upd.trace];      // (by value: the map may rehash)
  if (reader && !resync) hip_ok(hipStreamWaitEvent(p.side, reader, 0), "hipStreamWaitEvent");
  check_ok(campx_update_launch(g.spec_host, g.spec_dev, g.state, ids(actions), upd, g.B, (int32_t)T,
                               reset_first ? 1 : 0, p.side),
           "campx_update_launch");
  hip_ok(hipEventRecord(p.updated, p.side), "hipEventRecord");
  hip_ok(hipStreamWaitEvent(main, p.updated, 0), "hipStreamWaitEvent");
  check_ok(campx_render_launch(g.spec_host, g.spec_dev, ren, g.B, (int32_t)T, main), "campx_render_launch");
  if (!reader) {
    hip_ok(hipEventCreateWithFlags(&reader, hipEventDisableTiming), "hipEventCreateWithFlags");
    p.readers[upd.trace] = reader;
  }
  hip_ok(hipEventRecord(reader, main), "hipEventRecord");
}

// The update pass of one rollout and the render pass of the one before it as ONE call
// (campx_update_render_launch: a single launch where the game and the shapes allow it).
void update_render(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
                   const OptTensor& ret, const OptTensor& pair_table, const Tensor& actions,
                   const OptTensor& reward, const OptTensor& discount, const OptTensor& step_done,
                   const OptTensor& perf, Tensor& trace, const OptTensor& bad_count,
                   const OptTensor& bad_flag, bool reset_first, const Tensor& prev_trace,
                   Tensor& prev_obs) {
  const Game g = unpack_game(spec_host, spec_dev, pos, done, ret, pair_table);
  const int64_t T = want_actions("campx::update_render", actions, g.dev, g.B);
  TORCH_CHECK(T >= 1 && T <= 65535, "campx::update_render: 1 to 65535 frames");
  int64_t pitch = 0;
  CampxOutputs out{}, prev{};
  want_trace(trace, at::kByte, g.dev, g.K, T, g.B, pitch);
  want_trace(prev_trace, at::kByte, g.dev, g.K, T, g.B, prev.scalar_pitch);
  TORCH_CHECK(prev_trace.data_ptr() != trace.data_ptr(),
              "campx::update_render: the two rollouts need a trace buffer each");
  want_streams(out, g.dev, T, g.B, pitch, true, reward, discount, step_done, perf, bad_count, bad_flag);
  out.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  want_frames(prev, g.dev, Frames::kEvery, T, g.B, g.L, g.H, g.W, prev_obs, kNone, "prev_obs");
  prev.trace = reinterpret_cast<uint8_t*>(prev_trace.data_ptr());
  const DeviceGuard guard(g.dev);
  check_ok(campx_update_render_launch(g.spec_host, g.spec_dev, g.state, ids(actions), out, prev, g.B,
                                      (int32_t)T, reset_first ? 1 : 0, current_stream()),
           "campx_update_render_launch");
}

// One Engine.play() frame: actions [B], per-frame outputs [B].
void step(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
          const OptTensor& ret, const OptTensor& pair_table, const Tensor& actions, Tensor& obs,
          const OptTensor& board, const OptTensor& reward, const OptTensor& discount,
          const OptTensor& step_done, const OptTensor& perf, const OptTensor& bad_count,
          const OptTensor& bad_flag) {
  const Game g = unpack_game(spec_host, spec_dev, pos, done, ret, pair_table);
  want(actions, "actions", at::kChar, g.dev, {g.B});
  CampxOutputs out{};
  want_frames(out, g.dev, Frames::kOne, 1, g.B, g.L, g.H, g.W, obs, board);
  want_streams(out, g.dev, 1, g.B, 0, false, reward, discount, step_done, perf, bad_count, bad_flag);
  const DeviceGuard guard(g.dev);
  check_ok(campx_rollout_launch(g.spec_host, g.spec_dev, g.state, ids(actions), out, g.B, 1, 0,
                                current_stream()),
           "campx_rollout_launch");
}

// Shape tier (Hello World): reset (actions = None, emit_first), one frame (actions [B],
// obs [B, L, H, W]) or T frames (actions [T, B], obs [T, B, L, H, W]) through one op.
void shape_rollout(const Tensor& spec_host, const Tensor& spec_dev, Tensor& pos, Tensor& done,
                   const OptTensor& ret, const OptTensor& backdrop_state, const OptTensor& actions,
                   Tensor& obs, const OptTensor& board, const OptTensor& reward,
                   const OptTensor& discount, const OptTensor& step_done,
                   const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first,
                   bool emit_first, const OptTensor& trace, const OptTensor& tables) {
  const CampxShapeSpec* hs = static_cast<const CampxShapeSpec*>(
      host_blob(spec_host, sizeof(CampxShapeSpec), "CampxShapeSpec"));
  TORCH_CHECK(pos.device().is_cuda() && pos.dim() == 2,
              "campx::shape_rollout: state must be on a HIP device (no CPU implementation)");
  const c10::Device dev = pos.device();
  const int64_t B = pos.size(1), N = hs->n_things, L = hs->n_layers, H = hs->rows, W = hs->cols;
  want(pos, "pos", at::kChar, dev, {2 * N, B});
  want(done, "done", at::kByte, dev, {B});
  if (ret.has_value()) want(*ret, "ret", at::kFloat, dev, {B});
  if (backdrop_state.has_value()) want(*backdrop_state, "backdrop_state", at::kChar, dev, {B, H * W});
  const CampxShapeSpec* ds = static_cast<const CampxShapeSpec*>(
      dev_blob(spec_dev, sizeof(CampxShapeSpec), "CampxShapeSpec", dev));
  int64_t T = 0;
  bool frames = false;  // outputs carry a leading frame axis
  if (actions.has_value()) {
    frames = actions->dim() == 2;
    T = frames ? actions->size(0) : 1;
    if (frames) want(*actions, "actions", at::kChar, dev, {T, B});
    else want(*actions, "actions", at::kChar, dev, {B});
  }
  CampxOutputs out{};
  want_frames(out, dev, frames ? Frames::kAsGiven : Frames::kOne, T, B, L, H, W, obs, board);
  // (this tier's streams are contiguous: [T, B] with a frame axis, else [B])
  const int64_t scalars[2] = {T, B};
  const c10::IntArrayRef shape(scalars + (frames ? 0 : 1), frames ? 2 : 1);
  if (reward.has_value()) want(*reward, "reward", at::kFloat, dev, shape);
  if (discount.has_value()) want(*discount, "discount", at::kFloat, dev, shape);
  if (step_done.has_value()) want(*step_done, "step_done", at::kByte, dev, shape);
  if (bad_count.has_value()) want(*bad_count, "bad_count", at::kInt, dev, {1});
  out.reward = opt_ptr<float>(reward);
  out.discount = opt_ptr<float>(discount);
  out.done = opt_ptr<uint8_t>(step_done);
  out.bad_count = opt_ptr<int32_t>(bad_count);
  out.bad_flag = flag_ptr(bad_flag, dev);
  const void* tables_dev = nullptr;
  if (trace.has_value() && tables.has_value() && frames) {
    // the frame-major path: its scratch (campx_shape_scratch_bytes) and the game's row tables
    const int64_t need = campx_shape_scratch_bytes(hs, B, (int32_t)T);
    TORCH_CHECK(trace->device() == dev && trace->scalar_type() == at::kLong && trace->is_contiguous() &&
                    need > 0 && trace->numel() * 8 >= need,
                "campx::shape_rollout: trace must be a contiguous int64 tensor of at least ", need,
                " bytes on ", dev);
    TORCH_CHECK(tables->device() == dev && tables->scalar_type() == at::kLong && tables->is_contiguous() &&
                    tables->numel() * 8 >= campx_shape_tables_bytes(hs),
                "campx::shape_rollout: tables must hold campx_shape_tables_build()'s blob on ", dev);
    out.trace = reinterpret_cast<uint8_t*>(trace->data_ptr());
    tables_dev = tables->data_ptr();
  }
  CampxState state{reinterpret_cast<int8_t*>(pos.data_ptr()), reinterpret_cast<uint8_t*>(done.data_ptr()),
                   opt_ptr<float>(ret), nullptr};
  const DeviceGuard guard(dev);
  check_ok(campx_shape_rollout_launch(hs, ds, tables_dev, state, opt_ptr<int8_t>(backdrop_state),
                                      opt_ptr<int8_t>(actions), out, B, (int32_t)T,
                                      reset_first ? 1 : 0, emit_first ? 1 : 0, current_stream()),
           "campx_shape_rollout_launch");
}

// Wide tier (state-table games: boards above 128 cells, include/campx_hip.h): reset
// (actions = None), one frame (actions [B], outputs [B...]) or T frames (actions [T, B])
// through one op.  `trace`: int16 [K, B] / [K, T, B] (rows may be padded like the other
// per-frame streams).  With T frames, `obs` is [T, B, L, H, W] (every frame) or [B, L, H, W]
// (the last one).
void wide_rollout(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                  const OptTensor& ret, const OptTensor& actions, Tensor& obs, const OptTensor& board,
                  const OptTensor& reward, const OptTensor& discount, const OptTensor& step_done,
                  const OptTensor& perf, Tensor& trace, const OptTensor& bad_count,
                  const OptTensor& bad_flag, bool reset_first) {
  const char* what = "campx::wide_rollout";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  int64_t T = 0;
  bool frames = false;
  if (actions.has_value()) {
    frames = actions->dim() == 2;
    T = frames ? actions->size(0) : 1;
    if (frames) want(*actions, "actions", at::kChar, g.dev, {T, g.B});
    else want(*actions, "actions", at::kChar, g.dev, {g.B});
    TORCH_CHECK(T >= 1 && T <= 0x7fffffff, what, ": bad frame count");
  }
  CampxOutputs out{};
  int64_t pitch = 0;
  want_trace(trace, at::kShort, g.dev, g.K, T, g.B, pitch, frames);
  want_streams(out, g.dev, T, g.B, pitch, frames, reward, discount, step_done, perf, bad_count, bad_flag);
  out.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  want_frames(out, g.dev, frames ? Frames::kAsGiven : Frames::kOne, T, g.B, g.L, g.H, g.W, obs, board,
              "obs", what);
  if (!frames) {   // (one frame: to the library, every frame kept)
    out.obs_t_stride = g.B * g.L * g.H * g.W;
    if (board.has_value()) out.board_t_stride = g.B * g.H * g.W;
  }
  const DeviceGuard guard(g.dev);
  if (!actions.has_value())
    check_ok(campx_wide_reset_launch(g.hs, g.tables, g.state, out, g.B, current_stream()),
             "campx_wide_reset_launch");
  else
    check_ok(campx_wide_rollout_launch(g.hs, g.tables, g.state, ids(*actions), out, g.B, (int32_t)T,
                                       reset_first ? 1 : 0, current_stream()),
             "campx_wide_rollout_launch");
}

// Wide tier, the update pass alone (campx_wide_update_launch): campx::wide_rollout's T-frame form
// without observations.
void wide_update(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                 const OptTensor& ret, const Tensor& actions, const OptTensor& reward,
                 const OptTensor& discount, const OptTensor& step_done, const OptTensor& perf,
                 Tensor& trace, const OptTensor& bad_count, const OptTensor& bad_flag,
                 bool reset_first) {
  const WideGame g = unpack_wide("campx::wide_update", spec_host, tables, state, done, ret);
  const int64_t T = want_actions("campx::wide_update", actions, g.dev, g.B);
  TORCH_CHECK(T >= 1 && T <= 0x7fffffff, "campx::wide_update: bad frame count");
  int64_t pitch = 0;
  want_trace(trace, at::kShort, g.dev, g.K, T, g.B, pitch);
  CampxOutputs out{};
  want_streams(out, g.dev, T, g.B, pitch, true, reward, discount, step_done, perf, bad_count, bad_flag);
  out.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_update_launch(g.hs, g.tables, g.state, ids(actions), out, g.B, (int32_t)T,
                                    reset_first ? 1 : 0, current_stream()),
           "campx_wide_update_launch");
}

// Wide tier, closed loop: what campx::wide_policy_update (`rank` 2: `policy` float32 [n_states, 5],
// P = 1) and campx::wide_policy_population (`rank` 3: [P, n_states, 5]) share.  T is the trace's.
void closed_loop(const char* what, int rank, int64_t P, int64_t path, const Tensor& spec_host,
                 const Tensor& tables, Tensor& state, Tensor& done, const OptTensor& ret,
                 const Tensor& policy, int64_t seed, int64_t first_frame, const OptTensor& reward,
                 const OptTensor& discount, const OptTensor& step_done, const OptTensor& perf,
                 Tensor& trace, Tensor& actions_out, const OptTensor& states_out,
                 const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first) {
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  const int64_t S = g.hs->n_states, A = CAMPX_N_ACTIONS;
  const bool members = rank == 3;
  TORCH_CHECK(!members || (policy.dim() == 3 && P >= 1), what,
              ": policy must be float32 [P, n_states, 5] with P >= 1");
  if (members) want(policy, "policy", at::kFloat, g.dev, {P, S, A});
  else want(policy, "policy", at::kFloat, g.dev, {S, A});
  TORCH_CHECK(g.B % P == 0, what, ": the ", g.B, " environments do not split into ", P, " equal blocks");
  TORCH_CHECK(P * S < (1ll << 31), what, ": P * n_states must be below 2^31");
  TORCH_CHECK(first_frame >= 0, what, ": first_frame must be >= 0");
  TORCH_CHECK(path >= 0 && path <= 2, what, ": path must be 0, 1 or 2");
  TORCH_CHECK(trace.dim() == 3, what, ": trace must be int16 [K, T, B]");
  const int64_t T = trace.size(1);
  TORCH_CHECK(T >= 1 && T <= 0x7fffffff, what, ": bad frame count");
  int64_t pitch = 0;
  want_trace(trace, at::kShort, g.dev, g.K, T, g.B, pitch);
  want_rows(actions_out, "actions_out", at::kChar, g.dev, T, g.B, pitch);
  if (states_out.has_value()) want_rows(*states_out, "states_out", at::kInt, g.dev, T, g.B, pitch);
  CampxOutputs out{};
  want_streams(out, g.dev, T, g.B, pitch, true, reward, discount, step_done, perf, bad_count, bad_flag);
  out.trace = reinterpret_cast<uint8_t*>(trace.data_ptr());
  const DeviceGuard guard(g.dev);
  const float* weights = reinterpret_cast<const float*>(policy.data_ptr());
  int8_t* actions = reinterpret_cast<int8_t*>(actions_out.data_ptr());
  int32_t* rows = opt_ptr<int32_t>(states_out);
  check_ok(members ? campx_wide_policy_population_launch(
                         g.hs, g.tables, g.state, weights, (uint64_t)seed, first_frame, out, actions,
                         rows, g.B, (int32_t)T, reset_first ? 1 : 0, P, (int32_t)path, current_stream())
                   : campx_wide_policy_update_launch(
                         g.hs, g.tables, g.state, weights, (uint64_t)seed, first_frame, out, actions,
                         rows, g.B, (int32_t)T, reset_first ? 1 : 0, current_stream()),
           members ? "campx_wide_policy_population_launch" : "campx_wide_policy_update_launch");
}

// campx::wide_update with the action stream replaced by `policy` float32 [n_states, 5]; the actions taken
// and - optionally - the rows they were sampled from come back as streams of the call's row pitch.
void wide_policy_update(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                        const OptTensor& ret, const Tensor& policy, int64_t seed, int64_t first_frame,
                        const OptTensor& reward, const OptTensor& discount,
                        const OptTensor& step_done, const OptTensor& perf, Tensor& trace,
                        Tensor& actions_out, const OptTensor& states_out, const OptTensor& bad_count,
                        const OptTensor& bad_flag, bool reset_first) {
  closed_loop("campx::wide_policy_update", 2, 1, 0, spec_host, tables, state, done, ret, policy, seed,
              first_frame, reward, discount, step_done, perf, trace, actions_out, states_out, bad_count,
              bad_flag, reset_first);
}

// The same for `policy` float32 [P, n_states, 5], environment e sampling member e / (B / P); `states_out`
// holds the flat row member * n_states + state.  `path`: 0 chosen by arithmetic, 1 LDS, 2 global.
void wide_policy_population(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                            const OptTensor& ret, const Tensor& policy, int64_t seed,
                            int64_t first_frame, const OptTensor& reward, const OptTensor& discount,
                            const OptTensor& step_done, const OptTensor& perf, Tensor& trace,
                            Tensor& actions_out, const OptTensor& states_out,
                            const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first,
                            int64_t path) {
  closed_loop("campx::wide_policy_population", 3, policy.dim() == 3 ? policy.size(0) : 0, path,
              spec_host, tables, state, done, ret, policy, seed, first_frame, reward, discount,
              step_done, perf, trace, actions_out, states_out, bad_count, bad_flag, reset_first);
}

// Wide tier, online learners: what campx::wide_learn (`n` = B learners) and campx::wide_learn_shared
// (`n` = P) share - the checks of `q` float32 [n, n_states, 5], of `alpha`, `gamma`, `epsilon`
// float32 [n], of the scalars and of the window sums [ceil(frames / window), B] - and the fields
// that CampxLearner and CampxSharedLearner have in common, which carry the same names.
// `names`: what the op calls q, alpha, gamma and epsilon in its messages.
constexpr const char* kLearnerNames[4] = {"q", "alpha", "gamma", "epsilon"};
template <typename Learner>
Learner learner_fields(const char* what, const WideGame& g, int64_t n, Tensor& q, const Tensor& alpha,
                       const Tensor& gamma, const Tensor& epsilon, int64_t rule, int64_t seed,
                       int64_t first_frame, int64_t frames, int64_t window, Tensor& reward_sum,
                       const OptTensor& perf_sum, Tensor& episodes, const OptTensor& bad_count,
                       const OptTensor& bad_flag, bool reset_first, int64_t path,
                       const char* const (&names)[4] = kLearnerNames) {
  want(q, names[0], at::kFloat, g.dev, {n, g.hs->n_states, CAMPX_N_ACTIONS});
  TORCH_CHECK((reinterpret_cast<uintptr_t>(q.data_ptr()) & 15) == 0, what, ": ", names[0],
              " must be 16-byte aligned");
  want(alpha, names[1], at::kFloat, g.dev, {n});
  want(gamma, names[2], at::kFloat, g.dev, {n});
  want(epsilon, names[3], at::kFloat, g.dev, {n});
  TORCH_CHECK(rule == CAMPX_LEARN_Q || rule == CAMPX_LEARN_EXPECTED_SARSA, what,
              ": rule must be 0 (Q-learning) or 1 (expected SARSA)");
  TORCH_CHECK(first_frame >= 0, what, ": first_frame must be >= 0");
  TORCH_CHECK(frames >= 1 && frames <= 0x7fffffff, what, ": bad frame count");
  TORCH_CHECK(window >= 1 && window <= 0x7fffffff, what, ": window must be 1 .. 2^31 - 1");
  TORCH_CHECK(path >= 0 && path <= 2, what, ": path must be 0, 1 or 2");
  const int64_t W = (frames + window - 1) / window;
  want(reward_sum, "reward_sum", at::kFloat, g.dev, {W, g.B});
  if (perf_sum.has_value()) want(*perf_sum, "perf_sum", at::kInt, g.dev, {W, g.B});
  want(episodes, "episodes", at::kInt, g.dev, {W, g.B});
  if (bad_count.has_value()) want(*bad_count, "bad_count", at::kInt, g.dev, {1});
  Learner l{};
  l.q = reinterpret_cast<float*>(q.data_ptr());
  l.alpha = reinterpret_cast<const float*>(alpha.data_ptr());
  l.gamma = reinterpret_cast<const float*>(gamma.data_ptr());
  l.epsilon = reinterpret_cast<const float*>(epsilon.data_ptr());
  l.reward_sum = reinterpret_cast<float*>(reward_sum.data_ptr());
  l.perf_sum = opt_ptr<int32_t>(perf_sum);
  l.episodes = reinterpret_cast<int32_t*>(episodes.data_ptr());
  l.bad_count = opt_ptr<int32_t>(bad_count);
  l.bad_flag = flag_ptr(bad_flag, g.dev);
  l.seed = (uint64_t)seed;
  l.first_frame = first_frame;
  l.window = (int32_t)window;
  l.rule = (int32_t)rule;
  l.path = (int32_t)path;
  l.reset_first = reset_first ? 1 : 0;
  return l;
}

// Online tabular learners (campx_wide_learn_launch): environment e learns on its own table `q[e]`
// float32 [B, n_states, 5] for `frames` frames; `alpha`, `gamma`, `epsilon` float32 [B]; the window
// sums are [ceil(frames / window), B].  `rule`: 0 Q-learning, 1 expected SARSA.
void wide_learn(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                const OptTensor& ret, Tensor& q, const Tensor& alpha, const Tensor& gamma,
                const Tensor& epsilon, int64_t rule, int64_t seed, int64_t first_frame, int64_t frames,
                int64_t window, Tensor& reward_sum, const OptTensor& perf_sum, Tensor& episodes,
                const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first,
                int64_t path) {
  const char* what = "campx::wide_learn";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  TORCH_CHECK(g.B * g.hs->n_states * CAMPX_N_ACTIONS < (1ll << 31), what,
              ": B * n_states * 5 must be below 2^31");
  const CampxLearner l = learner_fields<CampxLearner>(
      what, g, g.B, q, alpha, gamma, epsilon, rule, seed, first_frame, frames, window, reward_sum,
      perf_sum, episodes, bad_count, bad_flag, reset_first, path);
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_learn_launch(g.hs, g.tables, g.state, &l, g.B, (int32_t)frames, current_stream()),
           "campx_wide_learn_launch");
}

// Shared online learners (campx_wide_shared_launch): the P = q.size(0) learners are each fed by
// B / P consecutive environments; `q` float32 [P, n_states, 5], `alpha`, `gamma`, `epsilon`
// float32 [P], `clamped` int64 [P] (written), the window sums [ceil(frames / window), B] per
// environment.  `scratch` int32 [3 * P * n_states * 5], zero on entry and left zero: the global
// path's accumulators (may be None when the launch takes the LDS path).
void wide_learn_shared(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                       const OptTensor& ret, Tensor& q, const Tensor& alpha, const Tensor& gamma,
                       const Tensor& epsilon, int64_t rule, int64_t seed, int64_t first_frame,
                       int64_t frames, int64_t window, Tensor& reward_sum, const OptTensor& perf_sum,
                       Tensor& episodes, Tensor& clamped, const OptTensor& scratch,
                       const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first,
                       int64_t path) {
  const char* what = "campx::wide_learn_shared";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  const int64_t S = g.hs->n_states, A = CAMPX_N_ACTIONS;
  TORCH_CHECK(q.dim() == 3 && q.size(0) >= 1, what, ": q must be float32 [P, n_states, 5] with P >= 1");
  const int64_t P = q.size(0);
  TORCH_CHECK(g.B % P == 0, what, ": the ", g.B, " environments do not split into ", P, " equal blocks");
  TORCH_CHECK(g.B / P <= 1024, what, ": ", g.B / P, " environments per learner are more than one "
              "workgroup holds (1024)");
  TORCH_CHECK(P * S * A < (1ll << 31), what, ": P * n_states * 5 must be below 2^31");
  CampxSharedLearner l = learner_fields<CampxSharedLearner>(
      what, g, P, q, alpha, gamma, epsilon, rule, seed, first_frame, frames, window, reward_sum,
      perf_sum, episodes, bad_count, bad_flag, reset_first, path);
  want(clamped, "clamped", at::kLong, g.dev, {P});
  if (scratch.has_value()) want(*scratch, "scratch", at::kInt, g.dev, {3 * P * S * A});
  l.clamped = reinterpret_cast<int64_t*>(clamped.data_ptr());
  l.scratch = scratch.has_value() ? scratch->data_ptr() : nullptr;
  l.scratch_bytes = scratch.has_value() ? 12 * P * S * A : 0;
  l.n_learners = P;
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_shared_launch(g.hs, g.tables, g.state, &l, g.B, (int32_t)frames, current_stream()),
           "campx_wide_shared_launch");
}

// Online learners with eligibility traces (campx_wide_traces_launch): campx::wide_learn's arguments
// and `traces` float32 [B, n_states, 5] (updated in place, as q), `lam` float32 [B], `trace`: 0
// accumulating, 1 replacing, `team`: 0 chosen by arithmetic, else the lanes of a learner.
void wide_learn_traces(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                       const OptTensor& ret, Tensor& q, Tensor& traces, const Tensor& alpha,
                       const Tensor& gamma, const Tensor& epsilon, const Tensor& lam, int64_t rule,
                       int64_t trace, int64_t seed, int64_t first_frame, int64_t frames, int64_t window,
                       Tensor& reward_sum, const OptTensor& perf_sum, Tensor& episodes,
                       const OptTensor& bad_count, const OptTensor& bad_flag, bool reset_first,
                       int64_t path, int64_t team) {
  const char* what = "campx::wide_learn_traces";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  TORCH_CHECK(g.B * g.hs->n_states * CAMPX_N_ACTIONS < (1ll << 31), what,
              ": B * n_states * 5 must be below 2^31");
  CampxTraceLearner l = learner_fields<CampxTraceLearner>(
      what, g, g.B, q, alpha, gamma, epsilon, rule, seed, first_frame, frames, window, reward_sum,
      perf_sum, episodes, bad_count, bad_flag, reset_first, path);
  want(traces, "traces", at::kFloat, g.dev, {g.B, g.hs->n_states, CAMPX_N_ACTIONS});
  TORCH_CHECK((reinterpret_cast<uintptr_t>(traces.data_ptr()) & 15) == 0, what,
              ": traces must be 16-byte aligned");
  want(lam, "lam", at::kFloat, g.dev, {g.B});
  TORCH_CHECK(trace == CAMPX_TRACE_ACCUMULATING || trace == CAMPX_TRACE_REPLACING, what,
              ": trace must be 0 (accumulating) or 1 (replacing)");
  TORCH_CHECK(team >= 0 && team <= 256 && (team & (team - 1)) == 0, what,
              ": team must be 0 or a power of two up to 256");
  l.traces = reinterpret_cast<float*>(traces.data_ptr());
  l.lam = reinterpret_cast<const float*>(lam.data_ptr());
  l.trace = (int32_t)trace;
  l.team = (int32_t)team;
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_traces_launch(g.hs, g.tables, g.state, &l, g.B, (int32_t)frames, current_stream()),
           "campx_wide_traces_launch");
}

// Dyna-Q online learners (campx_wide_dyna_launch): campx::wide_learn's arguments and the learners'
// model - `seen` int32 [B, n_states * 5] (16-byte aligned) and `n_seen` int32 [B], both updated in
// place -, `planning` int32 [B], the planning updates per frame, and `marks` int32
// [B, ceil(n_states * 5 / 32)], the global path's scratch (may be None when the launch takes the
// LDS path).
void wide_learn_dyna(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                     const OptTensor& ret, Tensor& q, Tensor& seen, Tensor& n_seen,
                     const Tensor& planning, const Tensor& alpha, const Tensor& gamma,
                     const Tensor& epsilon, int64_t rule, int64_t seed, int64_t first_frame,
                     int64_t frames, int64_t window, Tensor& reward_sum, const OptTensor& perf_sum,
                     Tensor& episodes, const OptTensor& marks, const OptTensor& bad_count,
                     const OptTensor& bad_flag, bool reset_first, int64_t path) {
  const char* what = "campx::wide_learn_dyna";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  const int64_t n_entries = g.hs->n_states * CAMPX_N_ACTIONS;
  TORCH_CHECK(g.B * n_entries < (1ll << 31), what, ": B * n_states * 5 must be below 2^31");
  CampxDynaLearner l = learner_fields<CampxDynaLearner>(
      what, g, g.B, q, alpha, gamma, epsilon, rule, seed, first_frame, frames, window, reward_sum,
      perf_sum, episodes, bad_count, bad_flag, reset_first, path);
  want(seen, "seen", at::kInt, g.dev, {g.B, n_entries});
  TORCH_CHECK((reinterpret_cast<uintptr_t>(seen.data_ptr()) & 15) == 0, what,
              ": seen must be 16-byte aligned");
  want(n_seen, "n_seen", at::kInt, g.dev, {g.B});
  want(planning, "planning", at::kInt, g.dev, {g.B});
  if (marks.has_value()) want(*marks, "marks", at::kInt, g.dev, {g.B, (n_entries + 31) / 32});
  l.seen = reinterpret_cast<int32_t*>(seen.data_ptr());
  l.n_seen = reinterpret_cast<int32_t*>(n_seen.data_ptr());
  l.planning = reinterpret_cast<const int32_t*>(planning.data_ptr());
  l.marks = opt_ptr<uint32_t>(marks);
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_dyna_launch(g.hs, g.tables, g.state, &l, g.B, (int32_t)frames, current_stream()),
           "campx_wide_dyna_launch");
}

// Actor-critic online learners (campx_wide_actor_launch): environment e owns `prefs[e]` float32
// [B, n_states, 5] and `values[e]` float32 [B, n_states], both 16-byte aligned and updated in place;
// `alpha_actor`, `alpha_critic`, `gamma` float32 [B]; the window sums as in campx::wide_learn.
// `bad_count` counts bad learners, `bad_rows` the environment-frames that met a bad row.
void wide_learn_actor(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                      const OptTensor& ret, Tensor& prefs, Tensor& values, const Tensor& alpha_actor,
                      const Tensor& alpha_critic, const Tensor& gamma, int64_t seed,
                      int64_t first_frame, int64_t frames, int64_t window, Tensor& reward_sum,
                      const OptTensor& perf_sum, Tensor& episodes, const OptTensor& bad_count,
                      const OptTensor& bad_rows, const OptTensor& bad_flag, bool reset_first,
                      int64_t path) {
  const char* what = "campx::wide_learn_actor";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  TORCH_CHECK(g.B * g.hs->n_states * CAMPX_N_ACTIONS < (1ll << 31), what,
              ": B * n_states * 5 must be below 2^31");
  // the checks the one-step learners' fields get: prefs is shaped and aligned as their q, the two
  // step sizes as their alpha and epsilon
  const CampxLearner as = learner_fields<CampxLearner>(
      what, g, g.B, prefs, alpha_actor, gamma, alpha_critic, CAMPX_LEARN_Q, seed, first_frame, frames,
      window, reward_sum, perf_sum, episodes, bad_count, bad_flag, reset_first, path);
  want(values, "values", at::kFloat, g.dev, {g.B, g.hs->n_states});
  TORCH_CHECK((reinterpret_cast<uintptr_t>(values.data_ptr()) & 15) == 0, what,
              ": values must be 16-byte aligned");
  if (bad_rows.has_value()) want(*bad_rows, "bad_rows", at::kInt, g.dev, {1});
  CampxActorLearner l{};
  l.prefs = as.q;
  l.values = reinterpret_cast<float*>(values.data_ptr());
  l.alpha_actor = as.alpha;
  l.alpha_critic = as.epsilon;
  l.gamma = as.gamma;
  l.reward_sum = as.reward_sum;
  l.perf_sum = as.perf_sum;
  l.episodes = as.episodes;
  l.bad_count = as.bad_count;
  l.bad_rows = opt_ptr<int32_t>(bad_rows);
  l.bad_flag = as.bad_flag;
  l.seed = as.seed;
  l.first_frame = as.first_frame;
  l.window = as.window;
  l.path = as.path;
  l.reset_first = as.reset_first;
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_actor_launch(g.hs, g.tables, g.state, &l, g.B, (int32_t)frames, current_stream()),
           "campx_wide_actor_launch");
}

// Shared actor-critic learners (campx_wide_actor_shared_launch): the P = prefs.size(0) learners are
// each fed by B / P consecutive environments; `prefs` float32 [P, n_states, 5] and `values` float32
// [P, n_states], both 16-byte aligned and updated in place; `alpha_actor`, `alpha_critic`, `gamma`
// float32 [P]; `clamped` int64 [P] (written); the window sums [ceil(frames / window), B] per
// environment.  `scratch` int32 [11 * P * n_states], zero on entry and left zero: the global path's
// accumulators (may be None when the launch takes the LDS path).
void wide_learn_actor_shared(const Tensor& spec_host, const Tensor& tables, Tensor& state, Tensor& done,
                             const OptTensor& ret, Tensor& prefs, Tensor& values,
                             const Tensor& alpha_actor, const Tensor& alpha_critic, const Tensor& gamma,
                             int64_t seed, int64_t first_frame, int64_t frames, int64_t window,
                             Tensor& reward_sum, const OptTensor& perf_sum, Tensor& episodes,
                             Tensor& clamped, const OptTensor& scratch, const OptTensor& bad_count,
                             const OptTensor& bad_rows, const OptTensor& bad_flag, bool reset_first,
                             int64_t path) {
  const char* what = "campx::wide_learn_actor_shared";
  const WideGame g = unpack_wide(what, spec_host, tables, state, done, ret);
  const int64_t S = g.hs->n_states, A = CAMPX_N_ACTIONS;
  TORCH_CHECK(prefs.dim() == 3 && prefs.size(0) >= 1, what,
              ": prefs must be float32 [P, n_states, 5] with P >= 1");
  const int64_t P = prefs.size(0);
  TORCH_CHECK(g.B % P == 0, what, ": the ", g.B, " environments do not split into ", P, " equal blocks");
  TORCH_CHECK(g.B / P <= 1024, what, ": ", g.B / P, " environments per learner are more than one "
              "workgroup holds (1024)");
  TORCH_CHECK(P * S * A < (1ll << 31), what, ": P * n_states * 5 must be below 2^31");
  // the checks the shared learners' fields get: prefs is shaped and aligned as their q, the two step
  // sizes as their alpha and epsilon
  static constexpr const char* names[4] = {"prefs", "alpha_actor", "gamma", "alpha_critic"};
  const CampxSharedLearner as = learner_fields<CampxSharedLearner>(
      what, g, P, prefs, alpha_actor, gamma, alpha_critic, CAMPX_LEARN_Q, seed, first_frame, frames,
      window, reward_sum, perf_sum, episodes, bad_count, bad_flag, reset_first, path, names);
  want(values, "values", at::kFloat, g.dev, {P, S});
  TORCH_CHECK((reinterpret_cast<uintptr_t>(values.data_ptr()) & 15) == 0, what,
              ": values must be 16-byte aligned");
  want(clamped, "clamped", at::kLong, g.dev, {P});
  if (scratch.has_value()) want(*scratch, "scratch", at::kInt, g.dev, {11 * P * S});
  if (bad_rows.has_value()) want(*bad_rows, "bad_rows", at::kInt, g.dev, {1});
  CampxSharedActorLearner l{};
  l.prefs = as.q;
  l.values = reinterpret_cast<float*>(values.data_ptr());
  l.alpha_actor = as.alpha;
  l.alpha_critic = as.epsilon;
  l.gamma = as.gamma;
  l.reward_sum = as.reward_sum;
  l.perf_sum = as.perf_sum;
  l.episodes = as.episodes;
  l.clamped = reinterpret_cast<int64_t*>(clamped.data_ptr());
  l.scratch = scratch.has_value() ? scratch->data_ptr() : nullptr;
  l.scratch_bytes = scratch.has_value() ? 44 * P * S : 0;
  l.bad_count = as.bad_count;
  l.bad_rows = opt_ptr<int32_t>(bad_rows);
  l.bad_flag = as.bad_flag;
  l.seed = as.seed;
  l.first_frame = as.first_frame;
  l.n_learners = P;
  l.window = as.window;
  l.path = as.path;
  l.reset_first = as.reset_first;
  const DeviceGuard guard(g.dev);
  check_ok(campx_wide_actor_shared_launch(g.hs, g.tables, g.state, &l, g.B, (int32_t)frames,
                                          current_stream()),
           "campx_wide_actor_shared_launch");
}

// Sampled frames of a stored trace rendered into a minibatch (campx_render_gather_launch /
// campx_wide_render_gather_launch): row i of `obs` [N, L, H, W] is the observation of frame
// t_idx[i], environment e_idx[i] of `trace` (want_stored_trace()).  Requests past the
// kernel's 32-bit bound go as several launches of a multiple of 16 rows each.
template <typename Launch>
void gather_rows(const char* what, const Tensor& trace, at::ScalarType entry, int64_t planes,
                 int64_t L, int64_t H, int64_t W, const Tensor& t_idx, const Tensor& e_idx, Tensor& obs,
                 const OptTensor& bad_count, const OptTensor& bad_flag, bool streaming, Launch launch) {
  TORCH_CHECK(trace.device().is_cuda(), what, ": trace must be on a HIP device (no CPU implementation)");
  const c10::Device dev = trace.device();
  const StoredTrace s = want_stored_trace(what, trace, entry, dev, planes);
  const int64_t N = want_pairs(what, t_idx, e_idx, dev);
  want(obs, "obs", obs.scalar_type(), dev, {N, L, H, W});
  if (bad_count.has_value()) want(*bad_count, "bad_count", at::kInt, dev, {1});
  CampxGather g{};
  g.trace = trace.data_ptr();
  g.n_planes = planes;
  g.T = s.T;
  g.pitch = s.pitch;
  g.plane = s.plane;
  g.idx64 = t_idx.scalar_type() == at::kLong ? 1 : 0;
  g.obs_format = obs_format_of(obs);
  g.bad_count = opt_ptr<int32_t>(bad_count);
  g.bad_flag = flag_ptr(bad_flag, dev);
  g.streaming = streaming ? 1 : 0;
  const int64_t row_bytes = L * H * W, idx_bytes = g.idx64 ? 8 : 4, elem = obs.element_size();
  const int64_t most = (((1ll << 32) - 65536 - 1) / row_bytes) & ~(int64_t)15;
  const DeviceGuard guard(dev);
  void* stream = current_stream();
  for (int64_t n0 = 0; n0 < N; n0 += most) {
    g.N = N - n0 < most ? N - n0 : most;
    g.t_idx = static_cast<const char*>(t_idx.data_ptr()) + n0 * idx_bytes;
    g.e_idx = static_cast<const char*>(e_idx.data_ptr()) + n0 * idx_bytes;
    g.obs = static_cast<char*>(obs.data_ptr()) + n0 * row_bytes * elem;
    check_ok(launch(&g, s.B, stream), what);
  }
}

void render_gather(const Tensor& spec_host, const Tensor& spec_dev, const Tensor& trace,
                   const Tensor& t_idx, const Tensor& e_idx, Tensor& obs, const OptTensor& bad_count,
                   const OptTensor& bad_flag, bool streaming) {
  const CampxSpec* hs = host_spec(spec_host);
  const CampxSpec* ds = dev_spec(spec_dev, trace.device());
  gather_rows("campx::render_gather", trace, at::kByte, hs->n_dyn, hs->n_layers, hs->rows, hs->cols,
              t_idx, e_idx, obs, bad_count, bad_flag, streaming,
              [&](const CampxGather* g, int64_t B, void* stream) {
                return campx_render_gather_launch(hs, ds, g, B, stream);
              });
}

void wide_render_gather(const Tensor& spec_host, const Tensor& tables, const Tensor& trace,
                        const Tensor& t_idx, const Tensor& e_idx, Tensor& obs,
                        const OptTensor& bad_count, const OptTensor& bad_flag, bool streaming) {
  const CampxWideSpec* hs = wide_spec(spec_host);
  want_wide_tables(tables, hs, trace.device());
  const void* blob = tables.data_ptr();
  gather_rows("campx::wide_render_gather", trace, at::kShort, wide_planes(hs), hs->n_layers, hs->rows,
              hs->cols, t_idx, e_idx, obs, bad_count, bad_flag, streaming,
              [&](const CampxGather* g, int64_t B, void* stream) {
                return campx_wide_render_gather_launch(hs, blob, g, B, stream);
              });
}

// Wide tier: the observations of the states `state_ids` int32 / int64 [N] (None: all of them, row
// i is state i) as `obs` [N, L, H, W] (campx_wide_render_states_launch).  `scratch`: the one-frame
// trace the launch writes, any contiguous tensor of campx_wide_render_states_scratch_bytes() on
// the device; None: allocated here (a caller that captures the op into a graph brings its own).
void wide_render_states(const Tensor& spec_host, const Tensor& tables, const OptTensor& state_ids,
                        Tensor& obs, const OptTensor& scratch, const OptTensor& bad_count,
                        const OptTensor& bad_flag) {
  const CampxWideSpec* hs = wide_spec(spec_host);
  TORCH_CHECK(tables.device().is_cuda(), "campx::wide_render_states: tables must be on a HIP device "
              "(no CPU implementation)");
  const c10::Device dev = tables.device();
  want_wide_tables(tables, hs, dev);
  TORCH_CHECK(obs.dim() == 4 && obs.size(0) >= 1, "campx::wide_render_states: obs must be [N, L, H, W]");
  const int64_t N = obs.size(0);
  want(obs, "obs", obs.scalar_type(), dev, {N, hs->n_layers, hs->rows, hs->cols});
  const int32_t format = obs_format_of(obs);
  if (state_ids.has_value()) {
    TORCH_CHECK(state_ids->scalar_type() == at::kLong || state_ids->scalar_type() == at::kInt,
                "campx::wide_render_states: state_ids must be int64 or int32");
    want(*state_ids, "state_ids", state_ids->scalar_type(), dev, {N});
  }
  if (bad_count.has_value()) want(*bad_count, "bad_count", at::kInt, dev, {1});
  const int64_t need = campx_wide_render_states_scratch_bytes(hs, N);
  TORCH_CHECK(need > 0, "campx::wide_render_states: bad spec or row count");
  const DeviceGuard guard(dev);
  Tensor trace;
  if (scratch.has_value()) {
    TORCH_CHECK(scratch->device() == dev && scratch->is_contiguous() && (int64_t)scratch->nbytes() >= need,
                "campx::wide_render_states: scratch must be a contiguous tensor of at least ", need,
                " bytes on ", dev);
    trace = *scratch;
  } else {
    trace = at::empty({need}, obs.options().dtype(at::kByte));
  }
  check_ok(campx_wide_render_states_launch(
               hs, tables.data_ptr(), state_ids.has_value() ? state_ids->data_ptr() : nullptr,
               state_ids.has_value() && state_ids->scalar_type() == at::kLong ? 1 : 0, N,
               obs.data_ptr(), format, trace.data_ptr(), (int64_t)trace.nbytes(),
               opt_ptr<int32_t>(bad_count), flag_ptr(bad_flag, dev), current_stream()),
           "campx_wide_render_states_launch");
}

// Wide tier: observation windows (campx_wide_render_windows_launch; include/campx_hip.h has the
// rule).  `source` 0: rows (t_idx[i], e_idx[i]) of `trace`, `obs` [N, L, h, w]; 1: the whole trace,
// `obs` [T, B, L, h, w]; 2: the states `t_idx` of the table (None: all of them, row i is state i),
// `obs` [N, L, h, w].  `thing` >= 0: egocentric on that plane; -1: fixed at (r0, c0).
// `layer_of_cell`: uint8 [max(n_variants, 1), 1024] on the device.
void wide_render_windows(const Tensor& spec_host, const Tensor& tables, const Tensor& layer_of_cell,
                         int64_t source, const OptTensor& trace, const OptTensor& t_idx,
                         const OptTensor& e_idx, Tensor& obs, int64_t h, int64_t w, int64_t thing,
                         int64_t r0, int64_t c0, int64_t pad_layer, const OptTensor& bad_count,
                         const OptTensor& bad_flag, bool streaming) {
  const char* what = "campx::wide_render_windows";
  const CampxWideSpec* hs = wide_spec(spec_host);
  TORCH_CHECK(tables.device().is_cuda(), what, ": tables must be on a HIP device (no CPU implementation)");
  const c10::Device dev = tables.device();
  want_wide_tables(tables, hs, dev);
  const int64_t V = hs->n_variants > 1 ? hs->n_variants : 1;
  want(layer_of_cell, "layer_of_cell", at::kByte, dev, {V, CAMPX_WIDE_MAX_CELLS});
  TORCH_CHECK(source >= CAMPX_WINDOWS_PAIRS && source <= CAMPX_WINDOWS_STATES, what, ": source must be 0, 1 or 2");
  TORCH_CHECK(h >= 1 && w >= 1 && h <= 2 * hs->rows - 1 && w <= 2 * hs->cols - 1, what,
              ": a window of ", h, " x ", w, " on a board of ", hs->rows, " x ", hs->cols);
  const int64_t L = hs->n_layers;
  CampxWindows q{};
  q.source = (int32_t)source;
  int64_t B = 1;
  if (source != CAMPX_WINDOWS_STATES) {
    TORCH_CHECK(trace.has_value(), what, ": this source needs a trace");
    const StoredTrace s = want_stored_trace(what, *trace, at::kShort, dev, wide_planes(hs));
    B = s.B;
    q.trace = trace->data_ptr();
    q.n_planes = wide_planes(hs);
    q.T = s.T;
    q.pitch = s.pitch;
    q.plane = s.plane;
  }
  if (source == CAMPX_WINDOWS_PAIRS) {
    TORCH_CHECK(t_idx.has_value() && e_idx.has_value(), what, ": sampled pairs need t_idx and e_idx");
    q.N = want_pairs(what, *t_idx, *e_idx, dev);
    q.t_idx = t_idx->data_ptr();
    q.e_idx = e_idx->data_ptr();
    q.idx64 = t_idx->scalar_type() == at::kLong ? 1 : 0;
    want(obs, "obs", obs.scalar_type(), dev, {q.N, L, h, w});
  } else if (source == CAMPX_WINDOWS_TRACE) {
    q.N = q.T * B;
    want(obs, "obs", obs.scalar_type(), dev, {q.T, B, L, h, w});
  } else {
    TORCH_CHECK(obs.dim() == 4 && obs.size(0) >= 1, what, ": obs must be [N, L, h, w]");
    q.N = obs.size(0);
    want(obs, "obs", obs.scalar_type(), dev, {q.N, L, h, w});
    if (t_idx.has_value()) {
      TORCH_CHECK(t_idx->scalar_type() == at::kLong || t_idx->scalar_type() == at::kInt,
                  what, ": state ids must be int64 or int32");
      want(*t_idx, "state_ids", t_idx->scalar_type(), dev, {q.N});
      q.state_ids = t_idx->data_ptr();
      q.idx64 = t_idx->scalar_type() == at::kLong ? 1 : 0;
    }
  }
  if (bad_count.has_value()) want(*bad_count, "bad_count", at::kInt, dev, {1});
  q.h = (int32_t)h;
  q.w = (int32_t)w;
  q.anchor = thing >= 0 ? CAMPX_WINDOW_ON_THING : CAMPX_WINDOW_FIXED;
  q.thing = (int32_t)(thing >= 0 ? thing : 0);
  TORCH_CHECK(thing < hs->n_dyn, what, ": thing ", thing, " of ", hs->n_dyn);
  TORCH_CHECK(thing >= 0 || (r0 >= -255 && r0 <= 255 && c0 >= -255 && c0 <= 255), what,
              ": a fixed window's corner must be within -255 .. 255");
  q.r0 = (int32_t)r0;
  q.c0 = (int32_t)c0;
  TORCH_CHECK(pad_layer >= -1 && pad_layer < L, what, ": pad layer ", pad_layer, " of ", L);
  q.pad_layer = (int32_t)pad_layer;
  q.obs_format = obs_format_of(obs);
  q.obs = obs.data_ptr();
  q.bad_count = opt_ptr<int32_t>(bad_count);
  q.bad_flag = flag_ptr(bad_flag, dev);
  q.streaming = streaming ? 1 : 0;
  TORCH_CHECK(q.N <= ((1ll << 32) - 65536 - 1) / (L * h * w), what, ": ", q.N, " rows of ", L * h * w,
              " elements are past what one call addresses (2^32 - 65536 - 1): split the request");
  const DeviceGuard guard(dev);
  check_ok(campx_wide_render_windows_launch(hs, tables.data_ptr(), layer_of_cell.data_ptr(), &q, B,
                                            current_stream()),
           "campx_wide_render_windows_launch");
}

// ---- campx::returns / vtrace / state_sums / table_lookup: the ops over [T, B] streams, every
// stream contiguous within a row, rows any pitch >= B apart, each stream its own.

// The first stream of such an op tells the device and the shape.  `kind`: "a float32", "an int32".
struct StreamShape {
  c10::Device dev;
  int64_t T, B;
};
StreamShape first_stream(const char* op, const Tensor& t, const char* name, const char* kind) {
  TORCH_CHECK(t.device().is_cuda() && t.dim() == 2, op, ": ", name, " must be ", kind,
              " [T, B] tensor on a HIP device (no CPU implementation)");
  const int64_t T = t.size(0), B = t.size(1);
  TORCH_CHECK(T >= 1 && T <= 0x7fffffff && B >= 1, op, ": bad shape [", T, ", ", B, "]");
  return {t.device(), T, B};
}

// One stream into the launch's struct: its pointer and its pitch.
template <typename P>
void stream_rows(const Tensor& t, const char* name, at::ScalarType dtype, const StreamShape& s, P*& p,
                 int64_t& pitch) {
  want_row_stream(t, name, dtype, s.dev, s.T, s.B);
  TORCH_CHECK(s.T == 1 || t.stride(0) >= s.B, "campx: ", name, " has row pitch ", t.stride(0),
              ", below its ", s.B, " columns");
  p = reinterpret_cast<P*>(t.data_ptr());
  pitch = s.T == 1 ? s.B : t.stride(0);
}
template <typename P>
void stream_rows(const OptTensor& t, const char* name, at::ScalarType dtype, const StreamShape& s, P*& p,
                 int64_t& pitch) {
  if (t.has_value()) stream_rows(*t, name, dtype, s, p, pitch);
}

// A device counter: int64, one element.  `what`: "bad_count must be an int64 tensor".
int64_t* counter(const char* op, const char* what, const Tensor& c, const c10::Device& dev) {
  TORCH_CHECK(c.device() == dev && c.scalar_type() == at::kLong && c.numel() == 1, op, ": ", what,
              " of one element on ", dev);
  return reinterpret_cast<int64_t*>(c.data_ptr());
}
int64_t* counter(const char* op, const char* what, const OptTensor& c, const c10::Device& dev) {
  return c.has_value() ? counter(op, what, *c, dev) : nullptr;
}

// float32 [B], or none.
const float* bootstrap_row(const OptTensor& bootstrap, const StreamShape& s) {
  if (bootstrap.has_value()) want(*bootstrap, "bootstrap", at::kFloat, s.dev, {s.B});
  return opt_ptr<const float>(bootstrap);
}

// Discounted returns and GAE advantages of [T, B] streams (campx_returns_launch).
void returns(const Tensor& reward, const Tensor& done, double gamma, const OptTensor& discount,
             const OptTensor& values, const OptTensor& bootstrap, double lam, Tensor& returns_out,
             const OptTensor& advantages) {
  const StreamShape s = first_stream("campx::returns", reward, "reward", "a float32");
  TORCH_CHECK(values.has_value() == advantages.has_value(),
              "campx::returns: values and advantages come together");
  CampxReturns r{};
  stream_rows(reward, "reward", at::kFloat, s, r.reward, r.reward_pitch);
  stream_rows(done, "done", at::kByte, s, r.done, r.done_pitch);
  stream_rows(discount, "discount", at::kFloat, s, r.discount, r.discount_pitch);
  stream_rows(values, "values", at::kFloat, s, r.values, r.values_pitch);
  stream_rows(advantages, "advantages", at::kFloat, s, r.advantages, r.advantages_pitch);
  stream_rows(returns_out, "returns", at::kFloat, s, r.returns, r.returns_pitch);
  r.bootstrap = bootstrap_row(bootstrap, s);
  r.gamma = (float)gamma;
  r.lam = (float)lam;
  const DeviceGuard guard(s.dev);
  check_ok(campx_returns_launch(&r, s.B, (int32_t)s.T, current_stream()), "campx_returns_launch");
}

// V-trace targets and advantages of [T, B] streams (campx_vtrace_launch): `ratio` exactly when the
// table set (target [Nt, A], behaviour [Nb, A], states, actions) is not given.
void vtrace(const Tensor& reward, const Tensor& done, double gamma, const Tensor& values,
            const OptTensor& ratio, const OptTensor& target, const OptTensor& behaviour,
            const OptTensor& states, const OptTensor& actions, const OptTensor& discount,
            const OptTensor& bootstrap, double lam, double rho_bar, double c_bar, double pg_rho_bar,
            const OptTensor& bad_count, int64_t path, Tensor& vs, Tensor& advantages) {
  const StreamShape s = first_stream("campx::vtrace", reward, "reward", "a float32");
  const c10::Device dev = s.dev;
  const bool table = target.has_value();
  TORCH_CHECK(behaviour.has_value() == table && states.has_value() == table &&
                  actions.has_value() == table && ratio.has_value() != table,
              "campx::vtrace: give ratio, or target, behaviour, states and actions together");
  TORCH_CHECK(path >= 0 && path <= 2, "campx::vtrace: bad path ", path);
  CampxVtrace v{};
  stream_rows(reward, "reward", at::kFloat, s, v.reward, v.reward_pitch);
  stream_rows(done, "done", at::kByte, s, v.done, v.done_pitch);
  stream_rows(values, "values", at::kFloat, s, v.values, v.values_pitch);
  stream_rows(discount, "discount", at::kFloat, s, v.discount, v.discount_pitch);
  v.bootstrap = bootstrap_row(bootstrap, s);
  if (table) {
    TORCH_CHECK(target->dim() == 2 && behaviour->dim() == 2 && target->size(0) >= 1 &&
                    target->size(1) >= 1 && target->size(1) <= 128 &&
                    behaviour->size(0) <= 0x7fffffff && behaviour->size(0) % target->size(0) == 0,
                "campx::vtrace: target must be [Nt, A <= 128] and behaviour [Nb, A], Nb a multiple "
                "of Nt; they are ", target->sizes(), " and ", behaviour->sizes());
    want(*target, "target", at::kFloat, dev, {target->size(0), target->size(1)});
    want(*behaviour, "behaviour", at::kFloat, dev, {behaviour->size(0), target->size(1)});
    v.target = opt_ptr<const float>(target);
    v.behaviour = opt_ptr<const float>(behaviour);
    v.n_target_states = target->size(0);
    v.n_behaviour_states = behaviour->size(0);
    v.n_actions = (int32_t)target->size(1);
  }
  stream_rows(states, "states", at::kInt, s, v.states, v.states_pitch);
  stream_rows(actions, "actions", at::kChar, s, v.actions, v.actions_pitch);
  stream_rows(ratio, "ratio", at::kFloat, s, v.ratio, v.ratio_pitch);
  v.bad_count = counter("campx::vtrace", "bad_count must be an int64 tensor", bad_count, dev);
  stream_rows(vs, "vs", at::kFloat, s, v.vs, v.vs_pitch);
  stream_rows(advantages, "advantages", at::kFloat, s, v.advantages, v.advantages_pitch);
  v.path = (int32_t)path;
  v.gamma = (float)gamma;
  v.lam = (float)lam;
  v.rho_bar = (float)rho_bar;
  v.c_bar = (float)c_bar;
  v.pg_rho_bar = (float)pg_rho_bar;
  const DeviceGuard guard(dev);
  check_ok(campx_vtrace_launch(&v, s.B, (int32_t)s.T, current_stream()), "campx_vtrace_launch");
}

// Per-(state, action) fixed-point sums of [T, B] streams (campx_state_sums_launch): `raw` int64
// [1 + K, n_states * n_actions] in any shape that is contiguous, the counters int64 of one element.
void state_sums(const Tensor& states, const OptTensor& actions, at::TensorList values,
                int64_t n_states, int64_t n_actions, int64_t frac_bits, bool accumulate,
                int64_t path, Tensor& raw, Tensor& skipped, Tensor& clamped) {
  const StreamShape sh = first_stream("campx::state_sums", states, "states", "an int32");
  const c10::Device dev = sh.dev;
  const int64_t K = (int64_t)values.size();
  TORCH_CHECK(K <= CAMPX_SUMS_MAX_VALUES, "campx::state_sums: at most ", CAMPX_SUMS_MAX_VALUES,
              " value streams, got ", K);
  TORCH_CHECK(n_states >= 1 && n_states <= 0x7fffffff && n_actions >= 1 && n_actions <= 128 &&
                  frac_bits >= 0 && frac_bits <= 62 && path >= 0 && path <= 2,
              "campx::state_sums: bad n_states / n_actions / frac_bits / path");
  CampxStateSums s{};
  stream_rows(states, "states", at::kInt, sh, s.states, s.states_pitch);
  stream_rows(actions, "actions", at::kChar, sh, s.actions, s.actions_pitch);
  for (int64_t k = 0; k < K; ++k)
    stream_rows(values[k], "values", at::kFloat, sh, s.values[k], s.values_pitch[k]);
  TORCH_CHECK(raw.device() == dev && raw.scalar_type() == at::kLong && raw.is_contiguous() &&
                  raw.numel() == (K + 1) * n_states * n_actions,
              "campx::state_sums: raw must be a contiguous int64 tensor of ", K + 1, " x ", n_states,
              " x ", n_actions, " elements on ", dev);
  s.acc = reinterpret_cast<int64_t*>(raw.data_ptr());
  s.skipped = counter("campx::state_sums", "skipped and clamped must be int64 tensors", skipped, dev);
  s.clamped = counter("campx::state_sums", "skipped and clamped must be int64 tensors", clamped, dev);
  s.n_states = n_states;
  s.n_actions = (int32_t)n_actions;
  s.n_values = (int32_t)K;
  s.frac_bits = (int32_t)frac_bits;
  s.accumulate = accumulate ? 1 : 0;
  s.path = (int32_t)path;
  const DeviceGuard guard(dev);
  check_ok(campx_state_sums_launch(&s, sh.B, (int32_t)sh.T, current_stream()), "campx_state_sums_launch");
}

// out[t, e] = table[states[t, e] * n_actions + actions[t, e]] (campx_table_lookup_launch); `table`
// float32 [n_states] without actions, [n_states, n_actions] with.
void table_lookup(const Tensor& table, const Tensor& states, const OptTensor& actions, Tensor& out,
                  const OptTensor& bad_count) {
  const StreamShape s = first_stream("campx::table_lookup", states, "states", "an int32");
  const c10::Device dev = s.dev;
  TORCH_CHECK(table.device() == dev && table.scalar_type() == at::kFloat && table.is_contiguous() &&
                  table.dim() == (actions.has_value() ? 2 : 1) && table.numel() >= 1,
              "campx::table_lookup: table must be a contiguous float32 [n_states",
              actions.has_value() ? ", n_actions" : "", "] tensor on ", dev);
  const int64_t S = table.size(0), A = actions.has_value() ? table.size(1) : 1;
  TORCH_CHECK(S <= 0x7fffffff && A <= 128, "campx::table_lookup: table too large: ", table.sizes());
  CampxTableLookup l{};
  stream_rows(states, "states", at::kInt, s, l.states, l.states_pitch);
  stream_rows(actions, "actions", at::kChar, s, l.actions, l.actions_pitch);
  stream_rows(out, "out", at::kFloat, s, l.out, l.out_pitch);
  l.bad_count = counter("campx::table_lookup", "bad_count must be an int64 tensor", bad_count, dev);
  l.table = reinterpret_cast<const float*>(table.data_ptr());
  l.n_states = S;
  l.n_actions = (int32_t)A;
  const DeviceGuard guard(dev);
  check_ok(campx_table_lookup_launch(&l, s.B, (int32_t)s.T, current_stream()),
           "campx_table_lookup_launch");
}

// The sweeps ops.  `what` names the op in its messages; `members`: `policy` is a population's
// [P, n_states, 5] and every per-member shape has that leading P; `solve`: the population's
// policies may be missing (the greedy reduction, P from `values_out`) and `rewards` given.
void sweeps(const char* what, bool members, bool solve, const Tensor& spec_host, const Tensor& tables,
            const OptTensor& policy, const OptTensor& rewards, const OptTensor& reward, double gamma,
            const OptTensor& gammas, const Tensor& values_in, Tensor& values_out, const OptTensor& scratch,
            const OptTensor& q, const OptTensor& greedy, Tensor& residual,
            const OptTensor& bad_rows, const OptTensor& bad_flag, int64_t path) {
  const CampxWideSpec* hs = wide_spec(spec_host);
  TORCH_CHECK(values_out.device().is_cuda(), what,
              ": values_out must be on a HIP device (no CPU implementation)");
  const c10::Device dev = values_out.device();
  const int64_t S = hs->n_states, A = CAMPX_N_ACTIONS;
  want_wide_tables(tables, hs, dev);
  TORCH_CHECK(!members || solve || (policy->dim() == 3 && policy->size(0) >= 1), what,
              ": policies must be float32 [P, n_states, 5], P >= 1");
  TORCH_CHECK(!solve || (values_out.dim() == 2 && values_out.size(0) >= 1), what,
              ": values_out must be float32 [P, n_states], P >= 1");
  TORCH_CHECK(!rewards.has_value() || !reward.has_value(), what,
              ": give rewards (one table per member) or reward (one for all), not both");
  TORCH_CHECK(!solve || !policy.has_value() || !greedy.has_value(), what,
              ": greedy is written by the greedy reduction only (policies None)");
  const int64_t P = solve ? values_out.size(0) : members ? policy->size(0) : 1;
  const auto each = [&](std::initializer_list<int64_t> shape) {      // ... of every member
    std::vector<int64_t> all(members ? 1 : 0, P);
    all.insert(all.end(), shape);
    return all;
  };
  if (policy.has_value()) want(*policy, members ? "policies" : "policy", at::kFloat, dev, each({S, A}));
  if (reward.has_value()) want(*reward, "reward", at::kFloat, dev, {S, A});
  if (rewards.has_value()) want(*rewards, "rewards", at::kFloat, dev, each({S, A}));
  if (gammas.has_value()) want(*gammas, "gammas", at::kFloat, dev, {P});
  want(values_in, "values_in", at::kFloat, dev, each({S}));
  want(values_out, "values_out", at::kFloat, dev, each({S}));
  if (scratch.has_value()) want(*scratch, "scratch", at::kFloat, dev, each({S}));
  if (q.has_value()) want(*q, "q", at::kFloat, dev, each({S, A}));
  if (greedy.has_value()) want(*greedy, "greedy", at::kChar, dev, each({S}));
  if (members) {
    TORCH_CHECK(residual.dim() == 2 && residual.size(0) >= 1 && residual.size(0) <= (1 << 20), what,
                ": residual must be float32 [sweeps, P], 1 <= sweeps <= 2^20");
    want(residual, "residual", at::kFloat, dev, {residual.size(0), P});
  } else {
    TORCH_CHECK(residual.device() == dev && residual.scalar_type() == at::kFloat && residual.dim() == 1 &&
                    residual.is_contiguous() && residual.numel() >= 1 && residual.numel() <= (1 << 20),
                what, ": residual must be a contiguous float32 [sweeps] tensor on ", dev,
                ", 1 <= sweeps <= 2^20");
  }
  if (bad_rows.has_value()) want(*bad_rows, "bad_rows", at::kInt, dev, {1});
  TORCH_CHECK(path >= 0 && path <= 2, what, ": path must be 0, 1 or 2");
  const DeviceGuard guard(dev);
  const float* v_in = reinterpret_cast<const float*>(values_in.data_ptr());
  float* v_out = reinterpret_cast<float*>(values_out.data_ptr());
  float* res = reinterpret_cast<float*>(residual.data_ptr());
  const int32_t n_sweeps = (int32_t)residual.size(0);
  if (solve)
    check_ok(campx_wide_population_solve_launch(
                 hs, tables.data_ptr(), opt_ptr<const float>(policy), opt_ptr<const float>(rewards), P,
                 opt_ptr<const float>(reward), (float)gamma, opt_ptr<const float>(gammas), v_in, v_out,
                 opt_ptr<float>(scratch), opt_ptr<float>(q), opt_ptr<int8_t>(greedy), res,
                 opt_ptr<int32_t>(bad_rows), flag_ptr(bad_flag, dev), n_sweeps, (int32_t)path,
                 current_stream()),
             "campx_wide_population_solve_launch");
  else if (members)
    check_ok(campx_wide_population_sweeps_launch(
                 hs, tables.data_ptr(), opt_ptr<const float>(policy), P, opt_ptr<const float>(reward),
                 (float)gamma, opt_ptr<const float>(gammas), v_in, v_out, opt_ptr<float>(scratch),
                 opt_ptr<float>(q), res, opt_ptr<int32_t>(bad_rows), flag_ptr(bad_flag, dev), n_sweeps,
                 (int32_t)path, current_stream()),
             "campx_wide_population_sweeps_launch");
  else
    check_ok(campx_wide_sweeps_launch(
                 hs, tables.data_ptr(), opt_ptr<const float>(policy), opt_ptr<const float>(reward),
                 (float)gamma, v_in, v_out, opt_ptr<float>(scratch), opt_ptr<float>(q),
                 opt_ptr<int8_t>(greedy), res, opt_ptr<int32_t>(bad_rows), flag_ptr(bad_flag, dev),
                 n_sweeps, (int32_t)path, current_stream()),
             "campx_wide_sweeps_launch");
}

// Sweeps of the Bellman backup over the state table (campx_wide_sweeps_launch): `policy` float32
// [n_states, 5] for the value of a policy, None for value iteration; as many sweeps as `residual`
// has elements.  `values_in` may be `values_out`.
void wide_sweeps(const Tensor& spec_host, const Tensor& tables, const OptTensor& policy,
                 const OptTensor& reward, double gamma, const Tensor& values_in, Tensor& values_out,
                 const OptTensor& scratch, const OptTensor& q, const OptTensor& greedy,
                 Tensor& residual, const OptTensor& bad_rows, const OptTensor& bad_flag,
                 int64_t path) {
  sweeps("campx::wide_sweeps", false, false, spec_host, tables, policy, std::nullopt, reward, gamma,
         std::nullopt, values_in, values_out, scratch, q, greedy, residual, bad_rows, bad_flag, path);
}

// The policy-evaluation sweeps for a population (campx_wide_population_sweeps_launch): `policies`
// float32 [P, n_states, 5], `residual` float32 [sweeps, P], `gammas` float32 [P] or None for the
// scalar `gamma`.  `values_in` may be `values_out`.
void wide_population_sweeps(const Tensor& spec_host, const Tensor& tables, const Tensor& policies,
                            const OptTensor& reward, double gamma, const OptTensor& gammas,
                            const Tensor& values_in, Tensor& values_out, const OptTensor& scratch,
                            const OptTensor& q, Tensor& residual, const OptTensor& bad_rows,
                            const OptTensor& bad_flag, int64_t path) {
  sweeps("campx::wide_population_sweeps", true, false, spec_host, tables, policies, std::nullopt, reward,
         gamma, gammas, values_in, values_out, scratch, q, std::nullopt, residual, bad_rows, bad_flag,
         path);
}

// Either reduction for a population (campx_wide_population_solve_launch): `policies` float32
// [P, n_states, 5] or None for value iteration, `rewards` float32 [P, n_states, 5] - a reward table
// per member - or None, `reward` the one table for all or None (not beside `rewards`), `greedy` int8
// [P, n_states] or None (not beside `policies`); the rest as campx::wide_population_sweeps.
void wide_population_solve(const Tensor& spec_host, const Tensor& tables, const OptTensor& policies,
                           const OptTensor& rewards, const OptTensor& reward, double gamma,
                           const OptTensor& gammas, const Tensor& values_in, Tensor& values_out,
                           const OptTensor& scratch, const OptTensor& q, const OptTensor& greedy,
                           Tensor& residual, const OptTensor& bad_rows, const OptTensor& bad_flag,
                           int64_t path) {
  sweeps("campx::wide_population_solve", true, true, spec_host, tables, policies, rewards, reward, gamma,
         gammas, values_in, values_out, scratch, q, greedy, residual, bad_rows, bad_flag, path);
}

// Both visitation ops.  `what` names the op in its messages; `members`: `policy` is a population's
// [P, n_states, 5], every per-member shape has that leading P, and `start` may also be one
// [n_states] shared by all.
void visit(const char* what, bool members, const Tensor& spec_host, const Tensor& tables,
           const Tensor& policy, const OptTensor& start, bool restart, Tensor& visits,
           Tensor& finished, Tensor& final_mass, const OptTensor& per_frame, Tensor& counts,
           const OptTensor& scratch, const OptTensor& bad_rows, const OptTensor& bad_flag,
           int64_t path) {
  const CampxWideSpec* hs = wide_spec(spec_host);
  TORCH_CHECK(visits.device().is_cuda(), what, ": visits must be on a HIP device (no CPU implementation)");
  const c10::Device dev = visits.device();
  const int64_t S = hs->n_states, A = CAMPX_N_ACTIONS;
  want_wide_tables(tables, hs, dev);
  TORCH_CHECK(!members || (policy.dim() == 3 && policy.size(0) >= 1), what,
              ": policies must be float32 [P, n_states, 5], P >= 1");
  const int64_t P = members ? policy.size(0) : 1;
  const auto each = [&](std::initializer_list<int64_t> shape) {      // ... of every member
    std::vector<int64_t> all(members ? 1 : 0, P);
    all.insert(all.end(), shape);
    return all;
  };
  want(policy, members ? "policies" : "policy", at::kFloat, dev, each({S, A}));
  const bool per_member = !members || (start.has_value() && start->dim() == 2);
  if (start.has_value()) {
    if (per_member) want(*start, "start", at::kLong, dev, each({S}));
    else want(*start, "start", at::kLong, dev, {S});
  }
  want(visits, "visits", at::kLong, dev, each({S, A}));
  if (members) {
    TORCH_CHECK(finished.dim() == 2 && finished.size(0) >= 1 && finished.size(0) <= (1 << 20), what,
                ": finished must be int64 [frames, P], 1 <= frames <= 2^20");
    want(finished, "finished", at::kLong, dev, {finished.size(0), P});
  } else {
    TORCH_CHECK(finished.device() == dev && finished.scalar_type() == at::kLong && finished.dim() == 1 &&
                    finished.is_contiguous() && finished.numel() >= 1 && finished.numel() <= (1 << 20),
                what, ": finished must be a contiguous int64 [frames] tensor on ", dev,
                ", 1 <= frames <= 2^20");
  }
  const int64_t T = finished.size(0);
  want(final_mass, "final_mass", at::kLong, dev, each({S}));
  if (per_frame.has_value()) {
    std::vector<int64_t> frames = each({S});
    frames.insert(frames.begin(), T + 1);
    want(*per_frame, "per_frame", at::kLong, dev, frames);
  }
  want(counts, "counts", at::kInt, dev, each({S, A}));
  if (scratch.has_value()) want(*scratch, "scratch", at::kLong, dev, each({S}));
  if (bad_rows.has_value()) want(*bad_rows, "bad_rows", at::kInt, dev, {1});
  TORCH_CHECK(path >= 0 && path <= 2, what, ": path must be 0, 1 or 2");
  const DeviceGuard guard(dev);
  const float* w = reinterpret_cast<const float*>(policy.data_ptr());
  int64_t* d_visits = reinterpret_cast<int64_t*>(visits.data_ptr());
  int64_t* d_finished = reinterpret_cast<int64_t*>(finished.data_ptr());
  int64_t* d_final = reinterpret_cast<int64_t*>(final_mass.data_ptr());
  int32_t* d_counts = reinterpret_cast<int32_t*>(counts.data_ptr());
  if (members)
    check_ok(campx_wide_visit_population_launch(
                 hs, tables.data_ptr(), w, P, opt_ptr<const int64_t>(start), per_member ? 1 : 0,
                 restart ? 1 : 0, (int32_t)T, d_visits, d_finished, d_final, opt_ptr<int64_t>(per_frame),
                 d_counts, opt_ptr<int64_t>(scratch), opt_ptr<int32_t>(bad_rows),
                 flag_ptr(bad_flag, dev), (int32_t)path, current_stream()),
             "campx_wide_visit_population_launch");
  else
    check_ok(campx_wide_visit_launch(
                 hs, tables.data_ptr(), w, opt_ptr<const int64_t>(start), restart ? 1 : 0, (int32_t)T,
                 d_visits, d_finished, d_final, opt_ptr<int64_t>(per_frame), d_counts,
                 opt_ptr<int64_t>(scratch), opt_ptr<int32_t>(bad_rows), flag_ptr(bad_flag, dev),
                 (int32_t)path, current_stream()),
             "campx_wide_visit_launch");
}

// Exact state visitation of a policy over the state table (campx_wide_visit_launch): as many
// frames as `finished` has elements, from `start` (int64 [n_states] units of 2^-38; None: one
// environment in state 0), which may be `final_mass`.
void wide_visit(const Tensor& spec_host, const Tensor& tables, const Tensor& policy,
                const OptTensor& start, bool restart, Tensor& visits, Tensor& finished,
                Tensor& final_mass, const OptTensor& per_frame, Tensor& counts,
                const OptTensor& scratch, const OptTensor& bad_rows, const OptTensor& bad_flag,
                int64_t path) {
  visit("campx::wide_visit", false, spec_host, tables, policy, start, restart, visits, finished,
        final_mass, per_frame, counts, scratch, bad_rows, bad_flag, path);
}

// Exact state visitation of a population of policies (campx_wide_visit_population_launch):
// `policies` float32 [P, n_states, 5], as many frames as `finished` [frames, P] has rows, from
// `start` - int64 [P, n_states] per member, which may be `final_mass`, or [n_states] shared by
// all; None: one environment in state 0 for every member.
void wide_visit_population(const Tensor& spec_host, const Tensor& tables, const Tensor& policies,
                           const OptTensor& start, bool restart, Tensor& visits, Tensor& finished,
                           Tensor& final_mass, const OptTensor& per_frame, Tensor& counts,
                           const OptTensor& scratch, const OptTensor& bad_rows,
                           const OptTensor& bad_flag, int64_t path) {
  visit("campx::wide_visit_population", true, spec_host, tables, policies, start, restart, visits,
        finished, final_mass, per_frame, counts, scratch, bad_rows, bad_flag, path);
}

void onehot_to_ids(const Tensor& onehot, Tensor& ids_out, Tensor& bad_count) {
  TORCH_CHECK(onehot.device().is_cuda(), "campx::onehot_to_ids: HIP tensors only");
  const c10::Device dev = onehot.device();
  const int64_t n = ids_out.numel();
  TORCH_CHECK(onehot.scalar_type() == at::kFloat && onehot.is_contiguous() &&
                  onehot.numel() == n * CAMPX_N_ACTIONS,
              "campx::onehot_to_ids: onehot must be contiguous float32 [..., 5]");
  TORCH_CHECK(ids_out.device() == dev && ids_out.scalar_type() == at::kChar && ids_out.is_contiguous(),
              "campx::onehot_to_ids: ids must be contiguous int8 on ", dev);
  want(bad_count, "bad_count", at::kInt, dev, {1});
  const DeviceGuard guard(dev);
  check_ok(campx_onehot_to_ids_launch(reinterpret_cast<const float*>(onehot.data_ptr()),
                                      reinterpret_cast<int8_t*>(ids_out.data_ptr()), n,
                                      reinterpret_cast<int32_t*>(bad_count.data_ptr()),
                                      current_stream()),
           "campx_onehot_to_ids_launch");
}

void check_actions(const Tensor& actions, Tensor& bad_count) {
  TORCH_CHECK(actions.device().is_cuda(), "campx::check_actions: HIP tensors only");
  const c10::Device dev = actions.device();
  TORCH_CHECK(actions.scalar_type() == at::kChar && actions.is_contiguous(),
              "campx::check_actions: actions must be contiguous int8");
  want(bad_count, "bad_count", at::kInt, dev, {1});
  const DeviceGuard guard(dev);
  check_ok(campx_check_actions_launch(ids(actions), actions.numel(),
                                      reinterpret_cast<int32_t*>(bad_count.data_ptr()),
                                      current_stream()),
           "campx_check_actions_launch");
}

// Meta / fake-tensor implementation of every op: the ops return nothing and write in place, so
// there is nothing to infer - the arguments are dropped from the stack.
void nothing_to_infer(const c10::OperatorHandle& op, torch::jit::Stack* stack) {
  torch::jit::drop(*stack, op.schema().arguments().size());
}

// ADInplaceOrView: run the op, then mark every argument the schema declares written
// (`Tensor(a!)`) as modified in place.
void run_then_bump_versions(const c10::OperatorHandle& op, c10::DispatchKeySet keys,
                            torch::jit::Stack* stack) {
  const auto& arguments = op.schema().arguments();
  const size_t n = arguments.size();
  at::Tensor written[16];
  size_t n_written = 0;
  for (size_t i = 0; i < n; ++i) {
    const c10::AliasInfo* alias = arguments[i].alias_info();
    if (!alias || !alias->isWrite()) continue;
    const c10::IValue& v = torch::jit::peek(*stack, i, n);
    if (v.isTensor() && v.toTensor().defined() && n_written < 16) written[n_written++] = v.toTensor();
  }
  {
    c10::impl::ExcludeDispatchKeyGuard below(c10::autograd_dispatch_keyset_with_ADInplaceOrView);
    op.redispatchBoxed(keys & c10::after_ADInplaceOrView_keyset, stack);
  }
  for (size_t i = 0; i < n_written; ++i)
    if (!written[i].is_inference()) written[i].unsafeGetTensorImpl()->bump_version();
}

// Every op, for the two boxed kernels (campx_amd/_hip.py OP_NAMES is the Python side's list).
const char* const kOps[] = {
    "reset", "step", "rollout", "update", "render", "rollout_pipelined", "update_render",
    "shape_rollout", "wide_rollout", "wide_update", "wide_policy_update", "wide_policy_population",
    "wide_learn", "wide_learn_shared", "wide_learn_traces", "wide_learn_dyna", "wide_learn_actor",
    "wide_learn_actor_shared", "render_gather",
    "wide_render_gather", "wide_render_states", "wide_render_windows", "returns", "vtrace", "state_sums",
    "table_lookup", "wide_sweeps", "wide_population_sweeps", "wide_population_solve", "wide_visit",
    "wide_visit_population",
    "onehot_to_ids",
    "check_actions"};

}  // namespace

TORCH_LIBRARY(campx, m) {
  m.def(
      "reset(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, Tensor(c!)? ret, "
      "Tensor? pair_table, Tensor(d!) obs, Tensor(e!)? board) -> ()");
  m.def(
      "step(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, Tensor(c!)? ret, "
      "Tensor? pair_table, Tensor actions, Tensor(d!) obs, Tensor(e!)? board, Tensor(f!)? reward, "
      "Tensor(g!)? discount, Tensor(h!)? step_done, Tensor(i!)? perf, Tensor(j!)? bad_count, "
      "Tensor(k!)? bad_flag) -> ()");
  m.def(
      "rollout(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, Tensor(c!)? ret, "
      "Tensor? pair_table, Tensor actions, Tensor(d!) obs, Tensor(e!)? board, Tensor(f!)? reward, "
      "Tensor(g!)? discount, Tensor(h!)? step_done, Tensor(i!)? perf, Tensor(j!)? trace, "
      "Tensor(k!)? bad_count, Tensor(l!)? bad_flag, bool reset_first, Tensor(m!)? scratch=None, "
      "Tensor(n!)? scratch_state=None, Tensor(o!)? error_flag=None) -> ()");
  m.def(
      "update(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, Tensor(c!)? ret, "
      "Tensor? pair_table, Tensor actions, Tensor(d!)? reward, Tensor(e!)? discount, "
      "Tensor(f!)? step_done, Tensor(g!)? perf, Tensor(h!) trace, Tensor(i!)? bad_count, "
      "Tensor(j!)? bad_flag, bool reset_first) -> ()");
  m.def(
      "render(Tensor spec_host, Tensor spec_dev, Tensor trace, Tensor(a!) obs, Tensor(b!)? board) "
      "-> ()");
  m.def(
      "rollout_pipelined(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor? pair_table, Tensor actions, Tensor(d!) obs, Tensor(e!)? board, "
      "Tensor(f!)? reward, Tensor(g!)? discount, Tensor(h!)? step_done, Tensor(i!)? perf, "
      "Tensor(j!) trace, Tensor(k!)? bad_count, Tensor(l!)? bad_flag, bool reset_first, bool resync) -> ()");
  m.def(
      "update_render(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor? pair_table, Tensor actions, Tensor(d!)? reward, Tensor(e!)? discount, "
      "Tensor(f!)? step_done, Tensor(g!)? perf, Tensor(h!) trace, Tensor(i!)? bad_count, "
      "Tensor(j!)? bad_flag, bool reset_first, Tensor prev_trace, Tensor(k!) prev_obs) -> ()");
  m.def(
      "shape_rollout(Tensor spec_host, Tensor spec_dev, Tensor(a!) pos, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!)? backdrop_state, Tensor? actions, Tensor(e!) obs, "
      "Tensor(f!)? board, Tensor(g!)? reward, Tensor(h!)? discount, Tensor(i!)? step_done, "
      "Tensor(j!)? bad_count, Tensor(k!)? bad_flag, bool reset_first, bool emit_first, "
      "Tensor(l!)? trace=None, Tensor? tables=None) -> ()");
  m.def(
      "wide_rollout(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor? actions, Tensor(d!) obs, Tensor(e!)? board, Tensor(f!)? reward, "
      "Tensor(g!)? discount, Tensor(h!)? step_done, Tensor(i!)? perf, Tensor(j!) trace, "
      "Tensor(k!)? bad_count, Tensor(l!)? bad_flag, bool reset_first) -> ()");
  m.def(
      "wide_update(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor actions, Tensor(d!)? reward, Tensor(e!)? discount, "
      "Tensor(f!)? step_done, Tensor(g!)? perf, Tensor(h!) trace, Tensor(i!)? bad_count, "
      "Tensor(j!)? bad_flag, bool reset_first) -> ()");
  m.def(
      "wide_policy_update(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor policy, int seed, int first_frame, Tensor(d!)? reward, "
      "Tensor(e!)? discount, Tensor(f!)? step_done, Tensor(g!)? perf, Tensor(h!) trace, "
      "Tensor(i!) actions_out, Tensor(j!)? states_out, Tensor(k!)? bad_count, Tensor(l!)? bad_flag, "
      "bool reset_first) -> ()");
  m.def(
      "wide_policy_population(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor policy, int seed, int first_frame, Tensor(d!)? reward, "
      "Tensor(e!)? discount, Tensor(f!)? step_done, Tensor(g!)? perf, Tensor(h!) trace, "
      "Tensor(i!) actions_out, Tensor(j!)? states_out, Tensor(k!)? bad_count, Tensor(l!)? bad_flag, "
      "bool reset_first, int path=0) -> ()");
  m.def(
      "wide_learn(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!) q, Tensor alpha, Tensor gamma, Tensor epsilon, int rule, int seed, "
      "int first_frame, int frames, int window, Tensor(e!) reward_sum, Tensor(f!)? perf_sum, "
      "Tensor(g!) episodes, Tensor(h!)? bad_count, Tensor(i!)? bad_flag, bool reset_first, "
      "int path=0) -> ()");
  m.def(
      "wide_learn_shared(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!) q, Tensor alpha, Tensor gamma, Tensor epsilon, int rule, int seed, "
      "int first_frame, int frames, int window, Tensor(e!) reward_sum, Tensor(f!)? perf_sum, "
      "Tensor(g!) episodes, Tensor(h!) clamped, Tensor(i!)? scratch, Tensor(j!)? bad_count, "
      "Tensor(k!)? bad_flag, bool reset_first, int path=0) -> ()");
  m.def(
      "wide_learn_traces(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!) q, Tensor(e!) traces, Tensor alpha, Tensor gamma, Tensor epsilon, "
      "Tensor lam, int rule, int trace, int seed, int first_frame, int frames, int window, "
      "Tensor(f!) reward_sum, Tensor(g!)? perf_sum, Tensor(h!) episodes, Tensor(i!)? bad_count, "
      "Tensor(j!)? bad_flag, bool reset_first, int path=0, int team=0) -> ()");
  m.def(
      "wide_learn_dyna(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!) q, Tensor(e!) seen, Tensor(f!) n_seen, Tensor planning, "
      "Tensor alpha, Tensor gamma, Tensor epsilon, int rule, int seed, int first_frame, int frames, "
      "int window, Tensor(g!) reward_sum, Tensor(h!)? perf_sum, Tensor(i!) episodes, "
      "Tensor(j!)? marks, Tensor(k!)? bad_count, Tensor(l!)? bad_flag, bool reset_first, "
      "int path=0) -> ()");
  m.def(
      "wide_learn_actor(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!) prefs, Tensor(e!) values, Tensor alpha_actor, Tensor alpha_critic, "
      "Tensor gamma, int seed, int first_frame, int frames, int window, Tensor(f!) reward_sum, "
      "Tensor(g!)? perf_sum, Tensor(h!) episodes, Tensor(i!)? bad_count, Tensor(j!)? bad_rows, "
      "Tensor(k!)? bad_flag, bool reset_first, int path=0) -> ()");
  m.def(
      "wide_learn_actor_shared(Tensor spec_host, Tensor tables, Tensor(a!) state, Tensor(b!) done, "
      "Tensor(c!)? ret, Tensor(d!) prefs, Tensor(e!) values, Tensor alpha_actor, Tensor alpha_critic, "
      "Tensor gamma, int seed, int first_frame, int frames, int window, Tensor(f!) reward_sum, "
      "Tensor(g!)? perf_sum, Tensor(h!) episodes, Tensor(i!) clamped, Tensor(j!)? scratch, "
      "Tensor(k!)? bad_count, Tensor(l!)? bad_rows, Tensor(m!)? bad_flag, bool reset_first, "
      "int path=0) -> ()");
  m.def(
      "render_gather(Tensor spec_host, Tensor spec_dev, Tensor trace, Tensor t_idx, Tensor e_idx, "
      "Tensor(a!) obs, Tensor(b!)? bad_count, Tensor(c!)? bad_flag, bool streaming=False) -> ()");
  m.def(
      "wide_render_gather(Tensor spec_host, Tensor tables, Tensor trace, Tensor t_idx, Tensor e_idx, "
      "Tensor(a!) obs, Tensor(b!)? bad_count, Tensor(c!)? bad_flag, bool streaming=False) -> ()");
  m.def(
      "wide_render_states(Tensor spec_host, Tensor tables, Tensor? state_ids, Tensor(a!) obs, "
      "Tensor(b!)? scratch, Tensor(c!)? bad_count, Tensor(d!)? bad_flag) -> ()");
  m.def(
      "wide_render_windows(Tensor spec_host, Tensor tables, Tensor layer_of_cell, int source, "
      "Tensor? trace, Tensor? t_idx, Tensor? e_idx, Tensor(a!) obs, int h, int w, int thing, int r0, "
      "int c0, int pad_layer, Tensor(b!)? bad_count, Tensor(c!)? bad_flag, bool streaming=False) -> ()");
  m.def(
      "returns(Tensor reward, Tensor done, float gamma, Tensor? discount, Tensor? values, "
      "Tensor? bootstrap, float lam, Tensor(a!) returns, Tensor(b!)? advantages) -> ()");
  m.def(
      "vtrace(Tensor reward, Tensor done, float gamma, Tensor values, Tensor? ratio, Tensor? target, "
      "Tensor? behaviour, Tensor? states, Tensor? actions, Tensor? discount, Tensor? bootstrap, "
      "float lam, float rho_bar, float c_bar, float pg_rho_bar, Tensor(a!)? bad_count, int path, "
      "Tensor(b!) vs, Tensor(c!) advantages) -> ()");
  m.def(
      "state_sums(Tensor states, Tensor? actions, Tensor[] values, int n_states, int n_actions, "
      "int frac_bits, bool accumulate, int path, Tensor(a!) raw, Tensor(b!) skipped, "
      "Tensor(c!) clamped) -> ()");
  m.def(
      "table_lookup(Tensor table, Tensor states, Tensor? actions, Tensor(a!) out, "
      "Tensor(b!)? bad_count) -> ()");
  m.def(
      "wide_sweeps(Tensor spec_host, Tensor tables, Tensor? policy, Tensor? reward, float gamma, "
      "Tensor values_in, Tensor(a!) values_out, Tensor(b!)? scratch, Tensor(c!)? q, "
      "Tensor(d!)? greedy, Tensor(e!) residual, Tensor(f!)? bad_rows, Tensor(g!)? bad_flag, "
      "int path) -> ()");
  m.def(
      "wide_population_sweeps(Tensor spec_host, Tensor tables, Tensor policies, Tensor? reward, "
      "float gamma, Tensor? gammas, Tensor values_in, Tensor(a!) values_out, Tensor(b!)? scratch, "
      "Tensor(c!)? q, Tensor(d!) residual, Tensor(e!)? bad_rows, Tensor(f!)? bad_flag, "
      "int path) -> ()");
  m.def(
      "wide_population_solve(Tensor spec_host, Tensor tables, Tensor? policies, Tensor? rewards, "
      "Tensor? reward, float gamma, Tensor? gammas, Tensor values_in, Tensor(a!) values_out, "
      "Tensor(b!)? scratch, Tensor(c!)? q, Tensor(d!)? greedy, Tensor(e!) residual, "
      "Tensor(f!)? bad_rows, Tensor(g!)? bad_flag, int path) -> ()");
  m.def(
      "wide_visit(Tensor spec_host, Tensor tables, Tensor policy, Tensor? start, bool restart, "
      "Tensor(a!) visits, Tensor(b!) finished, Tensor(c!) final_mass, Tensor(d!)? per_frame, "
      "Tensor(e!) counts, Tensor(f!)? scratch, Tensor(g!)? bad_rows, Tensor(h!)? bad_flag, "
      "int path) -> ()");
  m.def(
      "wide_visit_population(Tensor spec_host, Tensor tables, Tensor policies, Tensor? start, "
      "bool restart, Tensor(a!) visits, Tensor(b!) finished, Tensor(c!) final_mass, "
      "Tensor(d!)? per_frame, Tensor(e!) counts, Tensor(f!)? scratch, Tensor(g!)? bad_rows, "
      "Tensor(h!)? bad_flag, int path) -> ()");
  m.def("onehot_to_ids(Tensor onehot, Tensor(a!) ids, Tensor(b!) bad_count) -> ()");
  m.def("check_actions(Tensor actions, Tensor(a!) bad_count) -> ()");
}

TORCH_LIBRARY_IMPL(campx, CUDA, m) {
  m.impl("reset", &reset);
  m.impl("step", &step);
  m.impl("rollout", &rollout);
  m.impl("update", &update);
  m.impl("render", &render);
  m.impl("rollout_pipelined", &rollout_pipelined);
  m.impl("update_render", &update_render);
  m.impl("shape_rollout", &shape_rollout);
  m.impl("wide_rollout", &wide_rollout);
  m.impl("wide_update", &wide_update);
  m.impl("wide_policy_update", &wide_policy_update);
  m.impl("wide_policy_population", &wide_policy_population);
  m.impl("wide_learn", &wide_learn);
  m.impl("wide_learn_shared", &wide_learn_shared);
  m.impl("wide_learn_traces", &wide_learn_traces);
  m.impl("wide_learn_dyna", &wide_learn_dyna);
  m.impl("wide_learn_actor", &wide_learn_actor);
  m.impl("wide_learn_actor_shared", &wide_learn_actor_shared);
  m.impl("render_gather", &render_gather);
  m.impl("wide_render_gather", &wide_render_gather);
  m.impl("wide_render_states", &wide_render_states);
  m.impl("wide_render_windows", &wide_render_windows);
  m.impl("returns", &returns);
  m.impl("vtrace", &vtrace);
  m.impl("state_sums", &state_sums);
  m.impl("table_lookup", &table_lookup);
  m.impl("wide_sweeps", &wide_sweeps);
  m.impl("wide_population_sweeps", &wide_population_sweeps);
  m.impl("wide_population_solve", &wide_population_solve);
  m.impl("wide_visit", &wide_visit);
  m.impl("wide_visit_population", &wide_visit_population);
  m.impl("onehot_to_ids", &onehot_to_ids);
  m.impl("check_actions", &check_actions);
}

TORCH_LIBRARY_IMPL(campx, ADInplaceOrView, m) {
  for (const char* name : kOps)
    m.impl(name, torch::CppFunction::makeFromBoxedFunction<&run_then_bump_versions>());
}

TORCH_LIBRARY_IMPL(campx, Meta, m) {
  for (const char* name : kOps)
    m.impl(name, torch::CppFunction::makeFromBoxedFunction<&nothing_to_infer>());
}
