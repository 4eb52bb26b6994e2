"""The wide tier: games run from their STATE table, B environments per launch.

The one-cell tier's kernels index their tables by the things' cells - (rows*cols)^K * 5
entries, 7-bit cells - which stops at 128 cells and grows fast with K.  `tabulate.trace()`
enumerates the states a game can actually reach (by running its own `update()` classes,
rule classes included), and the table over THOSE - one row per state, (state, action) ->
state - has no such limits: PyColab-sized boards (16x16 mazes and up; campx/engine.py:31
sets none), up to eight things that show, and whatever hidden values stand behind them (the
z-order in force, keys picked up, doors opened).  The observation stream is the same render
kernel, fed by a 16-bit trace (csrc/k_wide.hip, include/campx_hip.h CampxWideSpec).
`WideGame` is what a batched `Engine` delegates to for games the one-cell tier cannot take;
same surface as `fused.FusedGame` (showtime / reset / play / rollout / rollout_buffers /
check_actions, `done`, `ret`, `perf`; the dynamic state is `state`, int32 [B] state indices),
through the torch op `campx::wide_rollout`.  No CPU path: constructing one without a HIP
device raises.
"""

import ctypes
import math

import torch

from . import _hip
from . import fused
from . import gamespec
from . import tabulate


# What this tier alone offers; the other batched tiers answer each of these with a
# NotImplementedError that names it (refuse_state_table_only()), and Engine forwards each.
STATE_TABLE_ONLY = (
    'rollout_policy_buffers', 'rollout_policy', 'rollout_population_buffers', 'rollout_population',
    'learner_buffers', 'learn_tabular', 'shared_learner_buffers', 'learn_shared', 'learn_traces', 'dyna_buffers', 'learn_dyna', 'learn_actor_critic', 'shared_actor_buffers', 'learn_actor_critic_shared', 'table_arrays', 'sweep_buffers', 'evaluate_policy',
    'value_iteration', 'population_sweep_buffers', 'evaluate_population', 'value_iteration_population',
    'visitation_buffers',
    'state_visitation', 'visit_population_buffers', 'visit_population', 'render_states', 'render_frame_windows', 'render_trace_windows', 'render_state_windows')


def refuse_state_table_only(tier, answers=None):
  """Give the class of another batched tier a method for every name of STATE_TABLE_ONLY that raises
  the tier's NotImplementedError with the name in it, whatever it is called with: through the tier's
  `_no_policy_rollouts(name)`, or the method `answers` names for it."""
  def refusal(name, answer):
    def refuse(self, *args, **kwargs):
      getattr(self, answer)(name)
    refuse.__name__ = name
    refuse.__qualname__ = '{}.{}'.format(tier.__name__, name)
    refuse.__doc__ = '`wide.WideGame.{}`: the state-table tier only; raises NotImplementedError.'.format(name)
    refuse.state_table_only = True
    return refuse
  for name in STATE_TABLE_ONLY:
    setattr(tier, name, refusal(name, (answers or {}).get(name, '_no_policy_rollouts')))


refuse_state_table_only(fused.FusedGame)       # (before WideGame overrides every one of them)


class WideGame(fused.FusedGame):

  def __init__(self, engine, batch, device, traced):
    if not torch.cuda.is_available():
      raise RuntimeError(
          'the wide tier needs a HIP device (torch.cuda.is_available() is False) and has '
          'no CPU fallback; use batch=None for the single-environment generic tier')
    self.device = torch.device('cuda' if device is None else device)
    if self.device.type != 'cuda':
      raise ValueError('wide tier: device must be a HIP/cuda device, got {}'.format(self.device))
    if self.device.index is None:
      self.device = torch.device('cuda', torch.cuda.current_device())
    self.batch = int(batch)
    if self.batch < 1:
      raise ValueError('batch must be >= 1')
    self.traced = traced
    self.description = None
    self.spec, self._arrays = tabulate.to_wide_spec(traced)
    self.chars = list(traced.chars)
    _hip.check(_hip.lib.campx_wide_spec_validate(ctypes.byref(self.spec)),
               'campx_wide_spec_validate')
    self.rows, self.cols = engine.rows, engine.cols
    self.n_layers = len(self.chars)
    self.n_dyn = int(self.spec.n_dyn)      # (pieces of the scenery are not among the things)
    # planes of the trace: the things, plus - a scenery of several variants - which one shows,
    # or - a scenery of pieces that come and go - the mask of those that do
    self._n_planes = self.n_dyn + (1 if self.spec.n_variants > 1 or self.spec.n_pieces > 0 else 0)
    self.uses_table = True
    self.any_reward = bool(self.spec.any_reward)
    self.has_perf = bool(self.spec.has_perf)
    B, dev = self.batch, self.device
    row = self.n_layers * self.rows * self.cols
    if B * row >= (1 << 32) - 65536:
      raise ValueError('wide tier: a frame of {} environments x {} bytes does not fit 32-bit '
                       'offsets; use a smaller batch'.format(B, row))
    n = int(_hip.lib.campx_wide_tables_bytes(ctypes.byref(self.spec)))
    self._tables = torch.empty((n,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
      _hip.check(_hip.lib.campx_wide_tables_build(
          ctypes.byref(self.spec), ctypes.c_void_p(self._tables.data_ptr()),
          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
          'campx_wide_tables_build')
    # The launches read the spec's plain fields only; the blob they get carries no pointers
    # to the host arrays (which stay alive in self._arrays anyway).
    for name in ('state_cells', 'next_state', 'reward', 'done', 'perf', 'variant_top_layer', 'state_variant',
                 'state_pieces'):
      setattr(self.spec, name, None)
    self._spec_host = torch.frombuffer(bytearray(gamespec.spec_bytes(self.spec)),
                                       dtype=torch.uint8)
    self.state = torch.zeros((B,), dtype=torch.int32, device=dev)   # index into traced.st_*
    self.pos = None                   # (positions: see the trace)
    self.done = torch.zeros((B,), dtype=torch.uint8, device=dev)
    self.ret = torch.zeros((B,), dtype=torch.float32, device=dev)
    self._obs = torch.empty((B, self.n_layers, self.rows, self.cols), dtype=torch.int8, device=dev)
    self._board = torch.empty((B, self.rows, self.cols), dtype=torch.int8, device=dev)
    self._reward = torch.empty((B,), dtype=torch.float32, device=dev)
    self._discount = torch.empty((B,), dtype=torch.float32, device=dev)
    self._step_done = torch.empty((B,), dtype=torch.uint8, device=dev)
    self._step_trace = self._trace_rows(None)
    self.perf = torch.zeros((B,), dtype=torch.int8, device=dev)
    self._perf_arg = self.perf if self.has_perf else None
    self._bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._onehot_bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    # environment-frames of rollout_policy() that met a bad policy row (raised with the bad ids)
    self._bad_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    # the same of rollout_population(), counted apart so that the error says where they came from
    self._bad_member_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._policy_frame = 0            # absolute frame the next rollout_policy() / rollout_population() continues at
    # bad rows of the policies given to evaluate_policy() (raised under the same flag)
    self._bad_plan_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    # the same of evaluate_population(), summed over the members
    self._bad_population_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._n_cus = None                # compute units of the device, asked when a plan first needs them
    # bad rows of the policies given to state_visitation() (raised under the same flag)
    self._bad_visit_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    # the same of visit_population(), summed over the members
    self._bad_visit_member_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    # ids of render_states() outside the table (raised with the rows of render_frames(), under
    # their flag), and the one-frame trace of its out= calls: the last block is the largest; the
    # smaller ones before it stay alive, a captured graph may still write into them
    self._bad_state_ids = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._states_scratch = []
    # the same two of the window calls, counted apart so that the error says where they came from
    self._bad_window_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_window_ids = torch.zeros((1,), dtype=torch.int32, device=dev)
    # learners of learn_tabular(), of learn_shared() and of learn_traces() with bad
    # hyper-parameters, once per launch (raised under the flag of the action ids), and the
    # [4, learners] tensors that Python-float hyper-parameters are filled into, by (method, learners)
    self._bad_learners = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_shared_learners = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_trace_learners = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_dyna_learners = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_actor_learners = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_actor_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_shared_actor_learners = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._bad_shared_actor_rows = torch.zeros((1,), dtype=torch.int32, device=dev)
    self._hyper_floats = {}
    self._hyper_ints = {}             # learn_dyna()'s `planning` given as a Python int, by learners
    self._layer_of_cell = None        # the window kernel's scenery table
    self._window_table()
    self._bad_flag = torch.zeros((1,), dtype=torch.int32).pin_memory()
    self._bad_flag_view = self._bad_flag.numpy()
    self.validate_actions = True
    self.frame = -1
    self._observation_cache = self._observation(self._obs, self._board)
    self._wide = _hip.ops.wide_rollout.default
    # (no launch of this tier raises the error word; check_ok() / check_actions() read it all the same)
    self._err_flag = torch.zeros((1,), dtype=torch.int32).pin_memory()
    self._err_flag_view = self._err_flag.numpy()
    self._init_gather()
    # this tier's lazy errors, at their places in the order of the message (fused.FusedGame
    # has the list): bad policy rows ride under the flag of the action ids, ids and rows of the
    # state and window renders under that of render_frames()'s rows
    bad_row = '(a weight that is negative or NaN, or a sum that is not a positive finite number)'
    acts, idx = self._bad_flag_view, self._bad_idx_flag_view
    self._lazy_errors.insert(1, (
        self._bad_rows, acts,
        '{} environment-frames of rollout_policy() met bad policy rows ' + bad_row + '; they took action {}'))
    self._lazy_errors.insert(2, (
        self._bad_member_rows, acts,
        '{} environment-frames of rollout_population() met bad policy rows ' + bad_row +
        '; they took action {}'))
    self._lazy_errors += [
        (self._bad_state_ids, idx,
         '{} state ids of render_states() are outside the game\'s table (they were rendered as state 0)'),
        (self._bad_plan_rows, acts,
         '{} rows of the policy given to evaluate_policy() are bad ' + bad_row +
         '; they were evaluated as taking action {}'),
        (self._bad_population_rows, acts,
         '{} rows of the policies given to evaluate_population() are bad ' + bad_row +
         '; they were evaluated as taking action {}'),
        (self._bad_visit_rows, acts,
         '{} rows of the policy given to state_visitation() are bad ' + bad_row +
         '; all their mass took action {}'),
        (self._bad_visit_member_rows, acts,
         '{} rows of the policies given to visit_population() are bad ' + bad_row +
         '; all their mass took action {}'),
        (self._bad_window_rows, idx,
         '{} rows of render_frame_windows() named a frame or an environment outside the trace (their '
         'windows were rendered from the nearest one inside)'),
        (self._bad_window_ids, idx,
         '{} state ids of render_state_windows() are outside the game\'s table (their windows were '
         'rendered as state 0\'s)'),
        (self._bad_learners, acts,
         '{} learners of learn_tabular() have bad hyper-parameters (alpha, gamma or epsilon not '
         'finite, or epsilon outside [0, 1]); they took action {} at every frame and their tables were '
         'left untouched'),
        (self._bad_shared_learners, acts,
         '{} learners of learn_shared() have bad hyper-parameters (alpha, gamma or epsilon not '
         'finite, or epsilon outside [0, 1]); their environments took action {} at every frame and '
         'their tables were left untouched'),
        (self._bad_trace_learners, acts,
         '{} learners of learn_traces() have bad hyper-parameters (alpha, gamma, epsilon or lam not '
         'finite, or epsilon or lam outside [0, 1]); they took action {} at every frame and their '
         'tables and traces were left untouched'),
        (self._bad_dyna_learners, acts,
         '{} learners of learn_dyna() are bad (alpha, gamma or epsilon not finite, epsilon outside '
         '[0, 1], planning outside 0 .. 1024, or a model whose n_seen or elements are outside the '
         'table); they took action {} at every frame and their tables and models were left untouched'),
        (self._bad_actor_learners, acts,
         '{} learners of learn_actor_critic() have bad hyper-parameters (alpha_actor, alpha_critic or '
         'gamma not finite); they took action {} at every frame and their preferences and values were '
         'left untouched'),
        (self._bad_actor_rows, acts,
         '{} environment-frames of learn_actor_critic() met rows of preferences that are not good (a '
         'NaN or a +inf, or five -inf); they took action {} and changed neither table'),
        (self._bad_shared_actor_learners, acts,
         '{} learners of learn_actor_critic_shared() have bad hyper-parameters (alpha_actor, '
         'alpha_critic or gamma not finite); their environments took action {} at every frame and '
         'their preferences and values were left untouched'),
        (self._bad_shared_actor_rows, acts,
         '{} environment-frames of learn_actor_critic_shared() met rows of preferences that are not '
         'good (a NaN or a +inf, or five -inf); they took action {} and contributed nothing')]

  def _trace_rows(self, T):
    """int16 [K, B] (one frame) or [K, T, B] trace buffer, rows padded like the other streams."""
    B = self.batch
    pitch = (B + 15) // 16 * 16 if fused.PAD_ROWS else B
    shape = (self._n_planes, pitch) if T is None else (self._n_planes, T, pitch)
    return torch.empty(shape, dtype=torch.int16, device=self.device)[..., :B]

  # --------------------------------------------------------------------- API

  def showtime(self):
    """its_showtime(): state from the art, first observation, reward None."""
    first = self._obs
    if first.dtype != torch.int8:       # set_play_obs_dtype(): the first frame is rendered as int8
      first = torch.empty(self._obs.shape, dtype=torch.int8, device=self.device)
    self._wide(self._spec_host, self._tables, self.state, self.done, self.ret, None, first,
               self._board, None, None, None, None, self._step_trace, None, None, False)
    if first is not self._obs:
      self._obs.copy_(first)
    self.frame = 0
    return self._observation_cache, None, 1.0

  def reset(self):
    return self.showtime()

  def play(self, actions):
    if (torch.is_tensor(actions) and actions.dtype == torch.int8 and actions.device == self.device
        and actions.shape == (self.batch,) and actions.is_contiguous()):
      ids = actions
    else:
      ids = self._action_ids(actions, (self.batch,))
    validate = self.validate_actions
    self._wide(self._spec_host, self._tables, self.state, self.done, self.ret, ids, self._obs,
               self._board, self._reward, self._discount, self._step_done, self._perf_arg,
               self._step_trace, self._bad if validate else None,
               self._bad_flag if validate else None, False)
    self.frame += 1
    if validate:
      self._after_launch()
    return (self._observation_cache, (self._reward if self.any_reward else None), self._discount)

  def rollout_buffers(self, T, keep_obs=True, want_board=False, obs_dtype=torch.int8, share=None):
    out = super(WideGame, self).rollout_buffers(T, keep_obs, want_board, obs_dtype, share)
    out['trace'] = self._trace_rows(T)
    return out

  def rollout_trace_buffers(self, T):
    out = super(WideGame, self).rollout_trace_buffers(T)
    out['trace'] = self._trace_rows(T)
    return out

  def _trace_only_refusal(self):
    return None

  def _rollout_trace_op(self, ids, out, validate, reset_first):
    _hip.ops.wide_update(self._spec_host, self._tables, self.state, self.done, self.ret, ids,
                         out['reward'], out['discount'], out['done'], out['perf'], out['trace'],
                         self._bad if validate else None, self._bad_flag if validate else None,
                         bool(reset_first))

  # ------------------------------------------------------------ closed-loop rollouts

  @property
  def n_states(self):
    """States of the game's table: the rows of a `rollout_policy()` policy."""
    return int(self.spec.n_states)

  def _check_policy(self, policy):
    S = self.n_states
    if (not torch.is_tensor(policy) or policy.dtype != torch.float32 or policy.dim() != 2
        or tuple(policy.shape) != (S, gamespec.N_ACTIONS) or policy.device != self.device
        or not policy.is_contiguous()):
      got = ('{} {} on {}'.format(policy.dtype, list(policy.shape), policy.device)
             if torch.is_tensor(policy) else type(policy).__name__)
      raise ValueError('policy must be a contiguous float32 [{}, {}] tensor (n_states x actions) '
                       'on {}, got {}'.format(S, gamespec.N_ACTIONS, self.device, got))

  def _tensor_ok(self, t, dtype, shape):
    return (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape
            and t.device == self.device and t.is_contiguous())

  @staticmethod
  def _check_count(name, n):
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 1 << 20:
      raise ValueError('{0} must be an int, 1 <= {0} <= 2^20, got {1!r}'.format(name, n))

  def _planned_path(self, path, plan_fn, *args, what=None, n_cus=None, words=4):
    """The path (1 LDS, 2 global) a planning call takes: `path` checked, then what the library's
    plan function says for this table.  `what`: what path 1 would have to hold, for the message
    that it does not fit (default: the table).  `n_cus`: for a plan that asks for the device's
    compute units after wide_lds_max; `words`: of the plan it writes."""
    if path not in (0, 1, 2):
      raise ValueError('path must be 0 (chosen by arithmetic), 1 (LDS) or 2 (global), got {!r}'.format(path))
    plan = (ctypes.c_int64 * words)()
    lds_max = _hip.config_get('wide_lds_max')
    code = plan_fn(self.n_states, *(args + (lds_max,) + (() if n_cus is None else (n_cus,)) + (path, plan)))
    if code != 0 and path != 1:      # (only a forced path 1 can be refused for a checked call)
      raise ValueError('path={}: the library refused the plan (code {}; library setting '
                       'wide_lds_max = {})'.format(path, code, lds_max))
    if code != 0:
      raise ValueError('path=1: {} does not fit the LDS of one workgroup (library setting '
                       'wide_lds_max); use path=0 or path=2'.format(
                           what or 'a table of {} states'.format(self.n_states)))
    return int(plan[0])

  def _check_out(self, out, want, made_by):
    """`out` holds every (key, dtype, shape) of `want`, as the dict `made_by` allocates does."""
    if not isinstance(out, dict) or any(not self._tensor_ok(out.get(k), d, sh) for k, d, sh in want):
      raise ValueError('out must be a dict from {} of this game: {}'.format(
          made_by, ', '.join('{!r} {} {}'.format(k, d, list(sh)) for k, d, sh in want)))

  def _check_state_ids(self, state_ids):
    """(ids, N) of a `state_ids` argument: (None, n_states) for None - all states."""
    if state_ids is None:
      return None, self.n_states
    ids = state_ids
    if (not torch.is_tensor(ids) or ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 1
        or ids.numel() < 1 or ids.device != self.device):
      got = ('{} {} on {}'.format(ids.dtype, list(ids.shape), ids.device)
             if torch.is_tensor(ids) else type(ids).__name__)
      raise ValueError('state_ids must be an int32 or int64 [N] tensor on {}, N >= 1 (or None for '
                       'all {} states), got {}'.format(self.device, self.n_states, got))
    return ids.contiguous(), int(ids.numel())

  def rollout_policy_buffers(self, T, want_states=True):
    """Allocate the dict of `rollout_policy(out=...)` once: `rollout_trace_buffers(T)` plus
    'actions' int8 [T, B] and - `want_states` - 'states' int32 [T, B], rows padded alike."""
    out = self.rollout_trace_buffers(T)
    B = self.batch
    pitch = (B + 15) // 16 * 16 if fused.PAD_ROWS else B
    out['actions'] = torch.empty((T, pitch), dtype=torch.int8, device=self.device)[..., :B]
    if want_states:
      out['states'] = torch.empty((T, pitch), dtype=torch.int32, device=self.device)[..., :B]
    return out

  def rollout_policy(self, policy, T, seed=0, first_frame=None, reset_first=False, out=None,
                     want_states=True):
    """T frames of update pass in ONE launch, every action sampled on the device from `policy`:
    the closed-loop form of `rollout_trace()`.

    `policy` is a contiguous float32 `[n_states, 5]` tensor on the game's device: row s holds the
    weights of the five actions in state s (a tabular softmax policy, an epsilon-greedy Q-table,
    a network evaluated once on the game's states).  Weights need not be normalised; an action of
    weight exactly 0 is never taken; a one-hot row is a deterministic policy.  A tensor that
    requires grad is used through `.detach()`.  The row read is that of the state the frame
    starts from - row 0 for an environment whose episode ended on the frame before.

    Sampling (include/campx_hip.h has the rule in full) is counter-based: environment e at
    absolute frame f draws word f & 3 of the Philox4x32-10 block of key `seed`, counter
    (e, f >> 2).  `first_frame=None` continues a per-game frame counter - 0 at construction,
    advanced by T with every call - so that two calls of T1 and T2 frames sample what one call of
    T1 + T2 does; an explicit `first_frame` is used as given and sets the counter to
    `first_frame + T`.

    Returns `rollout_trace()`'s dict - 'trace', 'reward', 'discount', 'done', 'perf', same
    shapes, dtypes and row padding - plus 'actions' int8 [T, B], the actions taken, and with
    `want_states` 'states' int32 [T, B], the row each was sampled from.  For a learner
    `log pi = torch.log(p[out['states'].long(), out['actions'].long()])` with
    `p = policy / policy.sum(1, keepdim=True)` (differentiable in whatever `policy` was computed
    from).  `render_frames()` on 'trace', or `rollout(out['actions'])` from the same start, gives
    the observations.  `frame`, `ret` and the lazy error accounting are `rollout_trace()`'s: a
    row with a negative or NaN weight, or whose sum is not a positive finite number, makes the
    environment-frames that meet it take action 4 and raises ValueError - with their count -
    from this call or a later one, or from `check_actions()`.
    `out`: a dict from `rollout_policy_buffers(T, want_states)`, overwritten.
    """
    self._check_policy(policy)
    return self._closed_loop(_hip.ops.wide_policy_update, (), self._bad_rows,
                             'rollout_policy_buffers', policy, T, seed, first_frame, reset_first,
                             out, want_states)

  def _closed_loop(self, op, op_tail, bad_rows, made_by, policy, T, seed, first_frame, reset_first,
                   out, want_states):
    """What `rollout_policy()` and `rollout_population()` do once their policy is checked: T and
    the frame counter, `out` (a dict from `made_by`), the launch of `op` - whose last arguments are
    `op_tail` - with bad rows counted into `bad_rows`, and the tail."""
    T = int(T)
    if T < 1:
      raise ValueError('a rollout needs at least one frame: T >= 1')
    first = self._policy_frame if first_frame is None else int(first_frame)
    if first < 0 or first + T >= 1 << 63:
      raise ValueError('first_frame must be >= 0 and first_frame + T below 2^63')
    seed = int(seed) & ((1 << 64) - 1)
    if out is None:
      out = self.rollout_policy_buffers(T, want_states)
    else:
      rows = ([out.get('actions')] + ([out.get('states')] if want_states else [])
              if isinstance(out, dict) else [None])
      trace = out.get('trace') if isinstance(out, dict) else None
      if (not torch.is_tensor(trace) or trace.dim() != 3 or trace.shape[1] != T
          or any(not torch.is_tensor(r) or tuple(r.shape) != (T, self.batch)
                 or (T > 1 and r.stride(0) != trace.stride(1)) for r in rows)):
        raise ValueError('out must be a dict from {}({}, want_states={}) of '
                         'this game ({} environments)'.format(made_by, T, bool(want_states), self.batch))
    validate = self.validate_actions
    op(self._spec_host, self._tables, self.state, self.done, self.ret, policy.detach(),
       seed - (1 << 64) if seed >= 1 << 63 else seed, first, out['reward'], out['discount'],
       out['done'], out['perf'], out['trace'], out['actions'],
       out.get('states') if want_states else None, bad_rows if validate else None,
       self._bad_flag if validate else None, bool(reset_first), *op_tail)
    self._policy_frame = first + T
    self.frame = T if reset_first else self.frame + T
    self.check_ok()
    if validate:
      self._after_launch()
    return out

  # ------------------------------------------------------------ closed-loop rollouts of a population

  def _check_population(self, policies, split=True):
    """P of a `policies` argument, checked as `_check_policy()` checks a policy; `split`: the
    members also share out the environments (a rollout's do, an evaluation's need not)."""
    S, A, B = self.n_states, gamespec.N_ACTIONS, self.batch
    if (not torch.is_tensor(policies) or policies.dtype != torch.float32 or policies.dim() != 3
        or tuple(policies.shape[1:]) != (S, A) or policies.shape[0] < 1
        or policies.device != self.device or not policies.is_contiguous()):
      got = ('{} {} on {}'.format(policies.dtype, list(policies.shape), policies.device)
             if torch.is_tensor(policies) else type(policies).__name__)
      raise ValueError('policies must be a contiguous float32 [P, {}, {}] tensor (members x n_states x '
                       'actions) on {}, got {}'.format(S, A, self.device, got))
    P = int(policies.shape[0])
    if not split:
      return P
    if P > B or B % P != 0:
      raise ValueError('policies: the {} environments do not split into P = {} equal blocks (P must '
                       'divide the batch)'.format(B, P))
    if P * S >= 1 << 31:
      raise ValueError('policies: P * n_states = {} x {} must be below 2^31 (the flat rows of '
                       '\'states\' are int32)'.format(P, S))
    return P

  def rollout_population_buffers(self, T, want_states=True):
    """Allocate the dict of `rollout_population(out=...)` once: `rollout_policy_buffers()`'s, stream
    for stream."""
    return self.rollout_policy_buffers(T, want_states)

  def rollout_population(self, policies, T, seed=0, first_frame=None, reset_first=False, out=None,
                         want_states=True, path=0):
    """`rollout_policy()` for a POPULATION of P policies in one launch: block m of the environments
    samples policy m.

    `policies` is a contiguous float32 `[P, n_states, 5]` tensor on the game's device, P a divisor
    of the batch B, `P * n_states < 2^31`; a tensor that requires grad is used through `.detach()`.
    With `n = B // P`, environment e belongs to member `e // n`: members own equal, contiguous
    blocks of environments, so every `[T, B]` stream of the result is `[T, P, n]` by
    `unflatten(1, (P, n))` and `game.ret.view(P, n).mean(1)` is each member's mean episode return.

    Sampling is `rollout_policy()`'s rule, word for word - key `seed`, counter (absolute environment
    e, absolute frame >> 2), thresholds in f32 in action order, a bad row takes action 4 and is
    counted -; the row read for environment e in state s is `policies[e // n, s]` (s = 0 after a
    'done').  `first_frame=None` continues the per-game frame counter `rollout_policy()` advances:
    the two calls can be mixed and continued.

    Returns `rollout_policy()`'s dict - same keys, shapes, dtypes and row padding - in which
    'states' holds the FLAT row `(e // n) * n_states + s`: the row of
    `policies.view(P * n_states, 5)` the action was sampled from.  The learner's calls then serve
    all members in one launch each: `returns.table_lookup(policies.view(-1, 5), out['states'],
    out['actions'])`, `returns.sum_by_state(out['states'], out['actions'], ...,
    n_states=P * n_states)`, `V.view(-1)[out['states'].long()]` for a critic `[P, n_states]`.  The
    game's own state is `out['states'] % n_states` (for `render_states()`).  With P = 1 the call is
    `rollout_policy()` byte for byte.

    `out`: a dict from `rollout_population_buffers(T, want_states)`, overwritten; the call then
    allocates nothing and is capturable in a HIP graph.  `path`: 0 - a workgroup keeps the table
    and the thresholds of the members its 256 environments belong to in LDS whenever they fit
    (library setting wide_lds_max), else table and weights are read through L1 / L2; 1 / 2 force
    either (1 raises ValueError for what does not fit).  Both give the same bytes.

    Argument errors raise ValueError before anything is launched.  Bad rows raise lazily, as
    `rollout_policy()`'s do, in a message that names this call.
    """
    P = self._check_population(policies)
    self._planned_path(
        path, _hip.lib.campx_wide_population_plan, 1 if self.has_perf else 0, self.batch, P,
        what='a table of {} states with the thresholds of the members of one workgroup ({} environments '
             'per member)'.format(self.n_states, self.batch // P))
    return self._closed_loop(_hip.ops.wide_policy_population, (path,), self._bad_member_rows,
                             'rollout_population_buffers', policies, T, seed, first_frame,
                             reset_first, out, want_states)

  # ------------------------------------------------------------ online tabular learners

  def _windows_of(self, T, window):
    """(T, window, W) of a learner call: `window=None` is one window of T frames."""
    T = int(T)
    if T < 1 or T >= 1 << 31:
      raise ValueError('a run needs at least one frame: 1 <= T < 2^31')
    if window is None:
      window = T
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window < 1 << 31:
      raise ValueError('window must be None or an int, 1 <= window < 2^31, got {!r}'.format(window))
    return T, window, (T + window - 1) // window

  def learner_buffers(self, T, window=None):
    """Allocate the dict of `learn_tabular(out=...)` once: 'reward_sum' float32 [W, B], 'episodes'
    int32 [W, B] and - a game with hidden performance - 'perf_sum' int32 [W, B], with
    W = ceil(T / window) (`window=None`: one window of T frames)."""
    T, window, W = self._windows_of(T, window)
    B, dev = self.batch, self.device
    out = {'reward_sum': torch.zeros((W, B), dtype=torch.float32, device=dev),
           'episodes': torch.zeros((W, B), dtype=torch.int32, device=dev)}
    if self.has_perf:
      out['perf_sum'] = torch.zeros((W, B), dtype=torch.int32, device=dev)
    return out

  def _hyper_parameter(self, name, value, row, call, B):
    """float32 [B] on the device of `alpha`, `gamma`, `epsilon` or `lam` for the B learners of method
    `call`: a tensor as given, a Python number checked here and filled into row `row` of a tensor
    the game keeps per (call, B) - no allocation after the first call, and a captured call of one
    method never sees the numbers of the other."""
    if torch.is_tensor(value):
      if not self._tensor_ok(value, torch.float32, (B,)):
        raise ValueError('{} must be a number or a contiguous float32 [{}] tensor (one per learner) '
                         'on {}, got {} {} on {}'.format(name, B, self.device, value.dtype,
                                                         list(value.shape), value.device))
      return value.detach()
    if isinstance(value, bool) or not isinstance(value, (int, float)):
      raise ValueError('{} must be a number or a float32 [{}] tensor, got {}'.format(
          name, B, type(value).__name__))
    unit = name in ('epsilon', 'lam')
    if (not math.isfinite(value) or abs(value) > torch.finfo(torch.float32).max
        or (unit and not 0.0 <= value <= 1.0)):
      raise ValueError('{} must be a finite number (as a float32){}, got {!r}'.format(
          name, ' in [0, 1]' if unit else '', value))
    if (call, B) not in self._hyper_floats:
      self._hyper_floats[call, B] = torch.zeros((4, B), dtype=torch.float32, device=self.device)
    return self._hyper_floats[call, B][row].fill_(float(value))

  def _learner_prologue(self, call, learners, T, window, rule, first_frame, seed, alpha, gamma,
                        epsilon, out, own, made_by, make_out, names=('alpha', 'gamma', 'epsilon')):
    """What learn_tabular() and learn_shared() do after their own checks of q and P: returns T,
    window, the first frame, the seed as the op's signed int64, the checked (or made) `out` and
    alpha, gamma, epsilon as float32 [learners].  `own`: the call's own entries of `out`;
    `made_by(T, window)`: the call that makes `out`, for the message; `make_out(T, window)`.
    `names`: what the call names its three hyper-parameters (learn_actor_critic()'s are two step
    sizes and gamma)."""
    B = self.batch
    T, window, W = self._windows_of(T, window)
    if rule not in _hip.LEARN_RULES:
      raise ValueError('rule must be \'q\' or \'expected_sarsa\', got {!r}'.format(rule))
    first = self._policy_frame if first_frame is None else int(first_frame)
    if first < 0 or first + T >= 1 << 63:
      raise ValueError('first_frame must be >= 0 and first_frame + T below 2^63')
    seed = int(seed) & ((1 << 64) - 1)
    want = [('reward_sum', torch.float32, (W, B)), ('episodes', torch.int32, (W, B))] + own
    if self.has_perf:
      want.append(('perf_sum', torch.int32, (W, B)))
    if out is None:
      out = make_out(T, window)
    else:
      self._check_out(out, want, made_by(T, window))
    hyper = (self._hyper_parameter(names[0], alpha, 0, call, learners),
             self._hyper_parameter(names[1], gamma, 1, call, learners),
             self._hyper_parameter(names[2], epsilon, 2, call, learners))
    return T, window, first, seed - (1 << 64) if seed >= 1 << 63 else seed, out, hyper

  def _learner_epilogue(self, first, T, reset_first, q, out, own=()):
    """The frame counters, the lazy errors and the result dict of a learner call."""
    self._policy_frame = first + T
    self.frame = T if reset_first else self.frame + T
    self.check_ok()
    if self.validate_actions:
      self._after_launch()
    res = {'q': q, 'reward_sum': out['reward_sum'], 'episodes': out['episodes']}
    for k in own:
      res[k] = out[k]
    if self.has_perf:
      res['perf_sum'] = out['perf_sum']
    return res

  def learn_tabular(self, T, q=None, alpha=0.1, gamma=0.99, epsilon=0.1, rule='q', seed=0,
                    first_frame=None, reset_first=False, window=None, out=None, path=0):
    """T frames of ONLINE tabular learning for B independent learners in ONE launch: environment e
    is learner e, with its own Q-table `q[e]`.  Every frame it acts epsilon-greedily on its table,
    and `q[e, s, a]` is updated at once - the next frame's action is chosen from the updated table
    (csrc/k_learn.hip, `campx::wide_learn`).  Nothing is shared between learners, so there are no
    atomics and the run is reproducible bit for bit (include/campx_hip.h has the rule in full;
    tests/learner_reference.py restates it in numpy).

    Args:
      q: contiguous float32 `[B, n_states, 5]` on the game's device (16-byte aligned,
          `B * n_states * 5 < 2^31`), updated IN PLACE; None: zeros.  `q[m]` compares with
          `value_iteration()`'s 'q'; `softmax(q, 2)` or a one-hot of `q.argmax(2)` is what
          `rollout_population()` takes.
      alpha, gamma, epsilon: the step size, the discount factor and the exploration rate, each a
          Python number or a float32 `[B]` tensor - a tensor is what makes a sweep.  A learner
          whose alpha, gamma or epsilon is not finite, or whose epsilon is outside [0, 1], is BAD:
          it takes action 4 at every frame, its table is left untouched, and it raises ValueError -
          counted once per call - lazily, as bad actions do: from `check_actions()` or a later
          call, under `validate_actions='sync'` from this one.  Python numbers are checked at once.
      rule: 'q' - Q-learning, the bootstrap is `max_a q[e, n, a]` - or 'expected_sarsa': the
          bootstrap is the expectation of `q[e, n, .]` under the learner's own epsilon-greedy
          policy, `(1 - epsilon) * max + epsilon * mean`.  In both, the target is
          `r + (gamma * D) * bootstrap` (r alone on a frame that ends the episode; a reward of None
          counts as 0; D is the frame's discount as in `evaluate_policy()`), and
          `q[e, s, a] += alpha * (target - q[e, s, a])`.  Expected SARSA is the on-policy form
          that needs nothing carried between frames; SARSA proper needs the NEXT frame's committed
          action, across launches too, and is not offered.  Several environments feeding ONE
          learner are `learn_shared()`: its atomics add integers, so it repeats bit for bit too.
      seed, first_frame: exploration is counter-based - learner e at absolute frame f draws from
          the Philox4x32-10 block of key `seed`, counter (e, f >> 1, 1) - a stream unrelated to
          `rollout_policy()`'s for the same seed.  `first_frame=None` continues the per-game frame
          counter that `rollout_policy()` advances, so that two calls of T1 and T2 frames learn
          what one call of T1 + T2 does; an explicit `first_frame` sets it to `first_frame + T`.
      reset_first: every learner starts a new episode (its table stays).
      window: frames per window of the learning curves; None: one window of T frames.  Windows
          count from this call's frame 0; the last one may be short.
      out: a dict from `learner_buffers(T, window)`, overwritten.  With `q` and `out` (and
          tensors, or the same numbers as before, for the hyper-parameters) the call allocates
          nothing and is capturable in a HIP graph.
      path: 0 - a workgroup keeps the table and its 256 learners' Q-tables in LDS whenever they
          fit (library setting wide_lds_max: up to 28 states), else each learner reads and writes
          its rows of `q` through L1 / L2; 1 / 2 force either (1 raises ValueError for what does
          not fit).  Both give the same bits.

    Returns a dict: 'q'; 'reward_sum' float32 `[W, B]`, the real reward per window, summed in
    frame order; 'perf_sum' int32 `[W, B]`, the hidden performance per window (games that have
    one); 'episodes' int32 `[W, B]`, the episodes that ended in the window; W = ceil(T / window).
    No `[T, B]` stream is written.  `state`, `done`, `ret` and `frame` carry over exactly as
    `rollout_policy()` leaves them.  Argument errors raise ValueError before anything is launched.
    """
    S, A, B, dev = self.n_states, gamespec.N_ACTIONS, self.batch, self.device
    if B * S * A >= 1 << 31:
      raise ValueError('learn_tabular(): B * n_states * 5 = {} x {} x 5 must be below 2^31; use a '
                       'smaller batch'.format(B, S))
    if q is not None and (not self._tensor_ok(q, torch.float32, (B, S, A)) or q.data_ptr() % 16):
      got = ('{} {} on {}'.format(q.dtype, list(q.shape), q.device) if torch.is_tensor(q)
             else type(q).__name__)
      raise ValueError('q must be a contiguous, 16-byte aligned float32 [{}, {}, {}] tensor (learners '
                       'x n_states x actions) on {}, or None for zeros; got {}'.format(B, S, A, dev, got))
    self._planned_path(path, _hip.lib.campx_wide_learn_plan, 1 if self.has_perf else 0, B,
                       what='a table of {} states with the Q-tables of a workgroup\'s 256 '
                            'learners'.format(S))
    T, window, first, seed, out, hyper = self._learner_prologue(
        'learn_tabular', B, T, window, rule, first_frame, seed, alpha, gamma, epsilon, out, [],
        'learner_buffers({}, window={})'.format, self.learner_buffers)
    if q is None:
      q = torch.zeros((B, S, A), dtype=torch.float32, device=dev)
    validate = self.validate_actions
    _hip.ops.wide_learn(
        self._spec_host, self._tables, self.state, self.done, self.ret, q.detach(), hyper[0],
        hyper[1], hyper[2], _hip.LEARN_RULES[rule], seed, first, T, window, out['reward_sum'],
        out.get('perf_sum') if self.has_perf else None, out['episodes'],
        self._bad_learners if validate else None, self._bad_flag if validate else None,
        bool(reset_first), path)
    return self._learner_epilogue(first, T, reset_first, q, out)

  # ------------------------------------------------------------ learners with eligibility traces

  def _traces_plan(self, path, team):
    """The five words of campx_wide_traces_plan() for this game - path, lanes of a learner, LDS
    bytes, threads, entries in LDS - after the checks of `path` and `team` that have a message."""
    S = self.n_states
    if path not in (0, 1, 2):
      raise ValueError('path must be 0 (chosen by arithmetic), 1 (LDS) or 2 (global), got {!r}'.format(path))
    if (isinstance(team, bool) or not isinstance(team, int) or not 0 <= team <= 256
        or team & (team - 1)):
      raise ValueError('team must be 0 (chosen by arithmetic) or a power of two up to 256, got {!r}'.format(team))
    plan = (ctypes.c_int64 * 5)()
    lds_max = _hip.config_get('wide_lds_max')
    code = _hip.lib.campx_wide_traces_plan(S, 1 if self.has_perf else 0, self.batch, lds_max, path,
                                           team, plan)
    if code != 0 and path == 1:
      raise ValueError('path=1, team={}: a table of {} states with the Q-tables and traces of a '
                       'workgroup\'s {} do not fit the LDS of one workgroup (library setting '
                       'wide_lds_max); use path=0 or path=2{}'.format(
                           team, S,
                           '256 / team = {} learners'.format(256 // team) if team else 'one learner',
                           ', or a larger team' if team else ''))
    if code != 0:
      raise ValueError('path={}, team={}: the library refused the plan (code {}; library setting '
                       'wide_lds_max = {})'.format(path, team, code, lds_max))
    return list(plan)

  def learn_traces(self, T, q=None, traces=None, lam=0.9, trace='accumulating', alpha=0.1, gamma=0.99,
                   epsilon=0.1, rule='q', seed=0, first_frame=None, reset_first=False, window=None,
                   out=None, path=0, team=0):
    """T frames of online tabular learning WITH ELIGIBILITY TRACES for B independent learners in ONE
    launch: Watkins's Q(lambda) (`rule='q'`) or expected SARSA(lambda).  Environment e is learner e,
    as in `learn_tabular()`, with its own table `q[e]` and its own trace per (state, action),
    `traces[e]`: every frame's TD error moves EVERY entry in proportion to its trace, so that a
    reward reaches the whole path that led to it at once, not one state per visit
    (csrc/k_learn.hip, `campx::wide_learn_traces`).  No reduction and no atomics: the run repeats
    bit for bit (include/campx_hip.h has the frame; tests/trace_learner_reference.py restates it
    in numpy).

    The frame of a learner in state s: it acts on `q[e, s]` as `learn_tabular()` does (the same
    exploration stream); for `rule='q'` an action whose value is not the row's maximum CUTS the
    traces (all zero); the TD error `delta` is `learn_tabular()`'s; the trace of (s, a) is bumped -
    `trace='accumulating'`: plus 1, `'replacing'`: set to 1; every entry with a trace that is not
    zero moves by `alpha * delta * trace`; and the traces decay by `gamma * D * lam`, or are
    zeroed when the frame ends the episode.  `lam=0` is `learn_tabular()` bit for bit.

    Args:
      q, traces: contiguous float32 `[B, n_states, 5]` on the game's device (16-byte aligned,
          `B * n_states * 5 < 2^31`), both updated IN PLACE; None: zeros.  Pass the returned
          'traces' on and calls of T1 and T2 frames learn what one call of T1 + T2 does.
      lam: the trace decay, a Python number in [0, 1] (checked at once) or a float32 `[B]` tensor -
          a tensor is a sweep of lambda.
      trace: 'accumulating' or 'replacing'.
      alpha, gamma, epsilon, rule, seed, first_frame, window: exactly as in `learn_tabular()`.  A
          learner that is bad there, or whose lam is not within [0, 1], takes action 4 at every
          frame, keeps its table AND its traces, and raises ValueError lazily, counted once.
      reset_first: every learner starts a new episode, and its traces from zero.
      out: a dict from `learner_buffers(T, window)`, overwritten.  With `q`, `traces` and `out`
          (and tensors, or the same numbers as before, for the hyper-parameters) the call
          allocates nothing and is capturable in a HIP graph.
      path, team: a learner is a team of `team` lanes (a power of two up to 256) that share the
          sweep over its entries; a workgroup holds 256 / team learners.  0 and 0: the smallest
          team for which the table and the workgroup's tables and traces fit the LDS (library
          setting wide_lds_max: one lane up to 14 states, two up to 28, ..., 256 up to about
          1 800), else tables and traces go through L1 / L2 with a team of 256.  `path=1` / `2`
          and `team=` force either; a forced shape that does not fit raises ValueError.  No
          choice changes a bit of any result.

    Returns a dict: 'q', 'traces', and `learn_tabular()`'s 'reward_sum', 'episodes' and
    'perf_sum'.  `state`, `done`, `ret` and `frame` carry over exactly as `learn_tabular()` leaves
    them.  Argument errors raise ValueError before anything is launched.
    """
    S, A, B, dev = self.n_states, gamespec.N_ACTIONS, self.batch, self.device
    if B * S * A >= 1 << 31:
      raise ValueError('learn_traces(): B * n_states * 5 = {} x {} x 5 must be below 2^31; use a '
                       'smaller batch'.format(B, S))
    for name, t in (('q', q), ('traces', traces)):
      if t is not None and (not self._tensor_ok(t, torch.float32, (B, S, A)) or t.data_ptr() % 16):
        got = ('{} {} on {}'.format(t.dtype, list(t.shape), t.device) if torch.is_tensor(t)
               else type(t).__name__)
        raise ValueError('{} must be a contiguous, 16-byte aligned float32 [{}, {}, {}] tensor '
                         '(learners x n_states x actions) on {}, or None for zeros; got {}'.format(
                             name, B, S, A, dev, got))
    if trace not in _hip.TRACE_KINDS:
      raise ValueError('trace must be \'accumulating\' or \'replacing\', got {!r}'.format(trace))
    self._traces_plan(path, team)
    # (lam first: a bad number must not leave the other rows of the cache filled for nothing)
    lams = self._hyper_parameter('lam', lam, 3, 'learn_traces', B)
    T, window, first, seed, out, hyper = self._learner_prologue(
        'learn_traces', B, T, window, rule, first_frame, seed, alpha, gamma, epsilon, out, [],
        'learner_buffers({}, window={})'.format, self.learner_buffers)
    if q is None:
      q = torch.zeros((B, S, A), dtype=torch.float32, device=dev)
    if traces is None:
      traces = torch.zeros((B, S, A), dtype=torch.float32, device=dev)
    validate = self.validate_actions
    _hip.ops.wide_learn_traces(
        self._spec_host, self._tables, self.state, self.done, self.ret, q.detach(), traces.detach(),
        hyper[0], hyper[1], hyper[2], lams, _hip.LEARN_RULES[rule], _hip.TRACE_KINDS[trace], seed,
        first, T, window, out['reward_sum'], out.get('perf_sum') if self.has_perf else None,
        out['episodes'], self._bad_trace_learners if validate else None,
        self._bad_flag if validate else None, bool(reset_first), path, team)
    res = self._learner_epilogue(first, T, reset_first, q, out)
    res['traces'] = traces
    return res

  # ------------------------------------------------------------ Dyna-Q learners

  def _dyna_plan(self, path):
    """The five words of campx_wide_dyna_plan() for this game: path, LDS bytes, threads, entries in
    LDS, bitmap words per learner."""
    S, B = self.n_states, self.batch
    if B * S * gamespec.N_ACTIONS >= 1 << 31:
      raise ValueError('learn_dyna(): B * n_states * 5 = {} x {} x 5 must be below 2^31; use a '
                       'smaller batch'.format(B, S))
    if path not in (0, 1, 2):
      raise ValueError('path must be 0 (chosen by arithmetic), 1 (LDS) or 2 (global), got {!r}'.format(path))
    plan = (ctypes.c_int64 * 5)()
    lds_max = _hip.config_get('wide_lds_max')
    code = _hip.lib.campx_wide_dyna_plan(S, 1 if self.has_perf else 0, B, lds_max, path, plan)
    if code != 0 and path == 1:
      raise ValueError('path=1: a table of {} states with the Q-tables, seen lists and bitmaps of a '
                       'workgroup\'s 256 learners does not fit the LDS of one workgroup (library '
                       'setting wide_lds_max); use path=0 or path=2'.format(S))
    if code != 0:
      raise ValueError('path={}: the library refused the plan (code {}; library setting '
                       'wide_lds_max = {})'.format(path, code, lds_max))
    return list(plan)

  def dyna_buffers(self, T, window=None, path=0):
    """Allocate the dict of `learn_dyna(out=...)` once: `learner_buffers(T, window)`'s tensors and -
    when a call with this `path` goes through global memory (path 2) - 'marks', its membership
    bitmap: int32 [B, ceil(n_states * 5 / 32)], scratch whose contents mean nothing between calls."""
    plan = self._dyna_plan(path)
    out = self.learner_buffers(T, window)
    if plan[0] == 2:
      out['marks'] = torch.zeros((self.batch, plan[4]), dtype=torch.int32, device=self.device)
    return out

  def learn_dyna(self, T, q=None, model=None, planning=5, alpha=0.1, gamma=0.99, epsilon=0.1,
                 rule='q', seed=0, first_frame=None, reset_first=False, window=None, out=None,
                 path=0):
    """T frames of DYNA-Q for B independent learners in ONE launch: `learn_tabular()`'s frame and,
    after every real step, `planning` more updates of pairs the learner REMEMBERS - more learning
    per frame of experience (Sutton & Barto ch. 8; csrc/k_learn.hip, `campx::wide_learn_dyna`).
    Environment e is learner e, with its own table `q[e]` and its own model.  The game's table is
    deterministic, so what a learner has to remember of a visited (s, a) is only THAT it visited
    it: the model is the list of the flat entries `s * 5 + a` it has met, in order of first visit.
    Nothing is shared between learners: no atomics, and the run repeats bit for bit
    (include/campx_hip.h has the frame; tests/dyna_learner_reference.py restates it in numpy).

    The frame: the real step is `learn_tabular()`'s; the pair is appended to the model if it is
    new; then, `planning` times, one after the other: a pair is drawn UNIFORMLY FROM THE SEEN PAIRS
    (not "a seen state, then an action taken in it": a state met with four actions is drawn four
    times as often as one met with one), and `q` of that pair gets the one-step update from the
    table's entry for it, each update seeing the ones before.  The next frame acts on `q` as
    planning left it.  `planning=0` is `learn_tabular()` bit for bit, and records the model.

    Args:
      q: as in `learn_tabular()`: float32 `[B, n_states, 5]`, updated IN PLACE; None: zeros.
      model: a dict `{'seen': int32 [B, n_states * 5], 'n_seen': int32 [B]}` of contiguous tensors
          on the game's device ('seen' 16-byte aligned), both updated IN PLACE; None: empty.  The
          first `n_seen[e]` elements of `seen[e]` are learner e's pairs; the rest is never read or
          written.  Pass the returned 'model' on and calls of T1 and T2 frames learn what one call
          of T1 + T2 does.  A learner whose `n_seen` or listed pairs are outside the table is BAD.
          A list with repeats is used as given: a repeat is drawn as often as it is listed.
      planning: updates per frame, a Python int in 0 .. 1024 (checked at once) or an int32 `[B]`
          tensor - a tensor is a sweep of n; a learner whose n is outside 0 .. 1024 is BAD.
      alpha, gamma, epsilon, rule, seed, first_frame, window: exactly as in `learn_tabular()`.
          The planning draws come from the exploration stream's key with a counter word of their
          own: (e, frame, 2 + k // 4).  A BAD learner - here or as in `learn_tabular()` - takes
          action 4 at every frame, keeps its table AND its model, and raises ValueError lazily,
          counted once per call.
      reset_first: every learner starts a new episode; table and model stay.
      out: a dict from `dyna_buffers(T, window, path)`, overwritten.  With `q`, `model`, `out` and
          tensors (or the same numbers as before) for the hyper-parameters the call allocates
          nothing and is capturable in a HIP graph.
      path: 0 - a workgroup keeps the table and its 256 learners' Q-tables, lists (16 bits an
          element) and bitmaps in LDS whenever they fit (library setting wide_lds_max: up to 18
          states), else they go through L1 / L2; 1 / 2 force either (1 raises ValueError for what
          does not fit).  Both give the same bits.

    Returns `learn_tabular()`'s dict plus 'model'.  `state`, `done`, `ret` and `frame` carry over
    exactly as `learn_tabular()` leaves them.  Argument errors raise ValueError before anything is
    launched.
    """
    S, A, B, dev = self.n_states, gamespec.N_ACTIONS, self.batch, self.device
    plan = self._dyna_plan(path)
    if q is not None and (not self._tensor_ok(q, torch.float32, (B, S, A)) or q.data_ptr() % 16):
      got = ('{} {} on {}'.format(q.dtype, list(q.shape), q.device) if torch.is_tensor(q)
             else type(q).__name__)
      raise ValueError('q must be a contiguous, 16-byte aligned float32 [{}, {}, {}] tensor (learners '
                       'x n_states x actions) on {}, or None for zeros; got {}'.format(B, S, A, dev, got))
    if model is not None and (
        not isinstance(model, dict) or not self._tensor_ok(model.get('seen'), torch.int32, (B, S * A))
        or model['seen'].data_ptr() % 16 or not self._tensor_ok(model.get('n_seen'), torch.int32, (B,))):
      raise ValueError('model must be None (empty) or a dict of contiguous int32 tensors on {}: '
                       '\'seen\' [{}, {}], 16-byte aligned, and \'n_seen\' [{}]'.format(dev, B, S * A, B))
    if torch.is_tensor(planning):
      if not self._tensor_ok(planning, torch.int32, (B,)):
        raise ValueError('planning must be an int or a contiguous int32 [{}] tensor (one per learner) '
                         'on {}, got {} {} on {}'.format(B, dev, planning.dtype, list(planning.shape),
                                                         planning.device))
    elif (isinstance(planning, bool) or not isinstance(planning, int)
          or not 0 <= planning <= _hip.DYNA_MAX_PLANNING):
      raise ValueError('planning must be an int, 0 <= planning <= {}, or an int32 [{}] tensor, got '
                       '{!r}'.format(_hip.DYNA_MAX_PLANNING, B, planning))
    own = [('marks', torch.int32, (B, plan[4]))] if plan[0] == 2 else []
    T, window, first, seed, out, hyper = self._learner_prologue(
        'learn_dyna', B, T, window, rule, first_frame, seed, alpha, gamma, epsilon, out, own,
        lambda T, window: 'dyna_buffers({}, window={}, path={})'.format(T, window, path),
        lambda T, window: self.dyna_buffers(T, window, path))
    if not torch.is_tensor(planning):
      if B not in self._hyper_ints:
        self._hyper_ints[B] = torch.zeros((B,), dtype=torch.int32, device=dev)
      planning = self._hyper_ints[B].fill_(planning)
    if q is None:
      q = torch.zeros((B, S, A), dtype=torch.float32, device=dev)
    if model is None:
      model = {'seen': torch.zeros((B, S * A), dtype=torch.int32, device=dev),
               'n_seen': torch.zeros((B,), dtype=torch.int32, device=dev)}
    validate = self.validate_actions
    _hip.ops.wide_learn_dyna(
        self._spec_host, self._tables, self.state, self.done, self.ret, q.detach(), model['seen'],
        model['n_seen'], planning, hyper[0], hyper[1], hyper[2], _hip.LEARN_RULES[rule], seed, first,
        T, window, out['reward_sum'], out.get('perf_sum') if self.has_perf else None,
        out['episodes'], out.get('marks') if plan[0] == 2 else None,
        self._bad_dyna_learners if validate else None, self._bad_flag if validate else None,
        bool(reset_first), path)
    res = self._learner_epilogue(first, T, reset_first, q, out)
    res['model'] = model
    return res

  # ------------------------------------------------------------ actor-critic learners

  def learn_actor_critic(self, T, prefs=None, values=None, alpha_actor=0.1, alpha_critic=0.1,
                         gamma=0.99, seed=0, first_frame=None, reset_first=False, window=None,
                         out=None, path=0):
    """T frames of ONE-STEP ACTOR-CRITIC for B independent learners in ONE launch: environment e is
    learner e, with a softmax policy of its own - the preferences `prefs[e]` - and a critic
    `values[e]` (Sutton & Barto 13.5, without the gamma^t factor; csrc/k_learn.hip,
    `campx::wide_learn_actor`).  The policy-gradient sibling of `learn_tabular()`: what
    `examples/actor_critic_per_state.py` does from the host - a rollout, a returns pass, a
    `sum_by_state()` and a torch step per update, for one learner - as one launch for a sweep of
    them.  Nothing is shared between learners: no atomics, and the run repeats bit for bit
    (include/campx_hip.h has rule and frame; tests/actor_critic_reference.py restates them in numpy).

    The frame, from state s: the weights `w = returns.softmax_weights(prefs[e, s])` - a stated
    float32 rule, NOT `exp`, so that they repeat bit for bit everywhere - and the action by
    `rollout_policy()`'s own sampler with `rollout_policy()`'s own stream (key `seed`, counter
    (e, frame >> 2), word frame & 3); the entry gives n, r, done, D;
    `delta = (r if done else r + (gamma * D) * values[e, n]) - values[e, s]`;
    `values[e, s] += alpha_critic * delta`; and, for each a', with `pi = w[a'] / sum(w)`,
    `prefs[e, s, a'] += (alpha_actor * delta) * ((a' == a) - pi)`.

    Args:
      prefs: contiguous float32 `[B, n_states, 5]` on the game's device (16-byte aligned,
          `B * n_states * 5 < 2^31`), updated IN PLACE; None: zeros, the uniform policy.  A
          preference of -inf is an action never taken.  A row with a NaN or a +inf (or five -inf)
          is NOT GOOD: an environment-frame that meets it takes action 4, changes neither table
          and is counted; the count raises ValueError lazily, as `rollout_policy()`'s bad rows do.
          `returns.softmax_weights(prefs)` is what `rollout_population()`,
          `evaluate_population()` and `state_visitation()` take: exactly the probabilities the
          learner sampled from.
      values: contiguous float32 `[B, n_states]` (16-byte aligned), updated IN PLACE; None: zeros.
      alpha_actor, alpha_critic, gamma: the two step sizes and the discount factor, each a Python
          number or a float32 `[B]` tensor - a tensor is what makes a sweep.  A learner with one
          that is not finite is BAD: it takes action 4 at every frame, both tables are left
          untouched, and it raises ValueError - counted once per call - lazily.  Python numbers are
          checked at once.  With both step sizes 0 the learners walk exactly as
          `rollout_population(softmax_weights(prefs), T, seed, first_frame)` does with P = B.
      seed, first_frame, reset_first, window: as in `learn_tabular()`, except that the stream is
          `rollout_policy()`'s, not the exploration stream.
      out: a dict from `learner_buffers(T, window)`, overwritten.  With `prefs`, `values`, `out`
          and tensors (or the same numbers as before) for the hyper-parameters the call allocates
          nothing and is capturable in a HIP graph.
      path: 0 - a workgroup keeps the table and its 256 learners' preferences and values in LDS
          whenever they fit (library setting wide_lds_max: 24 bytes a state and learner, up to 23
          states), else each learner works on its rows through L1 / L2; 1 / 2 force either (1
          raises ValueError for what does not fit).  Both give the same bits.

    Returns a dict: 'prefs', 'values' and `learn_tabular()`'s window rows 'reward_sum', 'episodes'
    and 'perf_sum'.  `state`, `done`, `ret` and `frame` carry over exactly as `learn_tabular()`
    leaves them.  Argument errors raise ValueError before anything is launched.

    NOT offered: REINFORCE with episode returns (use `rollout_policy()` and
    `returns.discounted_returns()`), lambda-traces for the actor, an entropy bonus or a temperature.
    The shared form in which several actors feed one learner is `learn_actor_critic_shared()`.
    """
    S, A, B, dev = self.n_states, gamespec.N_ACTIONS, self.batch, self.device
    if B * S * A >= 1 << 31:
      raise ValueError('learn_actor_critic(): B * n_states * 5 = {} x {} x 5 must be below 2^31; use '
                       'a smaller batch'.format(B, S))
    for name, t, shape in (('prefs', prefs, (B, S, A)), ('values', values, (B, S))):
      if t is not None and (not self._tensor_ok(t, torch.float32, shape) or t.data_ptr() % 16):
        got = ('{} {} on {}'.format(t.dtype, list(t.shape), t.device) if torch.is_tensor(t)
               else type(t).__name__)
        raise ValueError('{} must be a contiguous, 16-byte aligned float32 {} tensor on {}, or None '
                         'for zeros; got {}'.format(name, list(shape), dev, got))
    self._planned_path(path, _hip.lib.campx_wide_actor_plan, 1 if self.has_perf else 0, B,
                       what='a table of {} states with the preferences and values of a workgroup\'s '
                            '256 learners'.format(S))
    T, window, first, seed, out, hyper = self._learner_prologue(
        'learn_actor_critic', B, T, window, 'q', first_frame, seed, alpha_actor, gamma, alpha_critic,
        out, [], 'learner_buffers({}, window={})'.format, self.learner_buffers,
        names=('alpha_actor', 'gamma', 'alpha_critic'))
    if prefs is None:
      prefs = torch.zeros((B, S, A), dtype=torch.float32, device=dev)
    if values is None:
      values = torch.zeros((B, S), dtype=torch.float32, device=dev)
    validate = self.validate_actions
    _hip.ops.wide_learn_actor(
        self._spec_host, self._tables, self.state, self.done, self.ret, prefs.detach(),
        values.detach(), hyper[0], hyper[2], hyper[1], seed, first, T, window, out['reward_sum'],
        out.get('perf_sum') if self.has_perf else None, out['episodes'],
        self._bad_actor_learners if validate else None, self._bad_actor_rows if validate else None,
        self._bad_flag if validate else None, bool(reset_first), path)
    res = self._learner_epilogue(first, T, reset_first, prefs, out)
    del res['q']
    res['prefs'], res['values'] = prefs, values
    return res

  # ------------------------------------------------------------ shared online learners

  def _shared_plan(self, P, path, call='learn_shared()', plan_fn=None,
                   holds='the Q-table and the accumulators'):
    """The six words of campx_wide_shared_plan() - or of `plan_fn`, the same rule for another
    kernel - for P learners of this game: path, learners per workgroup, threads, LDS bytes, entries
    in LDS, accumulator copies, after the checks of P that have a message of their own.  `call`
    names the method in them; `holds`: what path 1 keeps per learner beside the table."""
    S, A, B = self.n_states, gamespec.N_ACTIONS, self.batch
    if isinstance(P, bool) or not isinstance(P, int) or P < 1 or P > B or B % P != 0:
      raise ValueError('{}: the {} environments do not split into P = {!r} equal blocks '
                       '(P must divide the batch)'.format(call, B, P))
    if B // P > 1024:
      raise ValueError('{}: {} environments per learner are more than one workgroup '
                       'holds: n = B / P must be at most 1024'.format(call, B // P))
    if P * S * A >= 1 << 31:
      raise ValueError('{}: P * n_states * 5 = {} x {} x 5 must be below 2^31'.format(call, P, S))
    if path not in (0, 1, 2):
      raise ValueError('path must be 0 (chosen by arithmetic), 1 (LDS) or 2 (global), got {!r}'.format(path))
    plan = (ctypes.c_int64 * 6)()
    lds_max = _hip.config_get('wide_lds_max')
    plan_fn = plan_fn or _hip.lib.campx_wide_shared_plan
    code = plan_fn(S, 1 if self.has_perf else 0, B, P, lds_max, path, plan)
    if code != 0 and path == 1:
      raise ValueError('path=1: a table of {} states with {} of one '
                       'learner does not fit the LDS of one workgroup (library setting '
                       'wide_lds_max); use path=0 or path=2'.format(S, holds))
    if code != 0:
      raise ValueError('path={}: the library refused the plan (code {}; library setting '
                       'wide_lds_max = {})'.format(path, code, lds_max))
    return list(plan)

  def shared_learner_buffers(self, P, T, window=None, path=0):
    """Allocate the dict of `learn_shared(out=...)` once, for P learners: `learner_buffers(T,
    window)`'s tensors, 'clamped' int64 [P] and - when a call with this `path` goes through global
    memory (path 2) - 'scratch', its accumulators: int32 [3 * P * n_states * 5], zero, and left
    zero by every call."""
    plan = self._shared_plan(P, path)
    out = self.learner_buffers(T, window)
    out['clamped'] = torch.zeros((P,), dtype=torch.int64, device=self.device)
    if plan[0] == 2:
      out['scratch'] = torch.zeros((3 * P * self.n_states * gamespec.N_ACTIONS,), dtype=torch.int32,
                                   device=self.device)
    return out

  def learn_shared(self, T, q, alpha=0.1, gamma=0.99, epsilon=0.1, rule='q', seed=0,
                   first_frame=None, reset_first=False, window=None, out=None, path=0):
    """T frames of online tabular learning for P SHARED learners in ONE launch: learner m owns the
    table `q[m]` and is fed by the n = B / P environments `[m * n, (m + 1) * n)` - one agent that
    learns from n parallel actors, `rollout_population()`'s split of the batch (csrc/k_learn.hip,
    `campx::wide_learn_shared`).

    The learner is synchronous.  Within a frame every environment of a learner acts
    epsilon-greedily on the same table - the table as the frame found it - and computes its own TD
    error, `learn_tabular()`'s, with the learner's alpha, gamma and epsilon.  The errors are
    quantised to 64-bit fixed point (32 fractional bits) and summed per (state, action) as
    integers, and each visited `q[m, s, a]` moves once, by alpha times the MEAN error of its
    visitors: the step size does not depend on n, and the run repeats bit for bit whatever the
    order in which environments arrive (include/campx_hip.h has the rule in full;
    tests/shared_learner_reference.py restates it in numpy).

    Args:
      q: contiguous float32 `[P, n_states, 5]` on the game's device (16-byte aligned,
          `P * n_states * 5 < 2^31`), updated IN PLACE; P is read from it, so None is not allowed.
          P must divide the batch, and 1 <= n = B / P <= 1024, the largest workgroup: a learner's
          environments sit in one workgroup, whose barrier is the per-frame synchronisation.  More
          actors than one workgroup holds would need a grid-wide barrier per frame: out of scope.
      alpha, gamma, epsilon: each a Python number or a float32 `[P]` tensor - a tensor is a sweep.
          A learner whose alpha, gamma or epsilon is not finite, or whose epsilon is outside
          [0, 1], is BAD: all its environments take action 4 at every frame, its table is left
          untouched, and it raises ValueError - counted once per learner and call - lazily, as bad
          learners of `learn_tabular()` do.  Python numbers are checked at once.
      rule: 'q' or 'expected_sarsa', with `learn_tabular()`'s meaning.
      seed, first_frame, reset_first, window: exactly as in `learn_tabular()`; the Philox counter
          is (absolute environment, frame >> 1, 1), the same stream.
      out: a dict from `shared_learner_buffers(P, T, window, path)`, overwritten.  With `out` (and
          tensors, or the same numbers as before, for the hyper-parameters) the call allocates
          nothing and is capturable in a HIP graph.
      path: 0 - a workgroup keeps the table, its learners' Q-tables and their accumulators in LDS
          whenever enough of them fit (library setting wide_lds_max), else Q-tables and
          accumulators are in global memory; 1 / 2 force either (1 raises ValueError when not even
          one learner fits).  Both give the same bits.

    Returns a dict: 'q'; 'reward_sum' float32, 'episodes' int32 and - games with hidden
    performance - 'perf_sum' int32, `[W, B]` each and PER ENVIRONMENT as `learn_tabular()` writes
    them (`.view(W, P, n)` gives a learner's curves); 'clamped' int64 `[P]`, written by the call:
    the TD errors of this call that were NaN (counted as 0) or beyond +-2^20 (counted as that).
    `state`, `done`, `ret` and `frame` carry over exactly as `learn_tabular()` leaves them.
    Argument errors raise ValueError before anything is launched.
    """
    S, A, B, dev = self.n_states, gamespec.N_ACTIONS, self.batch, self.device
    if (not torch.is_tensor(q) or q.dtype != torch.float32 or q.dim() != 3 or q.shape[0] < 1
        or tuple(q.shape[1:]) != (S, A) or q.device != dev or not q.is_contiguous()
        or q.data_ptr() % 16):
      got = ('{} {} on {}'.format(q.dtype, list(q.shape), q.device) if torch.is_tensor(q)
             else type(q).__name__)
      raise ValueError('q must be a contiguous, 16-byte aligned float32 [P, {}, {}] tensor (learners '
                       'x n_states x actions) on {}; got {}'.format(S, A, dev, got))
    P = int(q.shape[0])
    plan = self._shared_plan(P, path)
    own = [('clamped', torch.int64, (P,))]
    if plan[0] == 2:
      own.append(('scratch', torch.int32, (3 * P * S * A,)))
    T, window, first, seed, out, hyper = self._learner_prologue(
        'learn_shared', P, T, window, rule, first_frame, seed, alpha, gamma, epsilon, out, own,
        lambda T, window: 'shared_learner_buffers({}, {}, window={}, path={})'.format(P, T, window, path),
        lambda T, window: self.shared_learner_buffers(P, T, window, path))
    validate = self.validate_actions
    _hip.ops.wide_learn_shared(
        self._spec_host, self._tables, self.state, self.done, self.ret, q.detach(), hyper[0],
        hyper[1], hyper[2], _hip.LEARN_RULES[rule], seed, first, T, window, out['reward_sum'],
        out.get('perf_sum') if self.has_perf else None, out['episodes'], out['clamped'],
        out.get('scratch') if plan[0] == 2 else None,
        self._bad_shared_learners if validate else None, self._bad_flag if validate else None,
        bool(reset_first), path)
    return self._learner_epilogue(first, T, reset_first, q, out, ('clamped',))

  # ------------------------------------------------------------ shared actor-critic learners

  def _shared_actor_plan(self, P, path):
    """The six words of campx_wide_actor_shared_plan() for P learners of this game:
    `_shared_plan()`'s checks and messages, under this call's name."""
    return self._shared_plan(P, path, 'learn_actor_critic_shared()',
                             _hip.lib.campx_wide_actor_shared_plan,
                             'the preferences, values and accumulators')

  def shared_actor_buffers(self, P, T, window=None, path=0):
    """Allocate the dict of `learn_actor_critic_shared(out=...)` once, for P learners:
    `learner_buffers(T, window)`'s tensors, 'clamped' int64 [P] and - when a call with this `path`
    goes through global memory (path 2) - 'scratch', its accumulators: int32 [11 * P * n_states],
    zero, and left zero by every call."""
    plan = self._shared_actor_plan(P, path)
    out = self.learner_buffers(T, window)
    out['clamped'] = torch.zeros((P,), dtype=torch.int64, device=self.device)
    if plan[0] == 2:
      out['scratch'] = torch.zeros((11 * P * self.n_states,), dtype=torch.int32, device=self.device)
    return out

  def learn_actor_critic_shared(self, T, prefs, values, alpha_actor=0.1, alpha_critic=0.1, gamma=0.99,
                                seed=0, first_frame=None, reset_first=False, window=None, out=None,
                                path=0):
    """T frames of SYNCHRONOUS ADVANTAGE ACTOR-CRITIC (A2C) for P shared learners in ONE launch:
    learner m owns one softmax policy - the preferences `prefs[m]` - and one critic `values[m]`, and
    is fed by the n = B / P environments `[m * n, (m + 1) * n)`, `learn_shared()`'s and
    `rollout_population()`'s split of the batch (csrc/k_learn.hip,
    `campx::wide_learn_actor_shared`).  What otherwise takes `rollout_population()`, a returns pass,
    `sum_by_state()` and a torch step per update.

    Within a frame every actor of a learner samples from the same policy and bootstraps from the
    same critic - both as the frame found them - with `learn_actor_critic()`'s weights, sampler and
    stream, and computes `delta = (r if done else r + (gamma * D) * values[m, n]) - values[m, s]`.
    The errors are quantised to 64-bit fixed point (32 fractional bits) and summed per (state,
    action) as integers.  Each visited state then moves once: with `mean_k` the sum of action k's
    errors over the state's N visitors divided by N, and `mean_all` the same of all five,
    `values[m, s] += alpha_critic * mean_all` and
    `prefs[m, s, k] += alpha_actor * (mean_k - (w[k] / sum(w)) * mean_all)` - the mean over the
    visitors of the one-step actor-critic update.  The step size does not depend on n, and the run
    repeats bit for bit whatever the order in which environments arrive, the path or P
    (include/campx_hip.h has the rule in full; tests/shared_actor_reference.py restates it in numpy).
    n = 1 is NOT `learn_actor_critic()` bit for bit: the quantiser rounds the error to 2^-32 and the
    products are taken in another order.

    Args:
      prefs: contiguous float32 `[P, n_states, 5]` on the game's device (16-byte aligned,
          `P * n_states * 5 < 2^31`), updated IN PLACE; P is read from it.  P must divide the batch
          and 1 <= n = B / P <= 1024, the largest workgroup.  Rows that are not good - a NaN or a
          +inf, or five -inf - are treated as `learn_actor_critic()` treats them: an
          environment-frame that meets one takes action 4, contributes nothing and is counted; the
          count raises ValueError lazily.  `returns.softmax_weights(prefs)` is what
          `rollout_population()`, `evaluate_population()` and `visit_population()` take.
      values: contiguous float32 `[P, n_states]` (16-byte aligned), updated IN PLACE.
      alpha_actor, alpha_critic, gamma: each a Python number or a float32 `[P]` tensor - a tensor
          is a sweep.  A learner with one that is not finite is BAD: all its environments take
          action 4 at every frame, nothing of it changes, and it raises ValueError - counted once
          per learner and call - lazily.  Python numbers are checked at once.  With both step sizes
          0 the call walks exactly as `rollout_population(softmax_weights(prefs), T, seed,
          first_frame)` does.
      seed, first_frame, reset_first, window: exactly as in `learn_actor_critic()`; the Philox
          counter is (absolute environment, frame >> 2, 0), `rollout_policy()`'s stream.
      out: a dict from `shared_actor_buffers(P, T, window, path)`, overwritten.  With `out` (and
          tensors, or the same numbers as before, for the hyper-parameters) the call allocates
          nothing and is capturable in a HIP graph.
      path: 0 - a workgroup keeps the table and its learners' preferences, values and accumulators
          in LDS (68 bytes a state and learner) whenever enough of them fit (library setting
          wide_lds_max), else they are in global memory; 1 / 2 force either (1 raises ValueError
          when not even one learner fits).  Both give the same bits.

    Returns a dict: 'prefs', 'values'; 'reward_sum' float32, 'episodes' int32 and - games with
    hidden performance - 'perf_sum' int32, `[W, B]` each and PER ENVIRONMENT (`.view(W, P, n)` gives
    a learner's curves); 'clamped' int64 `[P]`, written by the call: the errors of this call that
    were NaN (counted as 0) or beyond +-2^20 (counted as that).  `state`, `done`, `ret` and `frame`
    carry over exactly as `learn_tabular()` leaves them.  Argument errors raise ValueError before
    anything is launched.

    NOT offered: an entropy bonus or a temperature, lambda-traces for the actor, REINFORCE with
    episode returns, n-step targets, and privatised accumulators.
    """
    S, A, B, dev = self.n_states, gamespec.N_ACTIONS, self.batch, self.device
    if (not torch.is_tensor(prefs) or prefs.dtype != torch.float32 or prefs.dim() != 3
        or prefs.shape[0] < 1 or tuple(prefs.shape[1:]) != (S, A) or prefs.device != dev
        or not prefs.is_contiguous() or prefs.data_ptr() % 16):
      got = ('{} {} on {}'.format(prefs.dtype, list(prefs.shape), prefs.device) if torch.is_tensor(prefs)
             else type(prefs).__name__)
      raise ValueError('prefs must be a contiguous, 16-byte aligned float32 [P, {}, {}] tensor '
                       '(learners x n_states x actions) on {}; got {}'.format(S, A, dev, got))
    P = int(prefs.shape[0])
    if not self._tensor_ok(values, torch.float32, (P, S)) or values.data_ptr() % 16:
      got = ('{} {} on {}'.format(values.dtype, list(values.shape), values.device)
             if torch.is_tensor(values) else type(values).__name__)
      raise ValueError('values must be a contiguous, 16-byte aligned float32 [{}, {}] tensor on {}; '
                       'got {}'.format(P, S, dev, got))
    plan = self._shared_actor_plan(P, path)
    own = [('clamped', torch.int64, (P,))]
    if plan[0] == 2:
      own.append(('scratch', torch.int32, (11 * P * S,)))
    T, window, first, seed, out, hyper = self._learner_prologue(
        'learn_actor_critic_shared', P, T, window, 'q', first_frame, seed, alpha_actor, gamma,
        alpha_critic, out, own,
        lambda T, window: 'shared_actor_buffers({}, {}, window={}, path={})'.format(P, T, window, path),
        lambda T, window: self.shared_actor_buffers(P, T, window, path),
        names=('alpha_actor', 'gamma', 'alpha_critic'))
    validate = self.validate_actions
    _hip.ops.wide_learn_actor_shared(
        self._spec_host, self._tables, self.state, self.done, self.ret, prefs.detach(),
        values.detach(), hyper[0], hyper[2], hyper[1], seed, first, T, window, out['reward_sum'],
        out.get('perf_sum') if self.has_perf else None, out['episodes'], out['clamped'],
        out.get('scratch') if plan[0] == 2 else None,
        self._bad_shared_actor_learners if validate else None,
        self._bad_shared_actor_rows if validate else None, self._bad_flag if validate else None,
        bool(reset_first), path)
    res = self._learner_epilogue(first, T, reset_first, prefs, out, ('clamped',))
    del res['q']
    res['prefs'], res['values'] = prefs, values
    return res

  # ------------------------------------------------------------ planning on the table

  def table_arrays(self):
    """The game's table - its complete, deterministic MDP - decoded from the blob the kernels
    walk, as device tensors `[n_states, 5]`, each entry as a rollout reports the frame that takes
    action a in state s: 'next_state' int32, 'reward' float32 (NaN = None), 'done' uint8,
    'discount' float32, 'perf' int8 (zeros for a game without hidden performance)."""
    S, A = self.n_states, gamespec.N_ACTIONS
    n = S * A
    entries = self._tables[:n * 8].view(torch.int32).view(S, A, 2)
    word = entries[..., 1]
    done = (word >> _hip.ENTRY_DONE_SHIFT) & 1
    code = ((word >> _hip.ENTRY_DCODE_SHIFT) & _hip.ENTRY_DCODE_MASK).long()
    listed = torch.tensor([float(x) for x in self.spec.discount_list], dtype=torch.float32,
                          device=self.device)
    plain = torch.where(done != 0, torch.zeros((), device=self.device),
                        torch.ones((), device=self.device))
    if self.has_perf:
      perf_off = (n * 8 + 15) // 16 * 16 + S * 16      # past the entries and the states' cells
      perf = self._tables[perf_off:perf_off + n].view(torch.int8).view(S, A).clone()
    else:
      perf = torch.zeros((S, A), dtype=torch.int8, device=self.device)
    return {'next_state': (word & _hip.ENTRY_NEXT_MASK).contiguous(),
            'reward': entries[..., 0].contiguous().view(torch.float32),
            'done': done.to(torch.uint8),
            'discount': torch.where(code != 0, listed[code], plain),
            'perf': perf}

  def _sweep_buffers(self, lead, sweeps, want_q):
    """What both dicts of buffers share; `lead`: the leading dimensions of a member's, () or (P,)."""
    S, dev = self.n_states, self.device
    out = {'values': torch.zeros(lead + (S,), dtype=torch.float32, device=dev),
           'residual': torch.zeros((int(sweeps),) + lead, dtype=torch.float32, device=dev),
           'scratch': torch.zeros(lead + (S,), dtype=torch.float32, device=dev)}
    if want_q:
      out['q'] = torch.zeros(lead + (S, gamespec.N_ACTIONS), dtype=torch.float32, device=dev)
    return out

  def sweep_buffers(self, sweeps, want_q=True, greedy=True):
    """Allocate the dict of `evaluate_policy(out=...)` (`greedy=False`) or
    `value_iteration(out=...)` once: 'values' float32 [S], 'residual' float32 [sweeps], 'scratch'
    float32 [S] (the second value vector of the one-launch-per-sweep path), with `want_q` 'q'
    float32 [S, 5] and with `greedy` 'greedy' int8 [S]."""
    out = self._sweep_buffers((), sweeps, want_q)
    if greedy:
      out['greedy'] = torch.zeros((self.n_states,), dtype=torch.int8, device=self.device)
    return out

  def _sweeps(self, P, policy, gamma, sweeps, values, reward, want_q, tol, check_every, out, path,
              rewards=None):
    """The body of `evaluate_policy()`, of `value_iteration()` (`policy` None) and - `P` not None,
    every per-member shape with that leading P - of `evaluate_population()` and of
    `value_iteration_population()` (`policy` None), their policy checked.  `rewards`: a reward
    table per member, a population's only."""
    S, A, dev = self.n_states, gamespec.N_ACTIONS, self.device
    greedy, members = policy is None, P is not None
    solve = members and (greedy or rewards is not None)     # campx::wide_population_solve's forms
    lead = (P,) if members else ()
    gammas = None
    if members and torch.is_tensor(gamma):
      if not self._tensor_ok(gamma, torch.float32, (P,)):
        raise ValueError('gamma must be a finite number or a contiguous float32 [{}] tensor (one per '
                         'member) on {}, got {} {} on {}'.format(P, dev, gamma.dtype, list(gamma.shape),
                                                                 gamma.device))
      gammas, gamma = gamma.detach(), 0.0
    elif (isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma)
          or abs(gamma) > torch.finfo(torch.float32).max):
      raise ValueError('gamma must be a finite number (as a float32){}, got {!r}'.format(
          ' or a float32 [{}] tensor'.format(P) if members else '', gamma))
    self._check_count('sweeps', sweeps)
    if values is not None and not self._tensor_ok(values, torch.float32, lead + (S,)):
      raise ValueError('values must be a contiguous float32 {} tensor ({}n_states) on {}, or '
                       'None for zeros'.format(list(lead + (S,)), 'members x ' if members else '', dev))
    if reward is not None and not self._tensor_ok(reward, torch.float32, (S, A)):
      raise ValueError('reward must be a contiguous float32 [{}, {}] tensor (n_states x actions) on '
                       '{}, or None for the table\'s own'.format(S, A, dev))
    if rewards is not None and reward is not None:
      raise ValueError('give rewards (one table per member) or reward (one for all members), not both')
    if rewards is not None and not self._tensor_ok(rewards, torch.float32, (P, S, A)):
      raise ValueError('rewards must be a contiguous float32 [{}, {}, {}] tensor (members x n_states x '
                       'actions) on {}, or None'.format(P, S, A, dev))
    if tol is not None and (isinstance(tol, bool) or not isinstance(tol, (int, float))
                            or not math.isfinite(tol) or tol < 0):
      raise ValueError('tol must be a finite number >= 0 or None, got {!r}'.format(tol))
    if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
      raise ValueError('check_every must be an int >= 1, got {!r}'.format(check_every))
    override = 0 if reward is None else 1
    if members:
      if self._n_cus is None:
        self._n_cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
      if solve:
        planned = self._planned_path(path, _hip.lib.campx_wide_population_solve_plan, P,
                                     0 if greedy else 1, 0 if rewards is None else 1,
                                     what='one member of {} states with its rewards'.format(S)
                                     if rewards is not None else None, n_cus=self._n_cus, words=5)
      else:
        planned = self._planned_path(path, _hip.lib.campx_wide_population_sweeps_plan, P, override,
                                     n_cus=self._n_cus, words=5)
    else:
      planned = self._planned_path(path, _hip.lib.campx_wide_sweeps_plan, 0 if greedy else 1, override)
    want = [('values', torch.float32, lead + (S,)), ('residual', torch.float32, (sweeps,) + lead)]
    if planned == 2:
      want.append(('scratch', torch.float32, lead + (S,)))
    if want_q:
      want.append(('q', torch.float32, lead + (S, A)))
    if greedy:
      want.append(('greedy', torch.int8, lead + (S,)))
    if out is None:
      out = (self.population_sweep_buffers(P, sweeps, want_q, greedy=greedy) if members
             else self.sweep_buffers(sweeps, want_q, greedy))
    else:
      self._check_out(out, want,
                      'population_sweep_buffers({}, {}, want_q={}{})'.format(
                          P, sweeps, bool(want_q), ', greedy=True' if greedy else '')
                      if members else
                      'sweep_buffers({}, want_q={}, greedy={})'.format(sweeps, bool(want_q), greedy))
      if values is not None and out.get('scratch') is not None and \
          values.data_ptr() == out['scratch'].data_ptr():
        raise ValueError('values must not be out[\'scratch\']')
    if reward is not None:
      reward = reward.detach()
    if rewards is not None:
      rewards = rewards.detach()
    v_out = out['values']
    if values is None:
      v_out.zero_()
      v_in = v_out
    else:
      v_in = values.detach()
    residual = out['residual']
    validate = self.validate_actions
    bad_rows = self._bad_population_rows if members else self._bad_plan_rows
    ran = 0
    while ran < sweeps:
      n = sweeps - ran if tol is None else min(check_every, sweeps - ran)
      count = validate and ran == 0 and not greedy        # bad rows: once per call
      head = (self._spec_host, self._tables, policy, reward, float(gamma))
      tail = (residual[ran:ran + n], bad_rows if count else None, self._bad_flag if count else None,
              path)
      q = out['q'] if want_q else None
      if solve:
        _hip.ops.wide_population_solve(self._spec_host, self._tables, policy, rewards, reward, float(gamma),
                                       gammas, v_in, v_out, out.get('scratch'), q,
                                       out['greedy'] if greedy else None, *tail)
      elif members:
        _hip.ops.wide_population_sweeps(*head, gammas, v_in, v_out, out.get('scratch'), q, *tail)
      else:
        _hip.ops.wide_sweeps(*head, v_in, v_out, out.get('scratch'), q,
                             out['greedy'] if greedy else None, *tail)
      ran += n
      v_in = v_out
      if tol is not None and bool((residual[ran - n:ran] <= tol).any()):     # (synchronises)
        break
    if validate:
      self._after_launch()
    res = {'values': v_out, 'residual': residual if ran == sweeps else residual[:ran], 'sweeps': ran}
    if want_q:
      res['q'] = out['q']
    if greedy:
      res['greedy'] = out['greedy']
    return res

  def evaluate_policy(self, policy, gamma, sweeps, values=None, reward=None, want_q=True, tol=None,
                      check_every=32, out=None, path=0):
    """The exact value of `policy` on the game's table: `sweeps` Jacobi sweeps of

        q[s, a] = r[s, a]                              if (s, a) ends the episode
                = r[s, a] + (gamma * D[s, a]) * v[next[s, a]]        otherwise
        v'[s]   = sum_a w[s, a] * q[s, a] / sum_a w[s, a]

    on the device (csrc/k_plan.hip, `campx::wide_sweeps`), where `rollout_policy()` can only sample
    it.  r, next and D - the frame's discount - are the table's, as `table_arrays()` shows them; a
    reward of None counts as 0.  float32 with every operation rounded on its own, sums in action
    order (include/campx_hip.h has the rule in full; tests/planning_reference.py restates it bit
    for bit), so the result does not depend on how the sweeps were run.

    Args:
      policy: what `rollout_policy()` takes, checked the same way: contiguous float32
          `[n_states, 5]` weights.  A bad row (a negative or NaN weight, a sum that is not a
          positive finite number) is evaluated as taking action 4 - as the sampler plays it - and
          raises ValueError with the count of such rows, lazily like bad actions: from
          `check_actions()` or a later call, under `validate_actions='sync'` from this one.
      gamma: the discount factor, a finite float.
      sweeps: how many sweeps to run, 1 .. 2^20.
      values: float32 `[n_states]` to start from, or None for zeros.  Running n sweeps and then m
          more from the 'values' of the first call equals n + m sweeps, bit for bit.
      reward: float32 `[n_states, 5]` to use instead of the table's rewards (NaN counts as 0):
          `table_arrays()['perf'].float()` gives a policy's exact hidden performance.
      want_q: also return 'q'.
      tol: None - the call never synchronises - or a residual to stop at: sweeps then run in blocks
          of `check_every`, the host reads each block's residuals once and stops after the first
          block that holds one <= tol.  The values are those of a plain call of 'sweeps' sweeps.
      out: a dict from `sweep_buffers(sweeps, want_q, greedy=False)`, overwritten; with `out` and
          `tol=None` the call allocates nothing and is capturable in a HIP graph.
      path: 0 - all sweeps in one launch by one workgroup that holds the table in LDS whenever it
          fits there, else one launch per sweep; 1 / 2 force either (1 raises ValueError for a
          table that does not fit).  Every path gives the same bits.

    Returns a dict: 'values' float32 `[n_states]`; 'q' float32 `[n_states, 5]` (with `want_q`) -
    the backup of the last sweep, so that 'values' is exactly its reduction; 'residual' float32
    `[sweeps run]`, per sweep the largest |v_k[s] - v_{k-1}[s]| (NaN if any difference is);
    'sweeps' int, the sweeps run.  Argument errors raise ValueError before anything is launched.
    """
    self._check_policy(policy)
    return self._sweeps(None, policy.detach(), gamma, sweeps, values, reward, want_q,
                        tol, check_every, out, path)

  def value_iteration(self, gamma, sweeps, values=None, reward=None, want_q=True, tol=None,
                      check_every=32, out=None, path=0):
    """`sweeps` sweeps of value iteration on the game's table: `evaluate_policy()` with
    `v'[s] = max_a q[s, a]` in place of the policy's average.  Same arguments (`out` from
    `sweep_buffers(sweeps, want_q)`), same result plus 'greedy' int8 `[n_states]`: per state the
    lowest action that attains the maximum of the returned q.  A one-hot policy built from it -
    `torch.nn.functional.one_hot(res['greedy'].long(), 5).float()` - is what `rollout_policy()`
    and `evaluate_policy()` take."""
    return self._sweeps(None, None, gamma, sweeps, values, reward, want_q, tol,
                        check_every, out, path)

  # ------------------------------------------------------------ planning for a population

  POPULATION_MAX_ELEMENTS = (1 << 31) - 1      # P * n_states * 5 of evaluate_population()

  def _check_members(self, P, call='evaluate_population', verb='evaluate'):
    S, A = self.n_states, gamespec.N_ACTIONS
    if isinstance(P, bool) or not isinstance(P, int) or P < 1:
      raise ValueError('P must be an int >= 1, got {!r}'.format(P))
    if P * S * A > self.POPULATION_MAX_ELEMENTS:
      raise ValueError('{}(): P * n_states * 5 = {} x {} x 5 must be at most '
                       '2^31 - 1; {} the population in parts'.format(call, P, S, verb))

  def population_sweep_buffers(self, P, sweeps, want_q=False, greedy=False):
    """Allocate the dict of `evaluate_population(out=...)` or - `greedy=True` - of
    `value_iteration_population(out=...)` once: 'values' float32 [P, S], 'residual'
    float32 [sweeps, P], 'scratch' float32 [P, S] (the second value array of the
    one-launch-per-sweep path), 'gamma' float32 [P] (for the caller to fill and pass as `gamma`; a
    number needs none), with `want_q` 'q' float32 [P, S, 5] and with `greedy` 'greedy' int8 [P, S]
    and 'rewards' float32 [P, S, 5] (for the caller to fill and pass as `rewards`; neither call
    reads it from here)."""
    self._check_members(P)
    self._check_count('sweeps', sweeps)
    out = self._sweep_buffers((P,), sweeps, want_q)
    out['gamma'] = torch.zeros((P,), dtype=torch.float32, device=self.device)
    if greedy:
      out['greedy'] = torch.zeros((P, self.n_states), dtype=torch.int8, device=self.device)
      out['rewards'] = torch.zeros((P, self.n_states, gamespec.N_ACTIONS), dtype=torch.float32,
                                   device=self.device)
    return out

  def evaluate_population(self, policies, gamma, sweeps, values=None, reward=None, want_q=False,
                          out=None, path=0, rewards=None):
    """`evaluate_policy()` for a POPULATION of P policies in one launch: member m of every result
    is, bit for bit, `evaluate_policy(policies[m], gamma[m], sweeps, ...)` - the exact score that
    population-based training, an evolution strategy, a sweep over gammas or a set of seeds selects
    on, without a launch per member (csrc/k_plan.hip, `campx::wide_population_sweeps`).  The rule is
    `evaluate_policy()`'s and is stated there; no result depends on P, on the order of the members
    or on the path.

    Args:
      policies: what `rollout_population()` takes, checked by the same helper - contiguous float32
          `[P, n_states, 5]` on the game's device - except that P need not divide the batch;
          `P * n_states * 5 <= 2^31 - 1`.  Bad rows are evaluated as taking action 4 and raise
          ValueError with their count, summed over the members, lazily as `evaluate_policy()`'s do,
          in a message that names this call.
      gamma: a finite number for every member, or a contiguous float32 `[P]` tensor on the game's
          device, one factor per member.  A tensor is NEVER read on the host: a NaN or an infinity
          in it is not refused, it propagates through `gamma * D` as the f32 rule says (the
          member's values come out NaN wherever the product is used).
      sweeps: how many sweeps to run, 1 .. 2^20.  There is no `tol`: stopping per member would
          need a host read; 'residual' is there for the caller to read where it matters.
      values: float32 `[P, n_states]` to start from, or None for zeros.  n sweeps and then m more
          from the returned 'values' equal n + m sweeps, bit for bit.
      reward: float32 `[n_states, 5]` used instead of the table's rewards by ALL members.
      rewards: contiguous float32 `[P, n_states, 5]`, a reward table PER MEMBER (NaN counts as 0):
          member m is then `evaluate_policy(policies[m], gamma[m], sweeps, reward=rewards[m])`, bit
          for bit (`campx::wide_population_solve`).  Not beside `reward`.  One policy under P
          rewards - its successor representation from S one-hot rewards, its reward value and its
          hidden performance together - is no form of its own:
          `policies = policy.expand(P, -1, -1).contiguous()` serves.  P equal rows give the bits of
          the shared `reward=` call.
      want_q: also return 'q'.
      out: a dict from `population_sweep_buffers(P, sweeps, want_q)`, overwritten; the call then
          allocates nothing and is capturable in a HIP graph ('scratch' is needed on path 2 only,
          'gamma' never).
      path: 0 - a workgroup keeps the table and several members' vectors in LDS and runs all
          sweeps in the one launch whenever one member fits there (library setting wide_lds_max),
          else one launch per sweep for all members; 1 / 2 force either (1 raises ValueError for a
          table that does not fit).  Both give the same bits.

    Returns a dict: 'values' float32 `[P, n_states]` - `[:, 0]` is each member's value of the state
    an episode starts from -; 'residual' float32 `[sweeps, P]`; 'sweeps'; with `want_q` 'q' float32
    `[P, n_states, 5]`.  Argument errors raise ValueError before anything is launched.
    """
    P = self._check_population(policies, split=False)
    self._check_members(P)
    return self._sweeps(P, policies.detach(), gamma, sweeps, values, reward, want_q, None, 32, out, path,
                        rewards=rewards)

  def value_iteration_population(self, gamma, sweeps, rewards=None, P=None, values=None, want_q=False,
                                 out=None, path=0):
    """`value_iteration()` for a POPULATION of P rewards or gammas in one launch: member m of every
    result is, bit for bit, `value_iteration(gamma[m], sweeps, values=values[m], reward=rewards[m])`
    - 'values', 'q', 'greedy' and every 'residual' - without a launch per member (csrc/k_plan.hip,
    `campx::wide_population_solve`).  It is what a reward-design question asks: which of P rewards
    - a sweep of `r + lambda * perf`, shaping terms, the candidates of an inverse-RL step - or
    which of P gammas makes the reward-optimal policy good.  The rule is `evaluate_policy()`'s with
    the greedy reduction; no result depends on P, on the order of the members, on how members are
    packed into workgroups or on the path.

    Args:
      gamma: a finite number for every member, or a contiguous float32 `[P]` tensor on the game's
          device.  A tensor is NEVER read on the host, as in `evaluate_population()`.
      sweeps: how many sweeps to run, 1 .. 2^20.  There is no `tol`, for `evaluate_population()`'s
          reason.
      rewards: contiguous float32 `[P, n_states, 5]` on the game's device, a reward table per
          member (NaN counts as 0), or None: the table's own rewards for every member.
      P: the members, where neither `rewards` nor a `gamma` tensor says it.  What is given must
          agree; `P * n_states * 5 <= 2^31 - 1`.  With none of the three there is no population:
          ValueError, `value_iteration()` is the call.
      values: float32 `[P, n_states]` to start from, or None for zeros.  n sweeps and then m more
          from the returned 'values' equal n + m sweeps, bit for bit.
      want_q: also return 'q'.
      out: a dict from `population_sweep_buffers(P, sweeps, want_q, greedy=True)`, overwritten; the
          call then allocates nothing and is capturable in a HIP graph ('scratch' is needed on path
          2 only, 'gamma' and 'rewards' never).
      path: as `evaluate_population()`'s; whether one member fits LDS depends on the form - its
          rewards take 20 bytes a state there.  Both give the same bits.

    Returns a dict: 'values' float32 `[P, n_states]`; 'greedy' int8 `[P, n_states]`, per member and
    state the lowest action that attains the maximum of the returned q; 'residual' float32
    `[sweeps, P]`; 'sweeps'; with `want_q` 'q' float32 `[P, n_states, 5]`.  Argument errors raise
    ValueError before anything is launched.
    """
    said = []
    if rewards is not None:
      if not torch.is_tensor(rewards) or rewards.dim() != 3 or rewards.shape[0] < 1:
        raise ValueError('rewards must be a contiguous float32 [P, {}, {}] tensor (members x n_states x '
                         'actions) on {}, or None'.format(self.n_states, gamespec.N_ACTIONS, self.device))
      said.append(('rewards', int(rewards.shape[0])))
    if torch.is_tensor(gamma) and gamma.dim() == 1:
      said.append(('gamma', int(gamma.shape[0])))
    if P is not None:
      if isinstance(P, bool) or not isinstance(P, int):
        raise ValueError('P must be an int >= 1 or None, got {!r}'.format(P))
      said.append(('P', P))
    if not said:
      raise ValueError('value_iteration_population(): nothing says how many members there are (rewards, '
                       'a gamma tensor or P); value_iteration() is the call for one reward and one gamma')
    if any(n != said[0][1] for _, n in said[1:]):
      raise ValueError('value_iteration_population(): the members disagree: {}'.format(
          ', '.join('{} says {}'.format(k, n) for k, n in said)))
    P = said[0][1]
    self._check_members(P, call='value_iteration_population', verb='solve')
    return self._sweeps(P, None, gamma, sweeps, values, None, want_q, None, 32, out, path, rewards=rewards)

  # ------------------------------------------------------------ exact visitation on the table

  VISIT_UNIT = 1 << 38             # one environment, in the int64 units of state_visitation()

  def visitation_buffers(self, frames, want_frames=False):
    """Allocate the dict of `state_visitation(out=...)` once: 'visits' int64 [S, 5], 'finished'
    int64 [frames], 'final' int64 [S], 'counts' int32 [S, 5], 'scratch' int64 [S] (the second mass
    vector of the one-launch-per-frame path) and - `want_frames` - 'per_frame' int64
    [frames + 1, S]."""
    return self._visit_buffers((), int(frames), want_frames)

  def _visit_buffers(self, lead, frames, want_frames):
    """What both dicts of buffers share; `lead`: the leading dimensions of a member's, () or (P,)."""
    S, A, dev = self.n_states, gamespec.N_ACTIONS, self.device
    out = {'visits': torch.zeros(lead + (S, A), dtype=torch.int64, device=dev),
           'finished': torch.zeros((frames,) + lead, dtype=torch.int64, device=dev),
           'final': torch.zeros(lead + (S,), dtype=torch.int64, device=dev),
           'counts': torch.zeros(lead + (S, A), dtype=torch.int32, device=dev),
           'scratch': torch.zeros(lead + (S,), dtype=torch.int64, device=dev)}
    if want_frames:
      out['per_frame'] = torch.zeros((frames + 1,) + lead + (S,), dtype=torch.int64, device=dev)
    return out

  def state_visitation(self, policy, frames, start=None, restart=True, want_frames=False, out=None,
                       path=0):
    """The exact visitation of `policy` on the game's table: how much probability sits in each
    state at each of `frames` frames, and how often each (state, action) is taken - what
    `rollout_policy()` followed by `returns.sum_by_state()` estimates with sampling noise, computed
    from the table on the device (csrc/k_visit.hip, `campx::wide_visit`).

    Mass is an int64 in units of 2^-38: one environment is 'unit' = 2^38.  Per state the sampler's
    2^24 equally likely values are counted into the five actions exactly as `rollout_policy()`
    plays them ('counts'); a state's mass m goes to its actions as `floor(m * N / 2^24)`
    differences, which sum to m to the last unit; an action's share moves to the entry's next state
    or - an entry that ends the episode - is counted into 'finished' and, with `restart`, moves to
    state 0 as a rollout's environment does.  Only integers are added, so the result does not
    depend on how the kernels ran (include/campx_hip.h has the rule in full;
    tests/visitation_reference.py restates it bit for bit).

    Args:
      policy: what `rollout_policy()` takes, checked the same way: contiguous float32
          `[n_states, 5]` weights.  A bad row (a negative or NaN weight, a sum that is not a
          positive finite number) sends all its mass to action 4 - as the sampler plays it - and
          raises ValueError with the count of such rows, lazily like `evaluate_policy()`'s: from
          `check_actions()` or a later call, under `validate_actions='sync'` from this one.
      frames: how many frames to run, 1 .. 2^20.
      start: where the mass starts.  None: one environment in state 0.  An int64 `[n_states]`
          tensor in units - every entry >= 0, the total at most 2^38 -, typically the 'final' of an
          earlier call: n frames and then m more from it equal n + m frames bit for bit, 'visits'
          and 'finished' adding up.  A float tensor `[n_states]` of probabilities - finite, >= 0,
          summing to 1 within 1e-4 - is quantised HERE, not by the kernels: every entry times 2^38
          rounded down, the units that are then missing from 2^38 given to the largest entry, so
          that the total is exactly 2^38.  `start` is validated eagerly (a few synchronising
          reads: this call is planning, not a hot loop).
      restart: True - mass whose episode ends starts over in state 0, the total stays put, as in a
          rollout of fixed length; False - it leaves, and 'finished' is what left at each frame.
      want_frames: also return 'per_frame'.
      out: a dict from `visitation_buffers(frames, want_frames)`, overwritten; 'final' may be the
          `start` of the call.
      path: 0 - all frames in one launch by one workgroup that holds the table in LDS whenever it
          fits there, else one launch per frame; 1 / 2 force either (1 raises ValueError for a
          table that does not fit).  Every path gives the same bits.

    Returns a dict: 'visits' int64 `[n_states, 5]`, the mass that took action a in state s, summed
    over the frames (`B * visits / 2^38` is the expectation of `sum_by_state()`'s count for B
    environments); 'finished' int64 `[frames]`, the mass whose episode ended at each frame; 'final'
    int64 `[n_states]`, the mass per state after the last frame; 'per_frame' int64
    `[frames + 1, n_states]` (with `want_frames`), the mass per state before each frame and after
    the last; 'counts' int32 `[n_states, 5]`, rows summing to 2^24; 'probs' float64
    `[n_states, 5]` = counts / 2^24, the exact probability with which `rollout_policy()` takes a
    in s - what `log pi` should be built from; 'unit' = 2^38.  Argument errors raise ValueError
    before anything is launched.
    """
    self._check_policy(policy)
    return self._visit(None, policy, frames, start, restart, want_frames, out, path)

  def _visit(self, P, policy, frames, start, restart, want_frames, out, path):
    """The body of `state_visitation()` and - `P` not None, every per-member shape with that
    leading P, a `start` per member or shared - of `visit_population()`, their policy checked."""
    S, A, dev = self.n_states, gamespec.N_ACTIONS, self.device
    members = P is not None
    lead = (P,) if members else ()
    per_member = ' per member' if members else ''
    unit = self.VISIT_UNIT
    self._check_count('frames', frames)
    if members:
      if want_frames:
        self._check_frame_elements(P, frames)
      if self._n_cus is None:
        self._n_cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
      planned = self._planned_path(path, _hip.lib.campx_wide_visit_population_plan, P, n_cus=self._n_cus,
                                   words=5)
    else:
      planned = self._planned_path(path, _hip.lib.campx_wide_visit_plan)
    if start is not None:
      if (not torch.is_tensor(start) or tuple(start.shape) not in ((S,), lead + (S,)) or start.device != dev
          or not (start.dtype == torch.int64 or start.is_floating_point())):
        if members:
          raise ValueError('start must be None, an int64 tensor of units of 2^-38 or a float tensor of '
                           'probabilities, [{0}, {1}] (per member) or [{1}] (shared), on {2}'.format(P, S, dev))
        raise ValueError('start must be None, an int64 [{0}] tensor of units of 2^-38 or a float '
                         '[{0}] tensor of probabilities, on {1}'.format(S, dev))
      start = start.detach()
      # row by row: a single call's [S] and a shared start are one row
      if start.dtype == torch.int64:
        if not start.is_contiguous():
          raise ValueError('an int64 start must be contiguous')
        totals = start.sum(-1)                   # (one row: its total, and no launch to find the largest)
        if (bool((start < 0).any()) or int(totals.max() if totals.dim() else totals) > unit
            or int(start.max()) > unit):
          raise ValueError('an int64 start must hold entries >= 0 that total at most 2^38' + per_member)
      else:
        p = start.double()
        if (not bool(torch.isfinite(p).all()) or bool((p < 0).any())
            or float((p.sum(-1) - 1.0).abs().max()) > 1e-4):
          raise ValueError('a float start must hold finite probabilities >= 0 that sum to 1 (within '
                           '1e-4)' + per_member)
        rows = p.reshape(-1, S)
        units = torch.floor(rows * float(unit)).long()
        largest = torch.argmax(rows, dim=1, keepdim=True)
        units.scatter_add_(1, largest, (unit - units.sum(1, keepdim=True)))
        if bool((units.gather(1, largest) < 0).any()):
          raise ValueError('a float start sums to more than 1 by more than its largest entry')
        start = units.reshape(p.shape).contiguous()
    want = [('visits', torch.int64, lead + (S, A)), ('finished', torch.int64, (frames,) + lead),
            ('final', torch.int64, lead + (S,)), ('counts', torch.int32, lead + (S, A))]
    if members:
      want.append(('probs', torch.float64, lead + (S, A)))
    if planned == 2:
      want.append(('scratch', torch.int64, lead + (S,)))
    if want_frames:
      want.append(('per_frame', torch.int64, (frames + 1,) + lead + (S,)))
    given = out is not None
    if not given:
      out = (self.visit_population_buffers(P, frames, want_frames) if members
             else self.visitation_buffers(frames, want_frames))
    else:
      self._check_out(out, want,
                      'visit_population_buffers({}, {}, want_frames={})'.format(P, frames, bool(want_frames))
                      if members else
                      'visitation_buffers({}, want_frames={})'.format(frames, bool(want_frames)))
    scratch = out.get('scratch')
    if members and start is not None:
      if scratch is not None and self._shares_bytes(start, scratch):
        raise ValueError('start must not be out[\'scratch\']')
      in_place = start.dim() == 2 and start.data_ptr() == out['final'].data_ptr()
      if not in_place and self._shares_bytes(start, out['final']):
        raise ValueError('start must not overlap out[\'final\'] (a [P, n_states] start may BE it)')
    elif given and start is not None and scratch is not None and start.data_ptr() == scratch.data_ptr():
      raise ValueError('start must not be out[\'scratch\']')
    validate = self.validate_actions
    bad_rows = self._bad_visit_member_rows if members else self._bad_visit_rows
    (_hip.ops.wide_visit_population if members else _hip.ops.wide_visit)(
        self._spec_host, self._tables, policy.detach(), start, bool(restart), out['visits'],
        out['finished'], out['final'], out['per_frame'] if want_frames else None, out['counts'],
        scratch, bad_rows if validate else None, self._bad_flag if validate else None, path)
    if validate:
      self._after_launch()
    if members:
      probs = out['probs']
      probs.copy_(out['counts'])
      probs.mul_(1.0 / float(1 << 24))
    else:
      probs = out['counts'].double() / float(1 << 24)
    res = {'visits': out['visits'], 'finished': out['finished'], 'final': out['final'],
           'counts': out['counts'], 'probs': probs, 'unit': unit}
    if want_frames:
      res['per_frame'] = out['per_frame']
    return res

  # ------------------------------------------------------------ exact visitation of a population

  VISIT_MAX_FRAME_ELEMENTS = (1 << 31) - 1     # (frames + 1) * P * n_states of visit_population()'s 'per_frame'

  def _check_frame_elements(self, P, frames):
    if (frames + 1) * P * self.n_states > self.VISIT_MAX_FRAME_ELEMENTS:
      raise ValueError('visit_population(): (frames + 1) * P * n_states = {} x {} x {} must be at most '
                       '2^31 - 1 with want_frames; split the frames or the population over several '
                       'calls'.format(frames + 1, P, self.n_states))

  def visit_population_buffers(self, P, frames, want_frames=False):
    """Allocate the dict of `visit_population(out=...)` once: 'visits' int64 [P, S, 5], 'finished'
    int64 [frames, P], 'final' int64 [P, S], 'counts' int32 [P, S, 5], 'probs' float64 [P, S, 5],
    'scratch' int64 [P, S] (the second mass array of the one-launch-per-frame path) and -
    `want_frames` - 'per_frame' int64 [frames + 1, P, S]."""
    self._check_members(P, 'visit_population', 'visit')
    self._check_count('frames', frames)
    if want_frames:
      self._check_frame_elements(P, frames)
    out = self._visit_buffers((P,), frames, want_frames)
    out['probs'] = torch.zeros((P, self.n_states, gamespec.N_ACTIONS), dtype=torch.float64,
                               device=self.device)
    return out

  def visit_population(self, policies, frames, start=None, restart=True, want_frames=False, out=None,
                       path=0):
    """`state_visitation()` for a POPULATION of P policies in one launch: member m of every result
    is, bit for bit, `state_visitation(policies[m], frames, start_m, restart)` - the forward half
    of the exact policy gradient for every member of a population, a sweep of learning rates or a
    set of seeds, without a launch per member (csrc/k_visit.hip, `campx::wide_visit_population`).
    The rule is `state_visitation()`'s and is stated there; no result depends on P, on the order of
    the members or on the path.

    Args:
      policies: what `evaluate_population()` takes, checked by the same helpers - contiguous
          float32 `[P, n_states, 5]` on the game's device, P need not divide the batch,
          `P * n_states * 5 <= 2^31 - 1`.  A bad row sends all its mass to action 4 and raises
          ValueError with the count of such rows, summed over the members, lazily as
          `state_visitation()`'s do, in a message that names this call.
      frames: how many frames to run, 1 .. 2^20.
      start: where the mass starts.  None: one environment in state 0 for every member.
          `[P, n_states]`: member m starts from row m; `[n_states]`: every member starts from it.
          int64 units - contiguous, every entry >= 0, each member's total at most 2^38 - or float
          probabilities, quantised HERE row by row exactly as `state_visitation()` quantises its
          float `start`.  Validated eagerly, with a few synchronising reads; `start=None` reads
          nothing.  An int64 `[P, n_states]` start may BE `out['final']`: the call then continues
          in place.  A shared `[n_states]` start must not overlap 'final', and no start may be
          `out['scratch']`.
      restart, want_frames: as in `state_visitation()`.  With `want_frames`,
          `(frames + 1) * P * n_states <= 2^31 - 1`; split a larger call.
      out: a dict from `visit_population_buffers(P, frames, want_frames)`, overwritten; with it
          (and `start` None or already int64) the call allocates nothing, and it synchronises only
          to validate a `start` ('scratch' is needed on path 2 only).
      path: 0 - a workgroup keeps the table and several members' vectors in LDS and runs all
          frames in the one launch whenever one member fits there (exactly the tables that fit
          `state_visitation()`'s LDS path), else one launch per frame for all members; 1 / 2 force
          either (1 raises ValueError for a table that does not fit).  Both give the same bits.

    Returns a dict, time-major where there is a frame axis: 'visits' int64 `[P, n_states, 5]`;
    'finished' int64 `[frames, P]`; 'final' int64 `[P, n_states]`; 'counts' int32
    `[P, n_states, 5]`; 'probs' float64 `[P, n_states, 5]` = counts / 2^24; 'unit' = 2^38; with
    `want_frames` 'per_frame' int64 `[frames + 1, P, n_states]`.  Argument errors raise ValueError
    before anything is launched.
    """
    P = self._check_population(policies, split=False)
    self._check_members(P, 'visit_population', 'visit')
    return self._visit(P, policies, frames, start, restart, want_frames, out, path)

  @staticmethod
  def _shares_bytes(a, b):
    """Two contiguous tensors share a byte."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()

  # ------------------------------------------------------------ observations by state

  def render_states(self, state_ids=None, obs_dtype=torch.int8, out=None):
    """The observations of states of the game's table, `[N, L, H, W]`: what a network that is
    evaluated once per state - the policy of `rollout_policy()`, a critic - is evaluated on.

    Row i is bit for bit the observation `play()` / `rollout()` show for an environment that is
    in state `state_ids[i]`.  State 0 is the reset state: row 0 of `render_states()` is the
    `its_showtime()` frame.  With `out = rollout_policy(...)`, `render_states(out['states'][t])`
    are the observations frame t's actions were sampled from, and `render_states(game.state)`
    the ones the rollout ended in.

    Args:
      state_ids: int32 or int64 `[N]` on the game's device, N >= 1; None: all states,
          `arange(n_states)`.  Ids outside `[0, n_states)` are rendered as state 0 and counted on
          the device; like bad actions they raise ValueError lazily - from a later call, or from
          `check_actions()` - because this call does not synchronise.
      obs_dtype: torch.int8 (0 / 1), torch.float16 or torch.bfloat16 (0.0 / 1.0).
      out: a contiguous `[N, L, H, W]` tensor of such a dtype to write into.  The call is then
          capturable in a HIP graph (no allocation, no host synchronisation: its scratch is kept
          with the game).
    """
    L, H, W = self.n_layers, self.rows, self.cols
    ids, N = self._check_state_ids(state_ids)
    scratch = None
    if out is None:
      if obs_dtype not in fused._OBS_DTYPES:
        raise ValueError('obs_dtype must be torch.int8, float16 or bfloat16')
      out = torch.empty((N, L, H, W), dtype=obs_dtype, device=self.device)
    else:
      if (not torch.is_tensor(out) or tuple(out.shape) != (N, L, H, W)
          or out.dtype not in fused._OBS_DTYPES or not out.is_contiguous()
          or out.device != self.device):
        raise ValueError('out must be a contiguous int8 / float16 / bfloat16 [{}, {}, {}, {}] tensor '
                         'on {}'.format(N, L, H, W, self.device))
      need = int(_hip.lib.campx_wide_render_states_scratch_bytes(ctypes.byref(self.spec), N))
      if not self._states_scratch or self._states_scratch[-1].numel() < need:
        self._states_scratch.append(torch.empty((need,), dtype=torch.uint8, device=self.device))
      scratch = self._states_scratch[-1]
    _hip.ops.wide_render_states(self._spec_host, self._tables, ids, out, scratch,
                                self._bad_state_ids, self._bad_idx_flag)
    self._after_index_launch()
    return out

  # ------------------------------------------------------------ observation windows

  def _window_table(self):
    """uint8 [variants, 1024] on the device: the scenery's layer per cell of each variant, from
    the host arrays the game keeps (the table blob is not touched).  The scenery's row is one-hot
    per cell - campx_wide_tables_build() sets exactly the byte of this layer - so the layer is all
    the window kernel needs of it."""
    if self._layer_of_cell is None:
      import numpy as np
      HW = self.rows * self.cols
      tops = self._arrays.get('variant_top_layer')
      if self.spec.n_variants > 1 and tops is not None:
        tops = np.asarray(tops, np.uint8).reshape(int(self.spec.n_variants), HW)
      else:
        tops = np.frombuffer(bytes(bytearray(self.spec.static_top_layer)), np.uint8)[:HW].reshape(1, HW)
      table = np.zeros((tops.shape[0], 1024), np.uint8)
      table[:, :HW] = tops
      self._layer_of_cell = torch.from_numpy(table).to(self.device)
    return self._layer_of_cell

  def _windows(self, method, source, window, trace, t_idx, e_idx, shape, obs_dtype, out):
    from . import windows
    if not isinstance(window, windows.Window):
      raise ValueError('{}(): window must be a campx_amd.windows.Window, got {}'.format(
          method, type(window).__name__))
    where = window.resolve(self.chars, self.spec)
    shape = tuple(shape) + (self.n_layers, window.height, window.width)
    rows = 1
    for n in shape[:-3]:
      rows *= n
    if rows * self.n_layers * window.height * window.width > (1 << 32) - 65536 - 1:
      raise ValueError('{}(): {} rows of {} x {} x {} elements are past what one call addresses '
                       '(2^32 - 65536 - 1 elements): split the request'.format(
                           method, rows, self.n_layers, window.height, window.width))
    if out is None:
      if obs_dtype not in fused._OBS_DTYPES:
        raise ValueError('obs_dtype must be torch.int8, float16 or bfloat16')
      out = torch.empty(shape, dtype=obs_dtype, device=self.device)
    elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype not in fused._OBS_DTYPES
          or not out.is_contiguous() or out.device != self.device):
      raise ValueError('out must be a contiguous int8 / float16 / bfloat16 {} tensor on {}'.format(
          list(shape), self.device))
    _hip.ops.wide_render_windows(
        self._spec_host, self._tables, self._window_table(), source, trace, t_idx, e_idx, out,
        window.height, window.width, where.thing, where.r0, where.c0, where.pad_layer,
        self._bad_window_ids if source == _hip.WINDOWS_STATES else self._bad_window_rows,
        self._bad_idx_flag, fused.GATHER_STREAMING)
    self._after_index_launch()
    return out

  def _check_window_trace(self, trace):
    planes = self._n_planes
    if (not torch.is_tensor(trace) or trace.dim() != 3 or trace.dtype != torch.int16
        or trace.shape[0] != planes or trace.shape[2] != self.batch or trace.device != self.device):
      raise ValueError('trace must be a {} [{}, T, {}] tensor of this game on {}'.format(
          torch.int16, planes, self.batch, self.device))

  def render_frame_windows(self, trace, t_idx, e_idx, window, obs_dtype=torch.int8, out=None):
    """Windows of the observations of sampled transitions, `[N, L, h, w]`: `render_frames()`
    cropped to what `window` shows, without the full observations being written.

    Row i is bit for bit `render_frames(trace, t_idx, e_idx)[i]` cut to the `h x w` cells whose
    top-left cell is `(row - h // 2, col - w // 2)` of the tracked thing's cell in that frame -
    or the window's fixed corner -, with cells off the board 0, or 1 in the layer of the window's
    `pad` character (include/campx_hip.h has the rule; `campx_amd.windows.Window`).  A thing that
    is hidden still centres its window where its trace entry says it is.

    Args:
      trace, t_idx, e_idx: as for `render_frames()`; indices outside the trace are clamped on the
          device, counted, and raise ValueError lazily - from a later call or `check_actions()` -
          in a message that names this call.
      window: a `campx_amd.windows.Window`.
      obs_dtype: torch.int8 (0 / 1), torch.float16 or torch.bfloat16 (0.0 / 1.0).
      out: a contiguous `[N, L, h, w]` tensor of such a dtype to write into.  The call then
          allocates nothing and does not synchronise: it is capturable in a HIP graph.
    """
    self._check_window_trace(trace)
    t_idx, e_idx = torch.as_tensor(t_idx), torch.as_tensor(e_idx)
    if t_idx.dim() != 1 or t_idx.shape != e_idx.shape or t_idx.numel() < 1:
      raise ValueError('t_idx and e_idx must be integer tensors [N] of one length N >= 1')
    if t_idx.dtype not in (torch.int32, torch.int64) or e_idx.dtype != t_idx.dtype:
      raise ValueError('t_idx and e_idx must both be int64 or both int32')
    t_idx = t_idx.to(self.device).contiguous()
    e_idx = e_idx.to(self.device).contiguous()
    return self._windows('render_frame_windows', _hip.WINDOWS_PAIRS, window, trace, t_idx, e_idx,
                         (int(t_idx.numel()),), obs_dtype, out)

  def render_trace_windows(self, trace, window, obs_dtype=torch.int8, out=None):
    """Windows of EVERY frame of a trace, `[T, B, L, h, w]`: `render_frame_windows()` of
    `(t, e)` for all t and e, without index tensors.  `trace` may be a view of a padded buffer, as
    `rollout_policy()` returns it.  `out`: a contiguous `[T, B, L, h, w]` tensor to write into
    (the call is then capturable in a HIP graph)."""
    self._check_window_trace(trace)
    return self._windows('render_trace_windows', _hip.WINDOWS_TRACE, window, trace, None, None,
                         (int(trace.shape[1]), self.batch), obs_dtype, out)

  def render_state_windows(self, window, state_ids=None, obs_dtype=torch.int8, out=None):
    """Windows of the observations of states of the game's table, `[N, L, h, w]`:
    `render_states()` cropped to what `window` shows.  The window round the agent is a function of
    the state, so a network that sees only the window is still a per-state table: evaluate it on
    `render_state_windows(window)` once and hand the result to `rollout_policy()`.

    Row i is bit for bit the window of `render_states(state_ids)[i]`; the states' entries are
    read from the table directly, no scratch trace is kept.  Row 0 of all states is the window of
    the `its_showtime()` frame.

    Args:
      window: a `campx_amd.windows.Window`.
      state_ids: int32 or int64 `[N]` on the game's device, N >= 1; None: all states.  Ids outside
          `[0, n_states)` are rendered as state 0, counted, and raise ValueError lazily, in a
          message that names this call.
      obs_dtype: torch.int8 (0 / 1), torch.float16 or torch.bfloat16 (0.0 / 1.0).
      out: a contiguous `[N, L, h, w]` tensor of such a dtype to write into (no allocation, no
          synchronisation: capturable in a HIP graph).
    """
    ids, N = self._check_state_ids(state_ids)
    return self._windows('render_state_windows', _hip.WINDOWS_STATES, window, None, ids, None,
                         (N,), obs_dtype, out)

  _trace_dtype = torch.int16

  def _trace_planes(self):
    return self._n_planes

  def _gather_op(self, trace, t_idx, e_idx, out):
    _hip.ops.wide_render_gather(self._spec_host, self._tables, trace, t_idx, e_idx, out,
                                self._bad_idx, self._bad_idx_flag, fused.GATHER_STREAMING)

  def rollout_deferred(self, actions, out, reset_first=False, actions_ready=False):
    """`FusedGame.rollout_deferred` for this tier, which has no shared launch: the rollout is
    run whole, at once, and `out` is simply complete a call early; returns the previous call's
    dict (None on the first)."""
    prev = getattr(self, '_deferred', None)
    if prev is not None and prev['obs'].data_ptr() == out['obs'].data_ptr():
      raise ValueError('the state-table tier runs a deferred rollout whole, at once: two dicts over ONE '
                       'observation buffer (rollout_buffers(T, share=...)) would hand back the previous '
                       'rollout\'s dict with this rollout\'s observations in it - give each dict its own '
                       'buffers (rollout_buffers(T) twice)')
    self.rollout(actions, out=out, reset_first=reset_first)
    self._deferred = out
    return prev

  def flush(self):
    prev, self._deferred = getattr(self, '_deferred', None), None
    return prev

  def rollout(self, actions, obs=None, board=None, keep_obs=True, reset_first=False,
              want_board=False, obs_dtype=torch.int8, out=None, pipelined=False):
    """T frames in one call (see `fused.FusedGame.rollout`; `pipelined` is not offered here).
    'trace' in the result is int16 [K, T, B]: cell | covered scenery layer << 10 | shows << 15."""
    if pipelined:
      raise ValueError('wide tier: pipelined rollouts are not offered')
    T = int(actions.shape[0])
    if T < 1:
      raise ValueError('a rollout needs at least one frame: actions [T, B] with T >= 1')
    if (torch.is_tensor(actions) and actions.dtype == torch.int8 and actions.device == self.device
        and actions.shape == (T, self.batch) and actions.is_contiguous()):
      ids = actions
    else:
      ids = self._action_ids(actions, (T, self.batch))
    if out is None:
      B, L, H, W, dev = self.batch, self.n_layers, self.rows, self.cols, self.device
      if obs is not None and keep_obs and (
          tuple(obs.shape) != (T, B, L, H, W) or obs.dtype != obs_dtype
          or not obs.is_contiguous() or obs.device != dev):
        raise ValueError('obs must be a contiguous {} [T,B,L,H,W] tensor on {}'.format(obs_dtype, dev))
      out = self.rollout_buffers(T, keep_obs, want_board or board is not None, obs_dtype)
      if obs is not None and keep_obs:
        out['obs'] = obs
      if board is not None:
        out['board'] = board
    validate = self.validate_actions
    self._wide(self._spec_host, self._tables, self.state, self.done, self.ret, ids, out['obs'],
               out['board'], out['reward'], out['discount'], out['done'], out['perf'],
               out['trace'], self._bad if validate else None,
               self._bad_flag if validate else None, bool(reset_first))
    self.frame = T if reset_first else self.frame + T
    if validate:
      self._after_launch()
    return out
