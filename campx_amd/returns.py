"""Discounted returns and GAE advantages of a rollout, in one launch and aware of episode ends.

A rollout of this engine rebuilds a finished environment in-kernel, so an episode may end on any
frame inside one and the next begins on the frame after.  The usual host loop

    for r in reversed(out['reward']): running = r + gamma * running

is T tiny launches, carries the return of the NEXT episode across every `done`, and turns a whole
column into NaN when one frame reports no reward (None, the NaN plane).  `discounted_returns()` is
the same backward pass as one kernel (csrc/k_returns.hip, `campx::returns`) that does neither.  It
is tier-agnostic: it takes the `[T, B]` streams of `rollout()`, `rollout_trace()`,
`rollout_policy()` or `capture_play`, padded rows as they are.

The rule is in include/campx_hip.h next to the sampling rule; tests/returns_reference.py restates
it in numpy float32, bit for bit.  No CPU path.

`vtrace_returns()` is that pass for streams that OTHER policies sampled - the stale actors of a
`rollout_population()` feeding one learner: V-trace targets and advantages, the importance ratio a
stream or looked up from the two policies' tables inside the kernel (csrc/k_vtrace.hip,
`campx::vtrace`; tests/vtrace_reference.py restates the rule).

The learner's half of such an episode is here too.  Everything a tabular loss needs from the
`[T, B]` streams is a sum per (state, action): `sum_by_state()` is that reduction in one launch, in
64-bit fixed point - order-independent, so bitwise reproducible - and `table_lookup()` is the
`table[states, actions]` gather without the two int64 copies of the streams, differentiable in the
table through `sum_by_state()` (csrc/k_sums.hip, `campx::state_sums`, `campx::table_lookup`;
tests/state_sums_reference.py restates the rule in numpy).

`softmax_weights()` turns the preferences of softmax policies into the sampler's weights by the
exponent rule of `WideGame.learn_actor_critic()` - a stated float32 rule, the same bits on the CPU,
on the device and inside that learner's kernel (tests/actor_critic_reference.py restates it).
"""

import math

import torch

from . import _hip


def _rows(t, name, dtype, T, B, device):
  if not torch.is_tensor(t):
    raise ValueError('{} must be a {} [T, B] tensor, got {}'.format(name, dtype, type(t).__name__))
  if t.dtype != dtype:
    raise ValueError('{} must be {}, it is {}'.format(name, dtype, t.dtype))
  if t.dim() != 2 or (T is not None and tuple(t.shape) != (T, B)):
    raise ValueError('{} must have shape {}, it has {}'.format(
        name, '[T, B]' if T is None else [T, B], list(t.shape)))
  if t.shape[0] < 1 or t.shape[1] < 1:
    raise ValueError('{} must have at least one frame and one environment, it has shape {}'.format(
        name, list(t.shape)))
  if device is not None and t.device != device:
    raise ValueError('{} must be on {}, it is on {}'.format(name, device, t.device))
  if t.shape[1] > 1 and t.stride(1) != 1:
    raise ValueError('{} must be contiguous within a row (stride(1) == 1), its strides are {}'.format(
        name, list(t.stride())))
  if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
    raise ValueError('{} has row pitch {}, below its {} columns'.format(name, t.stride(0), t.shape[1]))


def _first_stream(t, name, dtype, fn):
  """The stream that tells a call its shape and device; returns (T, B, device)."""
  _rows(t, name, dtype, None, None, None)
  T, B = int(t.shape[0]), int(t.shape[1])
  if t.device.type != 'cuda':
    raise ValueError('{} must be on a HIP device, it is on {} (there is no CPU path)'.format(name, t.device))
  if T > 0x7fffffff or B > 1 << 31:
    raise ValueError('{}: [T, B] = {} is too large'.format(fn, [T, B]))
  return T, B, t.device


def _got(x):
  return '{} {} on {}'.format(x.dtype, list(x.shape), x.device) if torch.is_tensor(x) else type(x).__name__


def _finite(x, name):
  if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
    raise ValueError('{} must be a finite number, got {!r}'.format(name, x))
  return float(x)


def _bootstrap(bootstrap, B, device):
  if bootstrap is None:
    return None
  if (not torch.is_tensor(bootstrap) or bootstrap.dtype != torch.float32
      or tuple(bootstrap.shape) != (B,) or bootstrap.device != device
      or not bootstrap.is_contiguous()):
    raise ValueError('bootstrap must be a contiguous float32 [{}] tensor on {}'.format(B, device))
  return bootstrap.detach()


def _counter(c, name, device):
  if not torch.is_tensor(c) or c.dtype != torch.int64 or c.numel() != 1 or c.device != device:
    raise ValueError('{} must be an int64 tensor of one element on {}'.format(name, device))


def _out_streams(out, want, T, B, device):
  """The dict of float32 `[T, B]` streams a call writes: a new one, or the caller's, checked."""
  if out is None:
    return {k: torch.empty((T, B), dtype=torch.float32, device=device) for k in want}
  if not isinstance(out, dict):
    raise ValueError('out must be a dict of float32 [T, B] tensors: {}'.format(list(want)))
  for k in want:
    _rows(out.get(k), "out['{}']".format(k), torch.float32, T, B, device)
  return out


def discounted_returns(reward, done, gamma, discount=None, values=None, bootstrap=None, lam=1.0,
                       out=None):
  """Returns - and, with `values`, GAE advantages - of `[T, B]` rollout streams: one launch.

  For t = T-1 down to 0, per environment e, in float32 with every operation rounded on its own:

      r      = 0 if isnan(reward[t]) else reward[t]
      c      = gamma * discount[t]                  (gamma when `discount` is None)
      G[t]   = r if done[t] else r + c * G[t+1]     (G[T] = bootstrap[e], or 0)
      delta  = (r if done[t] else r + c * V[t+1]) - V[t]          (V[T] = bootstrap[e], or 0)
      A[t]   = delta if done[t] else delta + (c * lam) * A[t+1]   (A[T] = 0)

  Args:
    reward: float32 `[T, B]`; NaN means "no reward" and counts as 0.
    done: uint8 `[T, B]`: the episode ended ON the frame (nothing is carried across it).
    gamma: the discount factor, a finite float.
    discount: float32 `[T, B]`, the engine's per-frame discount, or None for 1.0.
    values: float32 `[T, B]`, a critic at the state each frame STARTS in - `V[out['states']]` for
        a `rollout_policy()` - or None: no advantages.
    bootstrap: float32 `[B]`, the value of the state after the last frame, or None for 0.
    lam: GAE's lambda, a finite float (1.0: A = G - V).
    out: a dict of float32 `[T, B]` tensors to write into: 'returns', and 'advantages' when
        `values` is given.  The call is then capturable in a HIP graph.

  Every `[T, B]` tensor lives on one HIP device with `stride(1) == 1` and any row pitch >= B, each
  its own: the padded views of `rollout_buffers()` and its kin are taken without a copy.  A
  `values` that requires grad is used through `.detach()`.

  Returns a dict: 'returns' float32 `[T, B]`, and 'advantages' float32 `[T, B]` only when `values`
  is given.  Argument errors raise ValueError before anything is launched.
  """
  T, B, device = _first_stream(reward, 'reward', torch.float32, 'discounted_returns')
  _rows(done, 'done', torch.uint8, T, B, device)
  if discount is not None:
    _rows(discount, 'discount', torch.float32, T, B, device)
  if values is not None:
    _rows(values, 'values', torch.float32, T, B, device)
    values = values.detach()
  bootstrap = _bootstrap(bootstrap, B, device)
  gamma, lam = _finite(gamma, 'gamma'), _finite(lam, 'lam')
  want = ('returns',) + (('advantages',) if values is not None else ())
  out = _out_streams(out, want, T, B, device)
  _hip.ops.returns(reward, done, gamma, discount, values, bootstrap, lam,
                   out['returns'], out['advantages'] if values is not None else None)
  return out if set(out) == set(want) else {k: out[k] for k in want}


# ------------------------------------------------------------------ off-policy returns

def _bar(x, name):
  if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0:
    raise ValueError('{} must be a finite number >= 0, got {!r}'.format(name, x))
  return float(x)


def vtrace_returns(reward, done, gamma, values, ratio=None, target=None, behaviour=None, states=None,
                   actions=None, discount=None, bootstrap=None, lam=1.0, rho_bar=1.0, c_bar=1.0,
                   pg_rho_bar=None, bad_count=None, out=None, path=0):
  """V-trace targets and advantages of `[T, B]` streams that OTHER policies sampled: one launch.

  The off-policy counterpart of `discounted_returns()` (Espeholt et al. 2018, IMPALA): a learner
  fed by stale or perturbed actors, population-based training, one rollout used for several
  gradient steps.  For t = T-1 down to 0, per environment e, in float32 with every operation
  rounded on its own (include/campx_hip.h has the rule in full):

      r, c     as in discounted_returns()
      w        = ratio[t]                                             (ratio mode), or
                 target[states[t] % Nt, actions[t]] / behaviour[states[t], actions[t]]   (table mode)
      w        = w if w > 0 else +0           (NaN, negatives and -0 count as 0; +inf stays)
      rho, cs, rpg = min(w, rho_bar), min(w, c_bar), min(w, pg_rho_bar)
      delta    = rho * ((r if done[t] else r + c * V[t+1]) - V[t])    (V[T] = bootstrap[e], or 0)
      D[t]     = delta if done[t] else delta + ((c * lam) * cs) * D[t+1]       (D[T] = 0)
      vs[t]    = V[t] + D[t]
      adv[t]   = rpg * ((r if done[t] else r + c * vs[t+1]) - V[t])   (vs[T] = bootstrap[e], or 0)

  With every ratio 1 and every bar 1, `vs` is bit for bit `values + discounted_returns(...)
  ['advantages']` at the same `lam`.

  Args:
    reward, done, gamma, discount, bootstrap, lam: as in `discounted_returns()`.
    values: float32 `[T, B]`, the critic at the state each frame STARTS in.
    ratio: float32 `[T, B]`, pi(a|s) / mu(a|s) per frame - ratio mode, any tier's streams.
    target, behaviour, states, actions: table mode, the four together and no `ratio`.  `target` is
        the learner's float32 `[Nt, A]` of action probabilities, `behaviour` the float32 `[Nb, A]`
        the data was sampled with, Nb a multiple of Nt, A <= 128; `states` int32 and `actions` int8
        `[T, B]`.  For `rollout_population()`, whose states are `member * S + state`:
        `behaviour = probabilities.view(-1, 5)`, `target` the learner's `[S, 5]`; for
        `rollout_policy()` both are `[S, 5]`.  A frame whose state is outside [0, Nb) or whose
        action is outside [0, A) gets w = 0 and is added to `bad_count`; the tables are not read
        for it.
    rho_bar, c_bar, pg_rho_bar: the truncation levels, finite and >= 0; `pg_rho_bar=None` means
        `rho_bar`.
    bad_count: an int64 tensor of one element on the device, or None.
    out: a dict of float32 `[T, B]` tensors to write into, 'vs' and 'advantages'.  The call then
        allocates nothing and is capturable in a HIP graph.
    path: table mode, where the tables are read from: 0 lets the library choose, 1 forces both
        into LDS (ValueError when they do not fit), 2 reads them through the caches.  By the rule
        no bit of the result depends on it.

  Every `[T, B]` tensor lives on one HIP device with `stride(1) == 1` and any row pitch >= B, each
  its own.  Inputs are used through `.detach()`: the outputs are targets.  Returns a dict: 'vs',
  the critic's regression target, and 'advantages', the policy-gradient weight with the truncated
  ratio already inside.  Argument errors raise ValueError before anything is launched.  No CPU path.
  """
  gamma, lam = _finite(gamma, 'gamma'), _finite(lam, 'lam')
  rho_bar, c_bar = _bar(rho_bar, 'rho_bar'), _bar(c_bar, 'c_bar')
  pg_rho_bar = rho_bar if pg_rho_bar is None else _bar(pg_rho_bar, 'pg_rho_bar')
  _count_arg(path, 'path', 0, 2)
  tables = (target, behaviour, states, actions)
  given = sum(x is not None for x in tables)
  if given not in (0, 4) or (given == 4) == (ratio is not None):
    raise ValueError('give ratio, or target, behaviour, states and actions together - not both, not neither')
  T, B, device = _first_stream(reward, 'reward', torch.float32, 'vtrace_returns')
  _rows(done, 'done', torch.uint8, T, B, device)
  _rows(values, 'values', torch.float32, T, B, device)
  if discount is not None:
    _rows(discount, 'discount', torch.float32, T, B, device)
    discount = discount.detach()
  bootstrap = _bootstrap(bootstrap, B, device)
  if ratio is not None:
    _rows(ratio, 'ratio', torch.float32, T, B, device)
    ratio = ratio.detach()
  else:
    for name, x in (('target', target), ('behaviour', behaviour)):
      if (not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or x.device != device
          or not x.is_contiguous() or x.shape[0] < 1 or not 1 <= x.shape[1] <= 128):
        raise ValueError('{} must be a contiguous float32 [n_states, n_actions <= 128] tensor on {}, got {}'.format(
            name, device, _got(x)))
    Nt, Nb, A = int(target.shape[0]), int(behaviour.shape[0]), int(target.shape[1])
    if behaviour.shape[1] != A or Nb % Nt != 0 or Nb > 0x7fffffff:
      raise ValueError('behaviour must be [Nb, {}] with Nb a multiple of target\'s {} rows and at most '
                       '2^31 - 1, it is {}'.format(A, Nt, list(behaviour.shape)))
    _rows(states, 'states', torch.int32, T, B, device)
    _rows(actions, 'actions', torch.int8, T, B, device)
    if path == 1 and (Nt + Nb) * A * 4 > _hip.SUMS_LDS_BUDGET:
      raise ValueError('path=1: tables of {} + {} entries of 4 bytes do not fit the LDS budget of {} bytes'.format(
          Nt * A, Nb * A, _hip.SUMS_LDS_BUDGET))
    target, behaviour = target.detach(), behaviour.detach()
  if bad_count is not None:
    _counter(bad_count, 'bad_count', device)
  want = ('vs', 'advantages')
  out = _out_streams(out, want, T, B, device)
  _hip.ops.vtrace(reward.detach(), done, gamma, values.detach(), ratio, target, behaviour, states,
                  actions, discount, bootstrap, lam, rho_bar, c_bar, pg_rho_bar, bad_count,
                  int(path), out['vs'], out['advantages'])
  return out if set(out) == set(want) else {k: out[k] for k in want}


# ------------------------------------------------------------------ per-state sums and lookups

def _sums_streams(states, actions, fn):
  """Checks the index streams of `sum_by_state()` / `table_lookup()`; returns (T, B, device)."""
  T, B, device = _first_stream(states, 'states', torch.int32, fn)
  if actions is not None:
    _rows(actions, 'actions', torch.int8, T, B, device)
  return T, B, device


def _count_arg(x, name, low, high):
  if isinstance(x, bool) or not isinstance(x, int) or not low <= x <= high:
    raise ValueError('{} must be an integer in [{}, {}], got {!r}'.format(name, low, high, x))
  return x


def sums_limits(T, B):
  """(n2, largest frac_bits) of the fixed-point rule for N = T * B frames: n2 = ceil(log2(N)),
  a value is clamped to +-2^(62 - n2) quanta and frac_bits may be at most 62 - n2."""
  n2 = (int(T) * int(B) - 1).bit_length()
  return n2, 62 - n2


def sum_by_state(states, actions=None, values=(), n_states=None, n_actions=5, frac_bits=24,
                 accumulate=False, out=None, path=0):
  """Count and sum `[T, B]` streams per (state, action) - or per state - in one launch.

  The rule (include/campx_hip.h), in 64-bit fixed point so that the result does not depend on the
  order of the additions and is bitwise reproducible.  With f = `frac_bits` and N = T * B:

      n2    = ceil(log2(N))                     lim = 2^(62 - n2); f <= 62 - n2 is required
      q     = llrint(double(x) * 2^f)           round to nearest even; the product is exact
      q     = 0, counted in 'clamped'           if x is NaN
      q     = +-lim, counted in 'clamped'       if |double(x) * 2^f| > lim (+-Inf included)
      bin   = states[t, e] * n_actions + actions[t, e]      (n_actions = 1 without `actions`)
      raw[0][bin]     += 1
      raw[1 + k][bin] += q_k                    for each of the K value streams

  A frame whose state is outside [0, n_states) or whose action is outside [0, n_actions) adds
  nothing and is counted in 'skipped' (its values are not looked at).  N additions of at most lim
  cannot overflow an int64.  Without clamping, sums[k] is within count * 2^-(f + 1) of the exact sum.

  Args:
    states: int32 `[T, B]`, e.g. `rollout_policy()`'s 'states'.
    actions: int8 `[T, B]` ('actions'), or None: sums per state, results without the action axis.
    values: up to 4 float32 `[T, B]` streams (returns, advantages, their squares ...).  A stream
        that requires grad is used through `.detach()`.
    n_states: rows of the table the states index (`Engine.n_states`), 1 .. 2^31 - 1.
    n_actions: 1 .. 128; ignored (1) when `actions` is None.
    frac_bits: f above, 0 .. 62 - n2.
    accumulate: add onto `out` instead of overwriting it: several rollouts reduced into one step
        (the no-overflow bound holds per call).  Needs `out`.
    out: a dict with 'raw' int64 `[K + 1, n_states, n_actions]` (`[K + 1, n_states]` without
        actions), contiguous, and 'skipped' and 'clamped', int64 tensors of one element; the call
        allocates nothing the accumulators need and is capturable in a HIP graph.
    path: 0 lets the library choose where the accumulators live, 1 forces LDS (ValueError when
        they do not fit), 2 global memory.  By the rule, no bit of the result depends on it.

  Every `[T, B]` tensor lives on one HIP device with `stride(1) == 1` and any row pitch >= B, each
  its own.  Returns a dict: 'count' int64 `[n_states, n_actions]` (a view of raw[0]), 'sums'
  float64 `[K, n_states, n_actions]` = raw[1:] * 2^-f, 'raw' the accumulators themselves, 'skipped'
  and 'clamped' device int64 scalars - reading them is the caller's synchronisation.  Argument
  errors raise ValueError before anything is launched.  No CPU path.
  """
  T, B, device = _sums_streams(states, actions, 'sum_by_state')
  if not isinstance(values, (tuple, list)):
    raise ValueError('values must be a tuple of float32 [T, B] tensors, got {}'.format(type(values).__name__))
  K = len(values)
  if K > _hip.SUMS_MAX_VALUES:
    raise ValueError('at most {} value streams, got {}'.format(_hip.SUMS_MAX_VALUES, K))
  for k, v in enumerate(values):
    _rows(v, 'values[{}]'.format(k), torch.float32, T, B, device)
  values = [v.detach() for v in values]
  S = _count_arg(n_states, 'n_states', 1, 0x7fffffff)
  A = 1 if actions is None else _count_arg(n_actions, 'n_actions', 1, 128)
  n2, most = sums_limits(T, B)
  _count_arg(frac_bits, 'frac_bits (N = T * B = {}, n2 = {})'.format(T * B, n2), 0, most)
  _count_arg(path, 'path', 0, 2)
  if path == 1 and S * A * (K + 1) * 8 > _hip.SUMS_LDS_BUDGET:
    raise ValueError('path=1: {} accumulators of 8 bytes do not fit the LDS budget of {} bytes'.format(
        S * A * (K + 1), _hip.SUMS_LDS_BUDGET))
  shape = (K + 1, S) + (() if actions is None else (A,))
  if out is None:
    if accumulate:
      raise ValueError('accumulate=True adds onto out: pass the dict of an earlier call')
    counters = torch.empty((2,), dtype=torch.int64, device=device)
    out = {'raw': torch.empty(shape, dtype=torch.int64, device=device),
           'skipped': counters[0], 'clamped': counters[1]}
  else:
    if not isinstance(out, dict):
      raise ValueError("out must be a dict: 'raw' int64 {}, 'skipped' and 'clamped' int64 scalars".format(
          list(shape)))
    raw = out.get('raw')
    if (not torch.is_tensor(raw) or raw.dtype != torch.int64 or tuple(raw.shape) != shape
        or raw.device != device or not raw.is_contiguous()):
      raise ValueError("out['raw'] must be a contiguous int64 {} tensor on {}, got {}".format(
          list(shape), device, _got(raw)))
    for k in ('skipped', 'clamped'):
      _counter(out.get(k), "out['{}']".format(k), device)
  raw = out['raw']
  _hip.ops.state_sums(states, actions, values, S, A, int(frac_bits), bool(accumulate), int(path),
                      raw, out['skipped'], out['clamped'])
  return {'count': raw[0], 'sums': raw[1:].double() * 2.0 ** -frac_bits, 'raw': raw,
          'skipped': out['skipped'].view(()), 'clamped': out['clamped'].view(())}


class _TableLookup(torch.autograd.Function):
  """`table_lookup()`: the forward is campx::table_lookup, the backward one `sum_by_state()`."""

  @staticmethod
  def forward(ctx, table, states, actions, bad_count):
    T, B = states.shape
    x = torch.empty((T, B), dtype=torch.float32, device=states.device)
    _hip.ops.table_lookup(table.detach(), states, actions, x, bad_count)
    ctx.save_for_backward(states, *(() if actions is None else (actions,)))
    ctx.table_shape = tuple(table.shape)
    return x

  @staticmethod
  def backward(ctx, grad_out):
    if not ctx.needs_input_grad[0]:
      return None, None, None, None
    states = ctx.saved_tensors[0]
    actions = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
    T, B = states.shape
    grad_out = grad_out.detach()
    if grad_out.dtype != torch.float32:
      grad_out = grad_out.float()
    if (B > 1 and grad_out.stride(1) != 1) or (T > 1 and grad_out.stride(0) < B):
      grad_out = grad_out.contiguous()             # (a broadcast gradient: `x.sum().backward()`)
    S = ctx.table_shape[0]
    A = ctx.table_shape[1] if actions is not None else 1
    sums = sum_by_state(states, actions, values=(grad_out,), n_states=S, n_actions=A,
                        frac_bits=min(24, sums_limits(T, B)[1]))
    return sums['sums'][0].float(), None, None, None


def table_lookup(table, states, actions=None, bad_count=None):
  """`table[states, actions]` of a rollout's streams as they are: float32 `[T, B]`, one launch.

  `x[t, e] = table[states[t, e], actions[t, e]]` (`table[states[t, e]]` when `actions` is None),
  what `table[states.long(), actions.long()]` computes, without the two int64 copies of the
  streams.  Differentiable in `table`: the backward is
  `sum_by_state(states, actions, values=(grad_out,))['sums'][0].float()` - the per-bin sum of the
  incoming gradient by `sum_by_state()`'s fixed-point rule (frac_bits 24), bitwise reproducible,
  where the advanced index accumulates float32 in arrival order.

  Args:
    table: float32 `[n_states, n_actions]` (n_actions <= 128), or `[n_states]` when `actions` is
        None; contiguous, on the streams' device.
    states: int32 `[T, B]`; actions: int8 `[T, B]` or None - `stride(1) == 1`, any row pitch >= B.
    bad_count: an int64 tensor of one element on the device, or None.  A frame whose state or
        action is out of range gets 0.0 (and no gradient) and is added to it.

  Argument errors raise ValueError before anything is launched.  No CPU path.
  """
  T, B, device = _sums_streams(states, actions, 'table_lookup')
  want_dim = 1 if actions is None else 2
  if (not torch.is_tensor(table) or table.dtype != torch.float32 or table.dim() != want_dim
      or table.device != device or not table.is_contiguous() or table.numel() < 1
      or table.shape[0] > 0x7fffffff or (want_dim == 2 and table.shape[1] > 128)):
    raise ValueError('table must be a contiguous float32 {} tensor on {}, got {}'.format(
        '[n_states]' if actions is None else '[n_states, n_actions <= 128]', device, _got(table)))
  if bad_count is not None:
    _counter(bad_count, 'bad_count', device)
  return _TableLookup.apply(table, states, actions, bad_count)


# The exponent rule of the actor-critic learners (include/campx_hip.h, "Actor-critic online
# learners", rule 1): log2(e) and ln(2)^n / n!, each the nearest float32.
SOFTMAX_LOG2E = float.fromhex('0x1.715476p+0')
SOFTMAX_CUT = -100.0
SOFTMAX_POLY = tuple(float.fromhex(c) for c in (
    '0x1p+0', '0x1.62e43p-1', '0x1.ebfbep-3', '0x1.c6b08ep-5', '0x1.3b2ab6p-7', '0x1.5d87fep-10',
    '0x1.430912p-13'))


def softmax_weights(prefs):
  """The sampler's weights of softmax policies given as preferences: float32 `[..., 5]` in,
  float32 `[..., 5]` out, on the CPU or the device - THE SAME BITS on both, and the bits
  `learn_actor_critic()` samples from inside its kernel.

  The weights are a stated rule, not `exp`: with m the row's maximum, `w = 2^k * p(f)` for
  `t = (h - m) * log2e`, `k = rint(t)`, `f = t - k` and p a degree-6 polynomial by Horner, every
  multiply and add a float32 operation of its own; `w = 0` exactly for `t < -100`.  The maximum's
  weight is exactly 1, so a row's total lies in [1, 5]; the largest relative error against float64
  `exp(h - m)` is 3.74e-6 (include/campx_hip.h has the rule and its coefficients).  A row with a
  NaN or a +inf, or of five -inf, is not good: it gets five zeros, which `rollout_policy()` and
  the evaluation calls treat as a bad row by their own rule.  Elements of -inf in a good row get
  weight 0 - an action never taken.

  `rollout_population(softmax_weights(prefs), ...)`, `evaluate_population(softmax_weights(prefs),
  ...)` and `state_visitation(softmax_weights(prefs[m]), ...)` then see exactly the probabilities
  the learner sampled from.  Written in torch element-wise operations: no kernel of its own, not
  differentiable (the result is detached).
  """
  if (not torch.is_tensor(prefs) or prefs.dtype != torch.float32 or prefs.dim() < 1
      or prefs.shape[-1] != 5):
    raise ValueError('prefs must be a float32 [..., 5] tensor, got {}'.format(_got(prefs)))
  h = prefs.detach()
  m = h[..., 0]
  for a in range(1, 5):                       # the lowest index wins ties, NaN never wins
    m = torch.where(h[..., a] > m, h[..., a], m)
  m = m.unsqueeze(-1)
  good = (torch.sub(m, m) == 0) & (h <= m).all(dim=-1, keepdim=True)
  t = torch.mul(torch.sub(h, m), SOFTMAX_LOG2E)
  some = good & (t >= SOFTMAX_CUT)
  t = torch.where(some, t, torch.zeros_like(t))
  k = torch.round(t)                          # ties to even
  f = torch.sub(t, k)
  p = torch.full_like(f, SOFTMAX_POLY[6])
  for c in SOFTMAX_POLY[5::-1]:
    p = torch.add(torch.mul(p, f), c)
  scale = torch.bitwise_left_shift(k.to(torch.int32) + 127, 23).view(torch.float32)   # 2^k, exact
  return torch.where(some, torch.mul(p, scale), torch.zeros_like(p))
