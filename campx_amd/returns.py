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
  _rows(reward, 'reward', torch.float32, None, None, None)
  T, B = int(reward.shape[0]), int(reward.shape[1])
  device = reward.device
  if device.type != 'cuda':
    raise ValueError('reward must be on a HIP device, it is on {} (there is no CPU path)'.format(device))
  _rows(done, 'done', torch.uint8, T, B, device)
  if discount is not None:
    _rows(discount, 'discount', torch.float32, T, B, device)
  if values is not None:
    _rows(values, 'values', torch.float32, T, B, device)
    values = values.detach()
  if bootstrap is not None:
    if (not torch.is_tensor(bootstrap) or bootstrap.dtype != torch.float32
        or tuple(bootstrap.shape) != (B,) or bootstrap.device != device
        or not bootstrap.is_contiguous()):
      raise ValueError('bootstrap must be a contiguous float32 [{}] tensor on {}'.format(B, device))
    bootstrap = bootstrap.detach()
  for name, x in (('gamma', gamma), ('lam', lam)):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
      raise ValueError('{} must be a finite number, got {!r}'.format(name, x))
  want = ('returns',) + (('advantages',) if values is not None else ())
  if out is None:
    out = {k: torch.empty((T, B), dtype=torch.float32, device=device) for k in want}
  else:
    if not isinstance(out, dict):
      raise ValueError('out must be a dict of float32 [T, B] tensors: {}'.format(list(want)))
    for k in want:
      _rows(out.get(k), "out['{}']".format(k), torch.float32, T, B, device)
  _hip.ops.returns(reward, done, float(gamma), discount, values, bootstrap, float(lam),
                   out['returns'], out['advantages'] if values is not None else None)
  return out if set(out) == set(want) else {k: out[k] for k in want}
