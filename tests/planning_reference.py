"""Policy evaluation and value iteration on a state table, restated in numpy float32 from the rule
in include/campx_hip.h ("Exact policy evaluation and value iteration on the state table"): the
checker of tests/test_planning.py.  No torch, no HIP, no code shared with campx_amd/.

A table is four `[S, 5]` arrays, each entry as a rollout reports the frame that takes action a in
state s: `next_state` (int), `reward` float32 (NaN = None), `done`, `discount` float32 - the
`st_next`, `st_reward`, `st_done`, `st_discount` of a `tabulate.TracedGame` or of
`wide_table_reference.make_table()`.  Every operation below is one float32 operation, rounded on
its own, in the order the header gives.
"""

import numpy as np

N_ACTIONS = 5
F = np.float32


def frame_discount(code, done, discount_list):
  """D of the rule: discount_list[code], or - code 0 - 0.0 when the entry ends the episode and 1.0
  otherwise."""
  code, done = np.asarray(code), np.asarray(done)
  listed = np.asarray(discount_list, F)[code]
  return np.where(code != 0, listed, np.where(done != 0, F(0), F(1))).astype(F)


def backup(next_state, reward, done, discount, gamma, v):
  """q [S, 5] of the values v [S]."""
  with np.errstate(all='ignore'):
    reward = np.asarray(reward, F)
    r = np.where(np.isnan(reward), F(0), reward).astype(F)
    c = (F(gamma) * np.asarray(discount, F)).astype(F)
    vn = np.asarray(v, F)[np.asarray(next_state, np.int64)]
    carried = (r + (c * vn).astype(F)).astype(F)
    return np.where(np.asarray(done) != 0, r, carried).astype(F)


def policy_total(policy):
  """-> (c4 [S] float32, bad [S] bool): the sampler's total of a row's weights, and its test."""
  w = np.asarray(policy, F)
  with np.errstate(all='ignore'):
    c4 = ((((w[:, 0] + w[:, 1]).astype(F) + w[:, 2]).astype(F) + w[:, 3]).astype(F) + w[:, 4]).astype(F)
    good = (w >= 0).all(axis=1) & (c4 > 0) & (c4 < np.inf)
  return c4, ~good


def reduce_policy(q, policy):
  """-> (v' [S], number of bad rows)."""
  w = np.asarray(policy, F)
  c4, bad = policy_total(w)
  with np.errstate(all='ignore'):
    num = (w[:, 0] * q[:, 0]).astype(F)
    for a in range(1, N_ACTIONS):
      num = (num + (w[:, a] * q[:, a]).astype(F)).astype(F)
    v = (num / np.where(bad, F(1), c4)).astype(F)
  return np.where(bad, q[:, 4], v).astype(F), int(bad.sum())


def reduce_greedy(q):
  """-> (v' [S], greedy action [S] int8): best = q0; for a = 1 .. 4: if q[a] > best ..."""
  best = q[:, 0].copy()
  arg = np.zeros(len(q), np.int8)
  with np.errstate(all='ignore'):
    for a in range(1, N_ACTIONS):
      better = q[:, a] > best
      best = np.where(better, q[:, a], best).astype(F)
      arg = np.where(better, np.int8(a), arg).astype(np.int8)
  return best, arg


def residual_of(v_new, v_old):
  """The float whose bit pattern is the largest of the bit patterns of |v_new - v_old|."""
  with np.errstate(all='ignore'):
    d = np.abs((np.asarray(v_new, F) - np.asarray(v_old, F)).astype(F)).astype(F)
  return np.array([d.view(np.uint32).max()], np.uint32).view(F)[0]


def sweeps(next_state, reward, done, discount, gamma, n, policy=None, values=None,
           reward_override=None):
  """n Jacobi sweeps from `values` (None: zeros); `policy` [S, 5] weights, or None for the greedy
  reduction.  -> dict(values = v_n, q = q_n, greedy (policy None), residual [n], bad_rows,
  history = [v_0, v_1, ..., v_n])."""
  S = len(next_state)
  v = np.zeros(S, F) if values is None else np.asarray(values, F).copy()
  r = np.asarray(reward if reward_override is None else reward_override, F)
  history, residual = [v], np.zeros(n, F)
  q, greedy, bad = None, None, 0
  for k in range(n):
    q = backup(next_state, r, done, discount, gamma, v)
    if policy is None:
      new, greedy = reduce_greedy(q)
    else:
      new, bad = reduce_policy(q, policy)
    residual[k] = residual_of(new, v)
    v = new
    history.append(v)
  out = dict(values=v, q=q, residual=residual, bad_rows=bad, history=history)
  if policy is None:
    out['greedy'] = greedy
  return out
