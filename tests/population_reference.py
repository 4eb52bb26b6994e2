"""A host walk of a `tabulate.TracedGame`'s state table under a POPULATION of policies: the
checker of `WideGame.rollout_population()` (csrc/k_population.hip).  Built from
`policy_reference.words / sample` - the sampling rule restated in numpy - and shares no code with
the HIP path.

The B environments split into P equal contiguous blocks of n = B // P: environment e belongs to
member e // n and samples row `policies[e // n, s]` in state s (s = 0 after a done).  The Philox
counter is the absolute environment and the absolute frame, so P copies of one policy walk what
`policy_reference.PolicyWalker` walks.  'states' holds the flat row `(e // n) * n_states + s`.
"""

import numpy as np

import policy_reference as ref

N_ACTIONS = ref.N_ACTIONS


def members(B, P):
  """int64 [B]: the member of every environment."""
  B, P = int(B), int(P)
  assert P >= 1 and B % P == 0, (B, P)
  return np.arange(B, dtype=np.int64) // (B // P)


class PopulationWalker(object):
  """B environments of a `TracedGame` (anything with `n_states` and the `st_*` arrays) walked
  through its table, every action sampled from the environment's member of `policies`
  float32 [P, n_states, 5]."""

  def __init__(self, game, batch):
    self.game = game
    self.B = int(batch)
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, np.float32)
    self.frame = 0

  def rollout(self, policies, T, seed=0, first_frame=None, reset_first=False):
    """-> dict(states int32 (flat rows), actions int8, reward, discount float32, done uint8, perf
    int8, all [T, B]; bad: environment-frames that met a bad row; bad_by_member int64 [P]);
    `state`, `over`, `ret` carry over."""
    g = self.game
    policies = np.asarray(policies, np.float32)
    assert policies.ndim == 3 and policies.shape[1:] == (g.n_states, N_ACTIONS), policies.shape
    P, S = policies.shape[0], g.n_states
    member = members(self.B, P)
    flat = policies.reshape(P * S, N_ACTIONS)
    first = self.frame if first_frame is None else int(first_frame)
    env = np.arange(self.B, dtype=np.uint64)
    out = dict(states=np.zeros((T, self.B), np.int32), actions=np.zeros((T, self.B), np.int8),
               reward=np.zeros((T, self.B), np.float32), discount=np.zeros((T, self.B), np.float32),
               done=np.zeros((T, self.B), np.uint8), perf=np.zeros((T, self.B), np.int8), bad=0,
               bad_by_member=np.zeros(P, np.int64))
    if reset_first:
      self.over[:] = True
    for t in range(T):
      s = np.where(self.over, 0, self.state)
      row = member * S + s
      a, bad = ref.sample(ref.words(seed, env, first + t), flat[row])
      out['bad'] += int(bad.sum())
      np.add.at(out['bad_by_member'], member[bad], 1)
      a64 = a.astype(np.int64)
      self.ret = np.where(self.over, np.float32(0), self.ret).astype(np.float32)
      self.state = g.st_next[s, a64].astype(np.int64)
      reward = g.st_reward[s, a64].astype(np.float32)
      self.ret = (self.ret + np.where(np.isnan(reward), np.float32(0), reward)).astype(np.float32)
      self.over = g.st_done[s, a64] != 0
      out['states'][t] = row
      out['actions'][t] = a
      out['reward'][t] = reward
      out['discount'][t] = g.st_discount[s, a64]
      out['done'][t] = self.over
      out['perf'][t] = g.st_perf[s, a64]
    self.frame = first + T
    return out
