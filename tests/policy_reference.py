"""The sampling rule of closed-loop rollouts (include/campx_hip.h, csrc/k_policy.hip) restated
in numpy, and a host walk of a `tabulate.TracedGame`'s state table under it: the checker of
`WideGame.rollout_policy()`.  Shares no code with the HIP path.

The rule, for environment e and absolute frame f:
  * one Philox4x32-10 block per environment and group of four frames: key (seed & 0xffffffff,
    seed >> 32), counter (e, g & 0xffffffff, g >> 32, 0) with g = f >> 2; frame f takes output
    word f & 3;
  * u = float32(word >> 8) * 2^-24;
  * thresholds c0 = w0, c1 = c0 + w1, c2 = c1 + w2, c3 = c2 + w3, c4 = c3 + w4 (float32 sums in
    that order), r = u * c4 (one float32 multiply),
    action = (r >= c0) + (r >= c1) + (r >= c2) + (r >= c3);
  * a row with a negative or NaN weight, or whose c4 is not a positive finite number, is bad: the
    environment-frame that meets it takes action 4 and is counted.
"""

import numpy as np

N_ACTIONS = 5
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
  """counter uint32 [..., 4], key uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
  counter = np.asarray(counter, np.uint32)
  key = np.asarray(key, np.uint32)
  c = [counter[..., i].astype(np.uint64) for i in range(4)]
  k0, k1 = int(0), int(0)
  key0, key1 = key[..., 0].astype(np.uint64), key[..., 1].astype(np.uint64)
  for _ in range(10):
    ka = (key0 + np.uint64(k0)) & _MASK
    kb = (key1 + np.uint64(k1)) & _MASK
    p0, p1 = _M0 * c[0], _M1 * c[2]
    hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _MASK, p1 >> _32, p1 & _MASK
    c = [hi1 ^ c[1] ^ ka, lo1, hi0 ^ c[3] ^ kb, lo0]
    k0 = (k0 + _W0) & 0xffffffff
    k1 = (k1 + _W1) & 0xffffffff
  shape = np.broadcast(*c).shape
  return np.stack([np.broadcast_to(x, shape) for x in c], axis=-1).astype(np.uint32)


def words(seed, env, frame):
  """The random word of environment(s) `env` at absolute frame(s) `frame` (broadcast)."""
  seed = int(seed) & ((1 << 64) - 1)
  env, frame = np.broadcast_arrays(np.asarray(env, np.uint64), np.asarray(frame, np.uint64))
  g = frame >> np.uint64(2)
  counter = np.stack([env & _MASK, g & _MASK, g >> _32, np.zeros_like(g)], axis=-1).astype(np.uint32)
  key = np.array([seed & 0xffffffff, seed >> 32], np.uint32)
  block = philox4x32_10(counter, key)
  pick = (frame & np.uint64(3)).astype(np.int64)
  return np.take_along_axis(block, pick[..., None], axis=-1)[..., 0]


def thresholds(rows):
  """rows float32 [..., 5] -> (c float32 [..., 5], bad bool [...])."""
  w = np.asarray(rows, np.float32)
  c = np.empty(w.shape, np.float32)
  with np.errstate(all='ignore'):
    c[..., 0] = w[..., 0]
    for k in range(1, N_ACTIONS):
      c[..., k] = (c[..., k - 1] + w[..., k]).astype(np.float32)
    total = c[..., 4]
    bad = (~(w >= 0)).any(axis=-1) | ~((total > 0) & np.isfinite(total))
  return c, bad


def sample(x, rows):
  """Random words uint32 [...] and the weights float32 [..., 5] they meet -> (actions int8 [...],
  bad bool [...])."""
  c, bad = thresholds(rows)
  u = ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
  with np.errstate(all='ignore'):
    r = (u * c[..., 4]).astype(np.float32)
    a = sum((r >= c[..., k]).astype(np.int8) for k in range(4))
  return np.where(bad, np.int8(4), a).astype(np.int8), bad


class PolicyWalker(object):
  """B environments of a `TracedGame` walked through its `st_*` arrays, every action sampled by
  the rule above from `policy` float32 [n_states, 5]."""

  def __init__(self, game, batch):
    self.game = game
    self.B = int(batch)
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, np.float32)
    self.frame = 0

  def rollout(self, policy, T, seed=0, first_frame=None, reset_first=False):
    """-> dict(states int32, actions int8, reward, discount float32, done uint8, perf int8, all
    [T, B]; bad: environment-frames that met a bad row); `state`, `over`, `ret` carry over."""
    g = self.game
    policy = np.asarray(policy, np.float32)
    assert policy.shape == (g.n_states, N_ACTIONS)
    first = self.frame if first_frame is None else int(first_frame)
    env = np.arange(self.B, dtype=np.uint64)
    out = dict(states=np.zeros((T, self.B), np.int32), actions=np.zeros((T, self.B), np.int8),
               reward=np.zeros((T, self.B), np.float32), discount=np.zeros((T, self.B), np.float32),
               done=np.zeros((T, self.B), np.uint8), perf=np.zeros((T, self.B), np.int8), bad=0)
    if reset_first:
      self.over[:] = True
    for t in range(T):
      s = np.where(self.over, 0, self.state)
      a, bad = sample(words(seed, env, first + t), policy[s])
      out['bad'] += int(bad.sum())
      a64 = a.astype(np.int64)
      self.ret = np.where(self.over, np.float32(0), self.ret).astype(np.float32)
      assert g.st_reached[s, a64].all(), 'the walk left the tabulated (reachable) entries'
      self.state = g.st_next[s, a64].astype(np.int64)
      reward = g.st_reward[s, a64].astype(np.float32)
      self.ret = (self.ret + np.where(np.isnan(reward), np.float32(0), reward)).astype(np.float32)
      self.over = g.st_done[s, a64] != 0
      out['states'][t] = s
      out['actions'][t] = a
      out['reward'][t] = reward
      out['discount'][t] = g.st_discount[s, a64]
      out['done'][t] = self.over
      out['perf'][t] = g.st_perf[s, a64]
    self.frame = first + T
    return out
