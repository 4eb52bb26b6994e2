"""Actor-critic online learners (include/campx_hip.h, "Actor-critic online learners";
csrc/k_learn.hip) restated in numpy float32, operation by operation: the checker of
`WideGame.learn_actor_critic()` and of `campx_amd.returns.softmax_weights()`.  Shares no code with
the HIP path or with the torch helper; the Philox words and the thresholds are
tests/policy_reference.py's, the walker's bookkeeping tests/learner_reference.py's.

Rule 1, the weights of a row of preferences h[0..4] - a stated rule, NOT exp():
  m = the greedy maximum (the lowest index wins ties, NaN never wins); the row is good when
  (m - m) == 0 and h[a] <= m for all a; for a good row d = h[a] - m, t = d * log2e; t < -100 gives
  w = 0; else k = rint(t), f = t - k, p by Horner over c6 .. c0, w = ldexp(p, k).  A row that is not
  good has five zeros.
The frame of learner e at absolute frame f, from state s:
  1. w by rule 1 of prefs[e, s]; the action by policy_reference.sample() on policy_reference.words()
     - rollout_policy()'s sampler and stream;
  2. entry (s, a): n, r (NaN counted as 0), done, D;
  3. delta = (done ? r : r + (gamma * D) * values[e, n]) - values[e, s];
  4. values[e, s] += alpha_critic * delta;
  5. step = alpha_actor * delta; prefs[e, s, a'] += step * ((a' == a) - w[a'] / c4);
  6. the window sums, state, done and ret as in learner_reference.
A frame whose row is not good takes action 4 and changes neither table (counted in 'bad_rows'); a
learner whose alpha_actor, alpha_critic or gamma is not finite takes action 4 throughout and keeps
both tables (counted in 'bad').
"""

import numpy as np

import learner_reference as learn_ref
import policy_reference as ref

N_ACTIONS = 5
F = np.float32
LOG2E = F(float.fromhex('0x1.715476p+0'))
CUT = F(-100.0)
POLY = tuple(F(float.fromhex(c)) for c in (
    '0x1p+0', '0x1.62e43p-1', '0x1.ebfbep-3', '0x1.c6b08ep-5', '0x1.3b2ab6p-7', '0x1.5d87fep-10',
    '0x1.430912p-13'))


def weight_of(d):
  """float32 d = h - m (<= 0, or anything: the row test is the caller's) -> the rule's weight."""
  d = np.asarray(d, F)
  with np.errstate(all='ignore'):
    t = (d * LOG2E).astype(F)
    some = t >= CUT
    t = np.where(some, t, F(0)).astype(F)
    k = np.rint(t).astype(F)
    f = (t - k).astype(F)
    p = np.full(d.shape, POLY[6], F)
    for c in POLY[5::-1]:
      p = ((p * f).astype(F) + c).astype(F)
    w = np.ldexp(p, k.astype(np.int32)).astype(F)
  return np.where(some, w, F(0)).astype(F)


def softmax_weights(rows):
  """rows float32 [..., 5] -> (w float32 [..., 5], good bool [...])."""
  h = np.asarray(rows, F)
  with np.errstate(all='ignore'):
    m = h[..., 0]
    for a in range(1, N_ACTIONS):
      m = np.where(h[..., a] > m, h[..., a], m)
    good = ((m - m) == 0) & (h <= m[..., None]).all(axis=-1)
    w = weight_of((h - m[..., None]).astype(F))
  return np.where(good[..., None], w, F(0)).astype(F), good


class ActorCritics(object):
  """B learners on a `TracedGame`'s `st_*` arrays; `prefs` float32 [B, n_states, 5] and `values`
  float32 [B, n_states] are theirs."""

  def __init__(self, game, batch, prefs=None, values=None):
    self.game = game
    self.B = int(batch)
    S = game.n_states
    self.prefs = np.zeros((self.B, S, N_ACTIONS), F) if prefs is None else np.array(prefs, F)
    self.values = np.zeros((self.B, S), F) if values is None else np.array(values, F)
    assert self.prefs.shape == (self.B, S, N_ACTIONS) and self.values.shape == (self.B, S)
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, F)
    self.frame = 0

  def learn(self, T, alpha_actor=0.1, alpha_critic=0.1, gamma=0.99, seed=0, first_frame=None,
            reset_first=False, window=None, record=False):
    """-> dict(reward_sum float32 [W, B], perf_sum int32 [W, B], episodes int32 [W, B], bad: the bad
    learners, bad_rows: environment-frames of good learners that met a row that is not good, and -
    `record` - states, actions [T, B] and delta float32 [T, B]); `prefs`, `values`, `state`, `over`,
    `ret` and `frame` carry over."""
    g, B = self.game, self.B
    window = T if window is None else int(window)
    W = (T + window - 1) // window
    alpha_actor, alpha_critic, gamma = (learn_ref.per_learner(v, B)
                                        for v in (alpha_actor, alpha_critic, gamma))
    bad = ~(np.isfinite(alpha_actor) & np.isfinite(alpha_critic) & np.isfinite(gamma))
    first = self.frame if first_frame is None else int(first_frame)
    lanes = np.arange(B)
    env = lanes.astype(np.uint64)
    out = dict(reward_sum=np.zeros((W, B), F), perf_sum=np.zeros((W, B), np.int32),
               episodes=np.zeros((W, B), np.int32), bad=int(bad.sum()), bad_rows=0)
    if record:
      out['states'], out['actions'] = np.zeros((T, B), np.int32), np.zeros((T, B), np.int8)
      out['delta'] = np.zeros((T, B), F)
    if reset_first:
      self.over[:] = True
    with np.errstate(all='ignore'):
      for t in range(T):
        s = np.where(self.over, 0, self.state)
        h = self.prefs[lanes, s]                          # (a copy: the row as the frame found it)
        w, row_good = softmax_weights(h)
        acts = row_good & ~bad
        w = np.where(acts[:, None], w, F(0)).astype(F)
        a, _ = ref.sample(ref.words(seed, env, first + t), w)
        a = a.astype(np.int64)
        assert (a[~acts] == 4).all()
        out['bad_rows'] += int((~row_good & ~bad).sum())
        n = g.st_next[s, a].astype(np.int64)
        reward = g.st_reward[s, a].astype(F)
        r = np.where(np.isnan(reward), F(0), reward).astype(F)
        done = g.st_done[s, a] != 0
        D = g.st_discount[s, a].astype(F)
        v_s, v_n = self.values[lanes, s], self.values[lanes, np.where(done, 0, n)]
        c = (gamma * D).astype(F)
        target = np.where(done, r, (r + (c * v_n).astype(F)).astype(F)).astype(F)
        delta = (target - v_s).astype(F)
        fresh_v = (v_s + (alpha_critic * delta).astype(F)).astype(F)
        self.values[lanes, s] = np.where(acts, fresh_v, v_s)
        step = (alpha_actor * delta).astype(F)
        c4 = ref.thresholds(w)[0][:, 4]
        for k in range(N_ACTIONS):
          pi = (w[:, k] / c4).astype(F)
          grad = ((a == k).astype(F) - pi).astype(F)
          fresh = (h[:, k] + (step * grad).astype(F)).astype(F)
          self.prefs[lanes, s, k] = np.where(acts, fresh, h[:, k])
        w_at = t // window
        out['reward_sum'][w_at] = (out['reward_sum'][w_at] + r).astype(F)
        out['perf_sum'][w_at] += g.st_perf[s, a].astype(np.int32)
        out['episodes'][w_at] += done.astype(np.int32)
        if record:
          out['states'][t], out['actions'][t], out['delta'][t] = s, a, delta
        self.ret = (np.where(self.over, F(0), self.ret).astype(F) + r).astype(F)
        self.state = n
        self.over = done
    self.frame = first + T
    return out
