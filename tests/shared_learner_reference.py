"""Shared online learners (include/campx_hip.h, "Shared online learners"; csrc/k_learn.hip)
restated in numpy, and a host walk of a `tabulate.TracedGame`'s state table under them: the checker
of `WideGame.learn_shared()`.  Shares no code with the HIP path; the Philox words are
tests/learner_reference.py's and the greedy reduction tests/planning_reference.py's.

P learners; learner m owns q[m] and is fed by the n = B / P environments [m * n, (m + 1) * n).
Frame f of learner m, every float32 operation rounded on its own:
  1. every environment e of the learner does steps 1 - 6 of tests/learner_reference.py's rule with
     q[m] in place of q[e] and alpha_m, gamma_m, epsilon_m; it reads q[m] as it stands at the START
     of the frame; delta_e = target - q[m, s_e, a_e];
  2. d = float64(delta_e) * 2^32; z_e = rint(d) (half to even) as int64; NaN gives 0 and
     |d| > 2^52 gives +-2^52, both counted in clamped[m];
  3. for every (s, a) visited by c >= 1 environments of the learner: Z = sum z_e (`np.add.at` on
     int64), g = float64(Z) / float64(c), mean = float32(g * 2^-32), step = alpha_m * mean,
     q[m, s, a] = q[m, s, a] + step;
  4. the next frame starts from the updated table;
  5. the window sums, ret, state and done are per environment, as in learner_reference.
A learner whose alpha, gamma or epsilon is not finite, or whose epsilon is outside [0, 1], is bad:
all its environments take action 4 every frame, its table is untouched, nothing is accumulated.
"""

import numpy as np

import learner_reference as learn_ref
import planning_reference as plan_ref

N_ACTIONS = 5
F = np.float32
D = np.float64
RULES = learn_ref.RULES
SCALE = D(2.0 ** 32)
LIMIT = D(2.0 ** 52)
LIMIT_Q = np.int64(1) << np.int64(52)


def quantise(delta):
  """(z int64, clamped bool) of float32 TD errors: step 2."""
  with np.errstate(all='ignore'):
    d = np.asarray(delta, F).astype(D) * SCALE
    nan = np.isnan(d)
    over = ~nan & (np.abs(d) > LIMIT)
    z = np.rint(np.where(nan | over, D(0), d)).astype(np.int64)
    z = np.where(over, np.where(d > 0, LIMIT_Q, -LIMIT_Q), z)
  return z, nan | over


def mean_of(Z, c):
  """float32 mean of a bin whose c visitors' quantised errors sum to Z: step 3."""
  g = np.asarray(Z, np.int64).astype(D) / np.asarray(c, np.int64).astype(D)
  return (g * D(2.0 ** -32)).astype(F)


class SharedLearners(object):
  """P learners on a `TracedGame`'s `st_*` arrays, fed by B environments; `q` float32
  [P, n_states, 5] is theirs."""

  def __init__(self, game, batch, q):
    self.game = game
    self.B = int(batch)
    self.q = np.array(q, F)
    self.P = self.q.shape[0]
    assert self.q.shape == (self.P, game.n_states, N_ACTIONS) and self.B % self.P == 0
    self.n = self.B // self.P
    assert 1 <= self.n <= 1024
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, F)
    self.frame = 0

  def learn(self, T, alpha=0.1, gamma=0.99, epsilon=0.1, rule='q', seed=0, first_frame=None,
            reset_first=False, window=None, record=False):
    """-> dict(reward_sum float32 [W, B], perf_sum int32 [W, B], episodes int32 [W, B], clamped
    int64 [P], bad: the bad learners, and - `record` - states, actions [T, B], delta float32 [T, B]
    and z int64 [T, B]); `q`, `state`, `over`, `ret` and `frame` carry over."""
    assert rule in RULES
    g, B, P, n, q = self.game, self.B, self.P, self.n, self.q
    S = g.n_states
    window = T if window is None else int(window)
    W = (T + window - 1) // window
    alpha_m, gamma_m, epsilon_m = (learn_ref.per_learner(v, P) for v in (alpha, gamma, epsilon))
    bad_m = learn_ref.bad_learners(alpha_m, gamma_m, epsilon_m)
    member = np.arange(B) // n
    gamma, epsilon, bad = gamma_m[member], epsilon_m[member], bad_m[member]
    first = self.frame if first_frame is None else int(first_frame)
    env = np.arange(B).astype(np.uint64)
    out = dict(reward_sum=np.zeros((W, B), F), perf_sum=np.zeros((W, B), np.int32),
               episodes=np.zeros((W, B), np.int32), clamped=np.zeros(P, np.int64),
               bad=int(bad_m.sum()))
    if record:
      out['states'], out['actions'] = np.zeros((T, B), np.int32), np.zeros((T, B), np.int8)
      out['delta'], out['z'] = np.zeros((T, B), F), np.zeros((T, B), np.int64)
    if reset_first:
      self.over[:] = True
    flat = q.reshape(-1)                       # (a view: q is contiguous)
    with np.errstate(all='ignore'):
      keep = (F(1) - epsilon).astype(F)
      for t in range(T):
        w = t // window
        s = np.where(self.over, 0, self.state)
        x0, x1 = learn_ref.words(seed, env, first + t)
        u = ((x0 >> np.uint32(8)).astype(F) * F(2.0 ** -24)).astype(F)
        explore = u < epsilon
        anywhere = (((x1 >> np.uint32(8)).astype(np.uint64) * np.uint64(5)) >> np.uint64(24)).astype(np.int64)
        _, greedy = plan_ref.reduce_greedy(q[member, s])
        a = np.where(bad, 4, np.where(explore, anywhere, greedy.astype(np.int64)))
        nxt = g.st_next[s, a].astype(np.int64)
        reward = g.st_reward[s, a].astype(F)
        r = np.where(np.isnan(reward), F(0), reward).astype(F)
        done = g.st_done[s, a] != 0
        disc = g.st_discount[s, a].astype(F)
        rows = q[member, np.where(done, 0, nxt)]   # (copies: the table as the frame found it)
        best, _ = plan_ref.reduce_greedy(rows)
        if rule == 'expected_sarsa':
          m = rows[:, 0]
          for k in range(1, N_ACTIONS):
            m = (m + rows[:, k]).astype(F)
          m = (m * F(0.2)).astype(F)
          b = ((keep * best).astype(F) + (epsilon * m).astype(F)).astype(F)
        else:
          b = best
        c = (gamma * disc).astype(F)
        target = np.where(done, r, (r + (c * b).astype(F)).astype(F)).astype(F)
        delta = (target - q[member, s, a]).astype(F)
        z, clamp = quantise(delta)
        good = ~bad
        bins = (member * S + s) * N_ACTIONS + a
        total = np.zeros(P * S * N_ACTIONS, np.int64)
        count = np.zeros(P * S * N_ACTIONS, np.int64)
        np.add.at(total, bins[good], z[good])
        np.add.at(count, bins[good], 1)
        np.add.at(out['clamped'], member[good], clamp[good].astype(np.int64))
        hit = np.flatnonzero(count)
        step = (alpha_m[hit // (S * N_ACTIONS)] * mean_of(total[hit], count[hit])).astype(F)
        flat[hit] = (flat[hit] + step).astype(F)
        out['reward_sum'][w] = (out['reward_sum'][w] + r).astype(F)
        out['perf_sum'][w] += g.st_perf[s, a].astype(np.int32)
        out['episodes'][w] += done.astype(np.int32)
        if record:
          out['states'][t], out['actions'][t] = s, a
          out['delta'][t], out['z'][t] = delta, z
        self.ret = (np.where(self.over, F(0), self.ret).astype(F) + r).astype(F)
        self.state = nxt
        self.over = done
    self.frame = first + T
    return out
