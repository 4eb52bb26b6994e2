"""Online tabular learners (include/campx_hip.h, "Online tabular learners"; csrc/k_learn.hip)
restated in numpy float32, and a host walk of a `tabulate.TracedGame`'s state table under them: the
checker of `WideGame.learn_tabular()`.  Shares no code with the HIP path; the Philox block is
tests/policy_reference.py's and the greedy reduction tests/planning_reference.py's.

The rule, for learner e at absolute frame f, every float32 operation rounded on its own:
  1. one Philox4x32-10 block per learner and pair of frames: key (seed & 0xffffffff, seed >> 32),
     counter (e, g & 0xffffffff, g >> 32, 1) with g = f >> 1; x0 is word 2 * (f & 1), x1 the next;
  2. s = row 0 if the episode is over (or reset_first), else the environment's state;
  3. u = float32(x0 >> 8) * 2^-24; explore iff u < epsilon_e, with action ((x1 >> 8) * 5) >> 24;
     else the greedy action of q[e, s] (`planning_reference.reduce_greedy`);
  4. entry (s, a): next state n, reward r (NaN counted as 0), done, D = the frame's discount;
  5. bootstrap from q[e, n] BEFORE the update: 'q' the greedy maximum `best`; 'expected_sarsa'
     m = ((((q0 + q1) + q2) + q3) + q4) * 0.2, b = (keep * best) + (epsilon_e * m), keep = 1 - epsilon_e;
  6. target = done ? r : r + (gamma_e * D) * b   (`planning_reference.backup`'s arithmetic);
  7. delta = target - q[e, s, a]; q[e, s, a] = q[e, s, a] + alpha_e * delta;
  8. per window: reward_sum += r (float32, frame order), perf_sum += perf, episodes += done.
A learner whose alpha, gamma or epsilon is not finite, or whose epsilon is outside [0, 1], is bad:
it takes action 4 every frame and its table is left untouched.
"""

import numpy as np

import planning_reference as plan_ref
import policy_reference as ref

N_ACTIONS = 5
F = np.float32
RULES = ('q', 'expected_sarsa')
_MASK = np.uint64(0xffffffff)


def words(seed, env, frame):
  """(x0, x1) of learner(s) `env` at absolute frame `frame` (one frame, every learner)."""
  seed = int(seed) & ((1 << 64) - 1)
  env = np.asarray(env, np.uint64)
  g = int(frame) >> 1
  counter = np.stack([env & _MASK, np.full_like(env, g & 0xffffffff), np.full_like(env, g >> 32),
                      np.ones_like(env)], axis=-1).astype(np.uint32)
  block = ref.philox4x32_10(counter, np.array([seed & 0xffffffff, seed >> 32], np.uint32))
  k = 2 * (int(frame) & 1)
  return block[..., k], block[..., k + 1]


def per_learner(value, B):
  return np.broadcast_to(np.asarray(value, F), (B,)).astype(F)


def bad_learners(alpha, gamma, epsilon):
  with np.errstate(all='ignore'):
    return ~(np.isfinite(alpha) & np.isfinite(gamma) & np.isfinite(epsilon)
             & (epsilon >= 0) & (epsilon <= 1))


class Learners(object):
  """B learners on a `TracedGame`'s `st_*` arrays; `q` float32 [B, n_states, 5] is theirs."""

  def __init__(self, game, batch, q=None):
    self.game = game
    self.B = int(batch)
    S = game.n_states
    self.q = np.zeros((self.B, S, N_ACTIONS), F) if q is None else np.array(q, F)
    assert self.q.shape == (self.B, S, N_ACTIONS)
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, F)
    self.frame = 0

  def learn(self, T, alpha=0.1, gamma=0.99, epsilon=0.1, rule='q', seed=0, first_frame=None,
            reset_first=False, window=None, record=False):
    """-> dict(reward_sum float32 [W, B], perf_sum int32 [W, B], episodes int32 [W, B], bad: the bad
    learners, explored [T, B] bool, and - `record` - states, actions [T, B] and the float32 [T, B]
    intermediates delta and step = alpha * delta); `q`, `state`, `over`, `ret` and `frame` carry
    over."""
    assert rule in RULES
    g, B, q = self.game, self.B, self.q
    window = T if window is None else int(window)
    W = (T + window - 1) // window
    alpha, gamma, epsilon = (per_learner(v, B) for v in (alpha, gamma, epsilon))
    bad = bad_learners(alpha, gamma, epsilon)
    first = self.frame if first_frame is None else int(first_frame)
    lanes = np.arange(B)
    env = lanes.astype(np.uint64)
    out = dict(reward_sum=np.zeros((W, B), F), perf_sum=np.zeros((W, B), np.int32),
               episodes=np.zeros((W, B), np.int32), bad=int(bad.sum()),
               explored=np.zeros((T, B), bool))
    if record:
      out['states'], out['actions'] = np.zeros((T, B), np.int32), np.zeros((T, B), np.int8)
      out['delta'], out['step'] = np.zeros((T, B), F), np.zeros((T, B), F)
    if reset_first:
      self.over[:] = True
    with np.errstate(all='ignore'):
      keep = (F(1) - epsilon).astype(F)
      for t in range(T):
        w = t // window
        s = np.where(self.over, 0, self.state)
        x0, x1 = words(seed, env, first + t)
        u = ((x0 >> np.uint32(8)).astype(F) * F(2.0 ** -24)).astype(F)
        explore = u < epsilon
        anywhere = (((x1 >> np.uint32(8)).astype(np.uint64) * np.uint64(5)) >> np.uint64(24)).astype(np.int64)
        _, greedy = plan_ref.reduce_greedy(q[lanes, s])
        a = np.where(bad, 4, np.where(explore, anywhere, greedy.astype(np.int64)))
        n = g.st_next[s, a].astype(np.int64)
        reward = g.st_reward[s, a].astype(F)
        r = np.where(np.isnan(reward), F(0), reward).astype(F)
        done = g.st_done[s, a] != 0
        D = g.st_discount[s, a].astype(F)
        rows = q[lanes, n]                       # (a copy: the rows before this frame's update)
        best, _ = plan_ref.reduce_greedy(rows)
        if rule == 'expected_sarsa':
          m = rows[:, 0]
          for k in range(1, N_ACTIONS):
            m = (m + rows[:, k]).astype(F)
          m = (m * F(0.2)).astype(F)
          b = ((keep * best).astype(F) + (epsilon * m).astype(F)).astype(F)
        else:
          b = best
        c = (gamma * D).astype(F)
        target = np.where(done, r, (r + (c * b).astype(F)).astype(F)).astype(F)
        old = q[lanes, s, a]
        delta = (target - old).astype(F)
        step = (alpha * delta).astype(F)
        fresh = (old + step).astype(F)
        q[lanes, s, a] = np.where(bad, old, fresh)
        out['reward_sum'][w] = (out['reward_sum'][w] + r).astype(F)
        out['perf_sum'][w] += g.st_perf[s, a].astype(np.int32)
        out['episodes'][w] += done.astype(np.int32)
        out['explored'][t] = explore & ~bad
        if record:
          out['states'][t], out['actions'][t] = s, a
          out['delta'][t], out['step'][t] = delta, step
        self.ret = (np.where(self.over, F(0), self.ret).astype(F) + r).astype(F)
        self.state = n
        self.over = done
    self.frame = first + T
    return out
