"""Dyna-Q online learners (include/campx_hip.h, "Dyna-Q online learners"; csrc/k_learn.hip) restated
in numpy float32, operation by operation: the checker of `WideGame.learn_dyna()`.  Built on
tests/learner_reference.py's walker - its learners, its exploration words, its test of a bad
learner - and sharing no code with the HIP path; the Philox block is tests/policy_reference.py's.

Learner e owns q[e] and a model: the first n_seen[e] elements of seen[e] (int32 [n_states * 5]) are
the flat entries s * 5 + a it has met, in order of first visit.  Frame f of a good learner:
  1. the real step: learner_reference's steps 1 - 7, q[e, s, a] updated;
  2. record: i = s * 5 + a joins the list if it is not among its first n_seen elements (and the
     list is not already n_states * 5 long);
  3. plan, k = 0 .. planning[e] - 1, one after the other: x = word k & 3 of the Philox block of
     key `seed`, counter (e, f & 0xffffffff, f >> 32, 2 + (k >> 2)); idx = (x * n_seen) >> 32;
     i = seen[idx]; the table's entry i gives n, r, done, D; the bootstrap from q[e, n] as it
     stands; q[e, i] = q[e, i] + alpha * (target - q[e, i]);
  4. state, done, ret and the window sums as in learner_reference.
A learner that learner_reference calls bad, or whose planning is outside 0 .. 1024, or whose list at
the start of the call has n_seen outside 0 .. n_states * 5 or a listed element outside the table,
takes action 4 at every frame and keeps q, seen and n_seen untouched.
"""

import numpy as np

import learner_reference as learn_ref
import planning_reference as plan_ref
import policy_reference as ref

N_ACTIONS = learn_ref.N_ACTIONS
F = np.float32
RULES = learn_ref.RULES
MAX_PLANNING = 1024


def planning_words(seed, env, frame, block):
  """uint32 [..., 4]: block `block` (k >> 2) of the planning stream of learner(s) `env` at absolute
  frame `frame`."""
  seed = int(seed) & ((1 << 64) - 1)
  env = np.asarray(env, np.uint64)
  f = int(frame)
  counter = np.stack([env & np.uint64(0xffffffff), np.full_like(env, f & 0xffffffff),
                      np.full_like(env, f >> 32), np.full_like(env, 2 + int(block))],
                     axis=-1).astype(np.uint32)
  return ref.philox4x32_10(counter, np.array([seed & 0xffffffff, seed >> 32], np.uint32))


def bad_models(seen, n_seen, n_entries):
  """Learners whose list does not pass the screening."""
  n = n_seen.astype(np.int64)
  count_ok = (n >= 0) & (n <= n_entries)
  listed = np.arange(seen.shape[1])[None, :] < np.where(count_ok, n, 0)[:, None]
  outside = (seen < 0) | (seen >= n_entries)
  return ~count_ok | (listed & outside).any(axis=1)


class DynaLearners(learn_ref.Learners):
  """B Dyna-Q learners: `q` float32 [B, n_states, 5], `seen` int32 [B, n_states * 5], `n_seen`
  int32 [B]."""

  def __init__(self, game, batch, q=None, seen=None, n_seen=None):
    super(DynaLearners, self).__init__(game, batch, q)
    E = game.n_states * N_ACTIONS
    self.seen = np.zeros((self.B, E), np.int32) if seen is None else np.array(seen, np.int32)
    self.n_seen = np.zeros(self.B, np.int32) if n_seen is None else np.array(n_seen, np.int32)
    assert self.seen.shape == (self.B, E) and self.n_seen.shape == (self.B,)

  def _target(self, rows, r, done, D, rule, gamma, epsilon, keep):
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
    return np.where(done, r, (r + (c * b).astype(F)).astype(F)).astype(F)

  def learn_dyna(self, T, planning=5, alpha=0.1, gamma=0.99, epsilon=0.1, rule='q', seed=0,
                 first_frame=None, reset_first=False, window=None, record=False):
    """-> learner_reference's dict (`record`: states, actions [T, B] and planned, a list per frame
    of int64 [n_max, B] - the flat entry each planning step updated, -1 where none);
    `q`, `seen`, `n_seen`, `state`, `over`, `ret` and `frame` carry over."""
    assert rule in RULES
    g, B = self.game, self.B
    S = g.n_states
    E = S * N_ACTIONS
    q = self.q.reshape(B, E)                               # (a view: updated in place)
    window = T if window is None else int(window)
    W = (T + window - 1) // window
    alpha, gamma, epsilon = (learn_ref.per_learner(v, B) for v in (alpha, gamma, epsilon))
    planning = np.broadcast_to(np.asarray(planning, np.int64), (B,)).copy()
    bad = (learn_ref.bad_learners(alpha, gamma, epsilon) | (planning < 0) | (planning > MAX_PLANNING)
           | bad_models(self.seen, self.n_seen, E))
    good = ~bad
    n_max = int(planning[good].max()) if good.any() else 0
    first = self.frame if first_frame is None else int(first_frame)
    lanes = np.arange(B)
    env = lanes.astype(np.uint64)
    # the table by flat entry
    t_next = g.st_next.reshape(E).astype(np.int64)
    t_reward = g.st_reward.reshape(E).astype(F)
    t_reward = np.where(np.isnan(t_reward), F(0), t_reward).astype(F)
    t_done = g.st_done.reshape(E) != 0
    t_D = g.st_discount.reshape(E).astype(F)
    t_perf = g.st_perf.reshape(E).astype(np.int32)
    out = dict(reward_sum=np.zeros((W, B), F), perf_sum=np.zeros((W, B), np.int32),
               episodes=np.zeros((W, B), np.int32), bad=int(bad.sum()))
    if record:
      out['states'], out['actions'] = np.zeros((T, B), np.int32), np.zeros((T, B), np.int8)
      out['planned'] = []
    if reset_first:
      self.over[:] = True
    with np.errstate(all='ignore'):
      keep = (F(1) - epsilon).astype(F)
      for t in range(T):
        w = t // window
        s = np.where(self.over, 0, self.state)
        x0, x1 = learn_ref.words(seed, env, first + t)
        u = ((x0 >> np.uint32(8)).astype(F) * F(2.0 ** -24)).astype(F)
        explore = u < epsilon
        anywhere = (((x1 >> np.uint32(8)).astype(np.uint64) * np.uint64(5)) >> np.uint64(24)).astype(np.int64)
        _, greedy = plan_ref.reduce_greedy(self.q[lanes, s])
        a = np.where(bad, 4, np.where(explore, anywhere, greedy.astype(np.int64)))
        # 1. the real step
        i = s * N_ACTIONS + a
        n, r, done = t_next[i], t_reward[i], t_done[i]
        target = self._target(self.q[lanes, n], r, done, t_D[i], rule, gamma, epsilon, keep)
        old = q[lanes, i]
        fresh = (old + (alpha * (target - old).astype(F)).astype(F)).astype(F)
        q[lanes, i] = np.where(bad, old, fresh)
        # 2. record
        count = self.n_seen.astype(np.int64)
        listed = np.arange(E)[None, :] < count[:, None]
        new = good & ~((self.seen == i[:, None]) & listed).any(axis=1) & (count < E)
        self.seen[lanes[new], count[new]] = i[new]
        self.n_seen[new] += 1
        # 3. plan
        count = np.where(good, self.n_seen, 0).astype(np.uint64)
        planned = np.full((n_max, B), -1, np.int64)
        for k in range(n_max):
          if k & 3 == 0:
            block = planning_words(seed, env, first + t, k >> 2)
          active = good & (k < planning)
          x = block[:, k & 3].astype(np.uint64)
          at = ((x * count) >> np.uint64(32)).astype(np.int64)
          j = np.where(active, self.seen[lanes, at], 0).astype(np.int64)
          target = self._target(self.q[lanes, t_next[j]], t_reward[j], t_done[j], t_D[j], rule, gamma,
                                epsilon, keep)
          old = q[lanes, j]
          fresh = (old + (alpha * (target - old).astype(F)).astype(F)).astype(F)
          q[lanes, j] = np.where(active, fresh, old)
          planned[k] = np.where(active, j, -1)
        # 4. advance
        out['reward_sum'][w] = (out['reward_sum'][w] + r).astype(F)
        out['perf_sum'][w] += t_perf[i]
        out['episodes'][w] += done.astype(np.int32)
        if record:
          out['states'][t], out['actions'][t] = s, a
          out['planned'].append(planned)
        self.ret = (np.where(self.over, F(0), self.ret).astype(F) + r).astype(F)
        self.state = n
        self.over = done
    self.frame = first + T
    return out
