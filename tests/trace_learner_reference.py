"""Online learners with eligibility traces (include/campx_hip.h, "Online learners with eligibility
traces"; csrc/k_learn.hip) restated in numpy float32, operation by operation: the checker of
`WideGame.learn_traces()`.  Built on tests/learner_reference.py's walker - its learners, its Philox
words, its test of a bad learner - and sharing no code with the HIP path.

The frame of a good learner e in state s, table q, traces z (each [n_states * 5] here), every
float32 operation rounded on its own:
  1. act: row = q[s]; a = the epsilon-greedy action of learner_reference; old = row[a]; best = the
     greedy maximum of row;
  2. cut: rule 'q' (Watkins) - if not (old == best), a NaN included, z[:] = +0; 'expected_sarsa'
     never cuts;
  3. TD error: entry (s, a) -> n, r, done, D; delta = target - old, the bootstrap from q[n] as the
     table stands now;
  4. bump: 'accumulating' z[s, a] = z[s, a] + 1; 'replacing' z[s, a] = 1;
  5. sweep: step = alpha * delta; for every i with z[i] != 0 (a NaN counts):
     q[i] = q[i] + (step * z[i]); an entry whose trace is +-0 keeps its bits;
  6. decay: done - z[:] = +0; else c = (gamma * D) * lam and z[i] = c * z[i] for every i;
  7. state, done, ret and the window sums as in learner_reference.
`reset_first` zeroes a good learner's traces before frame 0.  A learner that learner_reference
calls bad, or whose lam is not within [0, 1], takes action 4 and keeps q and z untouched.
"""

import numpy as np

import learner_reference as learn_ref
import planning_reference as plan_ref

N_ACTIONS = learn_ref.N_ACTIONS
F = np.float32
RULES = learn_ref.RULES
KINDS = ('accumulating', 'replacing')


def bad_learners(alpha, gamma, epsilon, lam):
  with np.errstate(all='ignore'):
    return learn_ref.bad_learners(alpha, gamma, epsilon) | ~((lam >= 0) & (lam <= 1))


class TraceLearners(learn_ref.Learners):
  """B learners with a trace per (state, action): `q` and `z` float32 [B, n_states, 5]."""

  def __init__(self, game, batch, q=None, z=None):
    super(TraceLearners, self).__init__(game, batch, q)
    self.z = np.zeros_like(self.q) if z is None else np.array(z, F)
    assert self.z.shape == self.q.shape

  def learn_traces(self, T, lam=0.9, trace='accumulating', alpha=0.1, gamma=0.99, epsilon=0.1,
                   rule='q', seed=0, first_frame=None, reset_first=False, window=None, record=False):
    """-> learner_reference's dict (`record`: states, actions, delta, step and cut [T, B], touched
    [B, n_states * 5]); `q`, `z`, `state`, `over`, `ret` and `frame` carry over."""
    assert rule in RULES and trace in KINDS
    g, B = self.game, self.B
    q, z = self.q.reshape(B, -1), self.z.reshape(B, -1)            # (views: updated in place)
    window = T if window is None else int(window)
    W = (T + window - 1) // window
    alpha, gamma, epsilon, lam = (learn_ref.per_learner(v, B) for v in (alpha, gamma, epsilon, lam))
    bad = bad_learners(alpha, gamma, epsilon, lam)
    good = ~bad
    first = self.frame if first_frame is None else int(first_frame)
    lanes = np.arange(B)
    env = lanes.astype(np.uint64)
    out = dict(reward_sum=np.zeros((W, B), F), perf_sum=np.zeros((W, B), np.int32),
               episodes=np.zeros((W, B), np.int32), bad=int(bad.sum()),
               explored=np.zeros((T, B), bool))
    if record:
      out['states'], out['actions'] = np.zeros((T, B), np.int32), np.zeros((T, B), np.int8)
      out['delta'], out['step'] = np.zeros((T, B), F), np.zeros((T, B), F)
      out['cut'] = np.zeros((T, B), bool)
      out['touched'] = np.zeros(q.shape, bool)         # entries of q that some sweep wrote
    if reset_first:
      self.over[:] = True
      z[good] = F(0)
    with np.errstate(all='ignore'):
      keep = (F(1) - epsilon).astype(F)
      for t in range(T):
        w = t // window
        s = np.where(self.over, 0, self.state)
        x0, x1 = learn_ref.words(seed, env, first + t)
        u = ((x0 >> np.uint32(8)).astype(F) * F(2.0 ** -24)).astype(F)
        explore = u < epsilon
        anywhere = (((x1 >> np.uint32(8)).astype(np.uint64) * np.uint64(5)) >> np.uint64(24)).astype(np.int64)
        row = self.q[lanes, s]
        best_here, greedy = plan_ref.reduce_greedy(row)
        a = np.where(bad, 4, np.where(explore, anywhere, greedy.astype(np.int64)))
        old = self.q[lanes, s, a]
        # 2. cut
        cut = good & ~(old == best_here) if rule == 'q' else np.zeros(B, bool)
        z[cut] = F(0)
        # 3. TD error
        n = g.st_next[s, a].astype(np.int64)
        reward = g.st_reward[s, a].astype(F)
        r = np.where(np.isnan(reward), F(0), reward).astype(F)
        done = g.st_done[s, a] != 0
        D = g.st_discount[s, a].astype(F)
        rows = self.q[lanes, n]
        best, _ = plan_ref.reduce_greedy(rows)
        if rule == 'expected_sarsa':
          m = rows[:, 0]
          for k in range(1, N_ACTIONS):
            m = (m + rows[:, k]).astype(F)
          m = (m * F(0.2)).astype(F)
          b = ((keep * best).astype(F) + (epsilon * m).astype(F)).astype(F)
        else:
          b = best
        gd = (gamma * D).astype(F)
        target = np.where(done, r, (r + (gd * b).astype(F)).astype(F)).astype(F)
        delta = (target - old).astype(F)
        # 4. bump
        idx = s * N_ACTIONS + a
        bumped = (z[lanes, idx] + F(1)).astype(F) if trace == 'accumulating' else np.ones(B, F)
        z[lanes, idx] = np.where(good, bumped, z[lanes, idx])
        # 5. sweep
        step = (alpha * delta).astype(F)
        move = (step[:, None] * z).astype(F)
        touched = (z != 0) & good[:, None]
        q[touched] = (q + move).astype(F)[touched]
        if record:
          out['touched'] |= touched
        # 6. decay
        c = (gd * lam).astype(F)
        decayed = np.where(done[:, None], F(0), (c[:, None] * z).astype(F)).astype(F)
        z[good] = decayed[good]
        out['reward_sum'][w] = (out['reward_sum'][w] + r).astype(F)
        out['perf_sum'][w] += g.st_perf[s, a].astype(np.int32)
        out['episodes'][w] += done.astype(np.int32)
        out['explored'][t] = explore & good
        if record:
          out['states'][t], out['actions'][t] = s, a
          out['delta'][t], out['step'][t], out['cut'][t] = delta, step, cut
        self.ret = (np.where(self.over, F(0), self.ret).astype(F) + r).astype(F)
        self.state = n
        self.over = done
    self.frame = first + T
    return out
