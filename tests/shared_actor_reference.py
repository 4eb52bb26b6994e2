"""Shared actor-critic learners (include/campx_hip.h, "Shared actor-critic learners";
csrc/k_learn.hip) restated in numpy, and a host walk of a `tabulate.TracedGame`'s state table
under them: the checker of `WideGame.learn_actor_critic_shared()`.  Shares no code with the HIP
path; the softmax rule is tests/actor_critic_reference.py's, the sampler and its words
tests/policy_reference.py's, the quantiser and the mean tests/shared_learner_reference.py's.

P learners; learner m owns prefs[m] and values[m] and is fed by the n = B / P environments
[m * n, (m + 1) * n).  Frame f of learner m, every float32 operation rounded on its own; every
actor reads both tables as they stand at the START of the frame:
  (A) per actor in state s: w = the softmax rule of prefs[m, s]; the action by
      policy_reference.sample() on policy_reference.words(); a row that is not good takes action 4
      and contributes nothing (counted in 'bad_rows'); else with the entry's n, r, done, D
      delta = (done ? r : r + (gamma_m * D) * values[m, n]) - values[m, s];
      z = quantise(delta) (NaN -> 0, beyond 2^52 clamped, both counted in clamped[m]);
      Z[m, s, a] += z; N[m, s] += 1;
  (B) per (m, s) with N >= 1: Zall = sum_k Z[k] (int64); mean_k = mean_of(Z[k], N); mean_all =
      mean_of(Zall, N); values[m, s] += alpha_critic_m * mean_all; for each k: pi = w[k] / c4,
      grad = mean_k - pi * mean_all, prefs[m, s, k] += alpha_actor_m * grad.
A learner whose alpha_actor, alpha_critic or gamma is not finite is bad: all its environments take
action 4 every frame, nothing of it changes, nothing is accumulated (counted in 'bad').
"""

import numpy as np

import actor_critic_reference as actor_ref
import learner_reference as learn_ref
import policy_reference as ref
import shared_learner_reference as shared_ref

N_ACTIONS = 5
F = np.float32
quantise = shared_ref.quantise
mean_of = shared_ref.mean_of


class SharedActorCritics(object):
  """P learners on a `TracedGame`'s `st_*` arrays, fed by B environments; `prefs` float32
  [P, n_states, 5] and `values` float32 [P, n_states] are theirs."""

  def __init__(self, game, batch, prefs, values):
    self.game = game
    self.B = int(batch)
    self.prefs = np.array(prefs, F)
    self.values = np.array(values, F)
    self.P = self.prefs.shape[0]
    assert self.prefs.shape == (self.P, game.n_states, N_ACTIONS) and self.B % self.P == 0
    assert self.values.shape == (self.P, game.n_states)
    self.n = self.B // self.P
    assert 1 <= self.n <= 1024
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, F)
    self.frame = 0

  def learn(self, T, alpha_actor=0.1, alpha_critic=0.1, gamma=0.99, seed=0, first_frame=None,
            reset_first=False, window=None, record=False, order=None, delta_override=None):
    """-> dict(reward_sum float32 [W, B], perf_sum int32 [W, B], episodes int32 [W, B], clamped
    int64 [P], bad: the bad learners, bad_rows: environment-frames of good learners that met a row
    that is not good, and - `record` - states, actions [T, B], delta float32 [T, B] and z int64
    [T, B]); `prefs`, `values`, `state`, `over`, `ret` and `frame` carry over.  `order`: the
    permutation of the environments in which their contributions are accumulated (default:
    ascending).  `delta_override`: float32 [T, B] that replaces the frames' errors where it is
    not None - the quantiser's edges, which no table reaches by itself."""
    g, B, P, n = self.game, self.B, self.P, self.n
    S = g.n_states
    window = T if window is None else int(window)
    W = (T + window - 1) // window
    aa_m, ac_m, gamma_m = (learn_ref.per_learner(v, P) for v in (alpha_actor, alpha_critic, gamma))
    bad_m = ~(np.isfinite(aa_m) & np.isfinite(ac_m) & np.isfinite(gamma_m))
    member = np.arange(B) // n
    gam, bad = gamma_m[member], bad_m[member]
    order = np.arange(B) if order is None else np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(B))
    first = self.frame if first_frame is None else int(first_frame)
    env = np.arange(B).astype(np.uint64)
    out = dict(reward_sum=np.zeros((W, B), F), perf_sum=np.zeros((W, B), np.int32),
               episodes=np.zeros((W, B), np.int32), clamped=np.zeros(P, np.int64),
               bad=int(bad_m.sum()), bad_rows=0)
    if record:
      out['states'], out['actions'] = np.zeros((T, B), np.int32), np.zeros((T, B), np.int8)
      out['delta'], out['z'] = np.zeros((T, B), F), np.zeros((T, B), np.int64)
    if reset_first:
      self.over[:] = True
    h_flat = self.prefs.reshape(P * S, N_ACTIONS)        # (views: both are contiguous)
    v_flat = self.values.reshape(P * S)
    with np.errstate(all='ignore'):
      for t in range(T):
        s = np.where(self.over, 0, self.state)
        cell = member * S + s
        w, row_good = actor_ref.softmax_weights(h_flat[cell])
        acts = row_good & ~bad
        w = np.where(acts[:, None], w, F(0)).astype(F)
        a, _ = ref.sample(ref.words(seed, env, first + t), w)
        a = a.astype(np.int64)
        assert (a[~acts] == 4).all()
        out['bad_rows'] += int((~row_good & ~bad).sum())
        nxt = g.st_next[s, a].astype(np.int64)
        reward = g.st_reward[s, a].astype(F)
        r = np.where(np.isnan(reward), F(0), reward).astype(F)
        done = g.st_done[s, a] != 0
        disc = g.st_discount[s, a].astype(F)
        v_s = v_flat[cell]                              # (copies: the tables as the frame found them)
        v_n = v_flat[member * S + np.where(done, 0, nxt)]
        c = (gam * disc).astype(F)
        target = np.where(done, r, (r + (c * v_n).astype(F)).astype(F)).astype(F)
        delta = (target - v_s).astype(F)
        if delta_override is not None:
          delta = np.asarray(delta_override, F)[t]
        z, clamp = quantise(delta)
        total = np.zeros(P * S * N_ACTIONS, np.int64)
        count = np.zeros(P * S, np.int64)
        who = order[acts[order]]
        np.add.at(total, cell[who] * N_ACTIONS + a[who], z[who])
        np.add.at(count, cell[who], 1)
        np.add.at(out['clamped'], member[who], clamp[who].astype(np.int64))
        hit = np.flatnonzero(count)
        Z = total.reshape(P * S, N_ACTIONS)[hit]
        N = count[hit]
        mean_all = mean_of(Z.sum(axis=1), N)
        h = h_flat[hit]
        w_hit, good_hit = actor_ref.softmax_weights(h)
        assert good_hit.all()
        c4 = ref.thresholds(w_hit)[0][:, 4]
        m_hit = hit // S
        v_flat[hit] = (v_flat[hit] + (ac_m[m_hit] * mean_all).astype(F)).astype(F)
        for k in range(N_ACTIONS):
          pi = (w_hit[:, k] / c4).astype(F)
          grad = (mean_of(Z[:, k], N) - (pi * mean_all).astype(F)).astype(F)
          h_flat[hit, k] = (h[:, k] + (aa_m[m_hit] * grad).astype(F)).astype(F)
        w_at = t // window
        out['reward_sum'][w_at] = (out['reward_sum'][w_at] + r).astype(F)
        out['perf_sum'][w_at] += g.st_perf[s, a].astype(np.int32)
        out['episodes'][w_at] += done.astype(np.int32)
        if record:
          out['states'][t], out['actions'][t] = s, a
          out['delta'][t], out['z'][t] = delta, z
        self.ret = (np.where(self.over, F(0), self.ret).astype(F) + r).astype(F)
        self.state = nxt
        self.over = done
    self.frame = first + T
    return out
