#!/usr/bin/env python3
"""A sweep of online Q-learners on the boat race: how often does a learner end up where the reward
points - round and round past the same two arrows, reward up, hidden performance down - as a
function of its exploration rate, its step size and its seed?

Every environment is its own learner with its own Q-table (`learn_tabular()`): 4 096 of them by
default, a grid of 16 epsilons x 16 alphas with 16 seeds each.  Learner e draws its own random
numbers (the Philox counter holds e), so the 16 learners of a cell differ by seed alone.  The run is
a few calls of `learn_tabular()`, epsilon decaying between calls, each call one launch; no [T, B]
stream is ever written.  `value_iteration()` gives q* once, and with it the reward-optimal greedy
action of every state where q* decides (best and second-best differ).

Per cell of the grid the script prints the share of learners whose greedy policy is the
reward-optimal one in every decided state, and the mean reward and mean hidden performance per
frame of the run's last window.

    python examples/q_learning_sweep.py --calls 6 --frames 2000

A consumer of the engine, not part of it; tested in tests/test_example_q_learning.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402

EPSILONS = tuple(round(0.05 * (i + 1), 2) for i in range(16))          # 0.05 .. 0.8
ALPHAS = tuple(round(0.02 * 1.3 ** i, 4) for i in range(16))           # 0.02 .. 1.02


def grid(epsilons, alphas, seeds):
  """(epsilon, alpha) of every learner: learner (i * len(alphas) + j) * seeds + k is seed k of cell
  (epsilons[i], alphas[j])."""
  eps = [e for e in epsilons for _ in alphas for _ in range(seeds)]
  alpha = [a for _ in epsilons for a in alphas for _ in range(seeds)]
  return eps, alpha


def schedule(eps, decay, call):
  """The learners' epsilons during call `call`: epsilon * decay ^ call, rounded to float32 once."""
  return torch.tensor([e * decay ** call for e in eps], dtype=torch.float32)


def run(epsilons=EPSILONS, alphas=ALPHAS, seeds=16, calls=4, frames=1000, gamma=0.9, decay=0.5,
        window=None, rule='q', seed=0, sweeps=400, device='cuda'):
  """-> dict: 'q' [B, S, 5]; 'optimal' [S] and 'decided' [S] from q*; 'agrees' [B] bool; per cell
  [len(epsilons), len(alphas)]: 'share', 'reward', 'perf'."""
  eps, alpha = grid(epsilons, alphas, seeds)
  B = len(eps)
  game = boat_race.build(B, device)
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  window = frames if window is None else window
  q = torch.zeros((B, S, 5), device=device)
  alpha_t = torch.tensor(alpha, dtype=torch.float32, device=device)
  gamma_t = torch.full((B,), gamma, dtype=torch.float32, device=device)
  eps_t = torch.empty((B,), dtype=torch.float32, device=device)
  out = game.learner_buffers(frames, window)
  for call in range(calls):
    eps_t.copy_(schedule(eps, decay, call))
    res = game.learn_tabular(frames, q, alpha_t, gamma_t, eps_t, rule=rule, seed=seed,
                             reset_first=call == 0, window=window, out=out)
  # q*: where its best and second-best action differ, the reward-optimal action is decided
  best = game.value_iteration(gamma, sweeps)
  top = best['q'].sort(dim=1, descending=True).values
  decided = top[:, 0] != top[:, 1]
  optimal = best['greedy'].long()
  agrees = ((q.argmax(2) == optimal) | ~decided).all(1)
  last = frames - (frames - 1) // window * window        # frames of the last window
  cells = (len(epsilons), len(alphas), seeds)
  game.fused.check_actions()
  return {'q': q, 'optimal': optimal, 'decided': decided, 'agrees': agrees,
          'share': agrees.float().view(cells).mean(2),
          'reward': res['reward_sum'][-1].view(cells).mean(2) / last,
          'perf': res['perf_sum'][-1].float().view(cells).mean(2) / last}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--seeds', type=int, default=16)
  p.add_argument('--calls', type=int, default=4)
  p.add_argument('--frames', type=int, default=1000)
  p.add_argument('--gamma', type=float, default=0.9)
  p.add_argument('--decay', type=float, default=0.5)
  p.add_argument('--rule', default='q', choices=['q', 'expected_sarsa'])
  args = p.parse_args()
  r = run(seeds=args.seeds, calls=args.calls, frames=args.frames, gamma=args.gamma, decay=args.decay,
          rule=args.rule)
  print('reward-optimal greedy actions {} (decided in states {})'.format(
      r['optimal'].tolist(), r['decided'].nonzero().view(-1).tolist()))
  print('epsilon  alpha    share optimal  reward/frame  performance/frame')
  for i, e in enumerate(EPSILONS):
    for j, a in enumerate(ALPHAS):
      print('{:7.2f}  {:6.4f}  {:13.3f}  {:12.3f}  {:17.3f}'.format(
          e, a, float(r['share'][i, j]), float(r['reward'][i, j]), float(r['perf'][i, j])))
