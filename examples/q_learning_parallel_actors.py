#!/usr/bin/env python3
"""How many parallel actors should feed one Q-learner?  A sweep of n = 1, 16 and 256 actors per
learner on the boat race, the same number of frames each.

`learn_shared()` runs P learners of n actors each in one launch: within a frame every actor of a
learner acts on the same table, the TD errors are summed per (state, action) in fixed point, and the
table moves once, by alpha times their mean - so the step size does not depend on n, and a run
repeats bit for bit.  Each n gets a game of its own with `learners` learners, B = learners * n
environments.

Per n and learner the script prints the reward and the hidden performance per actor and frame of
the run's last window, and the exact discounted return of the learner's greedy policy from the
start state through `evaluate_population()` - on the boat race the policy that the reward points to
is not the one the hidden performance favours.

    python examples/q_learning_parallel_actors.py --learners 4 --frames 2000

A consumer of the engine, not part of it; tested in tests/test_example_parallel_actors.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402

ACTORS = (1, 16, 256)


def run_one(n, learners=4, frames=1000, window=None, alpha=0.1, gamma=0.9, epsilon=0.1, rule='q',
            seed=0, sweeps=400, device='cuda'):
  """-> dict for `learners` learners of n actors: 'q' [P, S, 5]; 'reward' and 'perf' [P], per actor
  and frame of the last window; 'greedy_return' [P], the exact return of each greedy policy from
  state 0; 'clamped' [P]."""
  P, B = learners, learners * n
  game = boat_race.build(B, device)
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  window = frames if window is None else window
  q = torch.zeros((P, S, 5), device=device)
  res = game.learn_shared(frames, q, alpha=alpha, gamma=gamma, epsilon=epsilon, rule=rule, seed=seed,
                          reset_first=True, window=window)
  last = frames - (frames - 1) // window * window          # frames of the last window
  greedy = torch.nn.functional.one_hot(q.argmax(2), 5).float()
  values = game.evaluate_population(greedy, gamma, sweeps)['values']
  game.fused.check_actions()
  return {'q': q,
          'reward': res['reward_sum'][-1].view(P, n).mean(1) / last,
          'perf': res['perf_sum'][-1].float().view(P, n).mean(1) / last,
          'greedy_return': values[:, 0], 'clamped': res['clamped']}


def run(actors=ACTORS, **kwargs):
  return {n: run_one(n, **kwargs) for n in actors}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--learners', type=int, default=4)
  p.add_argument('--frames', type=int, default=1000)
  p.add_argument('--alpha', type=float, default=0.1)
  p.add_argument('--gamma', type=float, default=0.9)
  p.add_argument('--epsilon', type=float, default=0.1)
  p.add_argument('--rule', default='q', choices=['q', 'expected_sarsa'])
  args = p.parse_args()
  results = run(learners=args.learners, frames=args.frames, alpha=args.alpha, gamma=args.gamma,
                epsilon=args.epsilon, rule=args.rule)
  print('actors  learner  reward/frame  performance/frame  greedy policy\'s return')
  for n, r in results.items():
    for m in range(args.learners):
      print('{:6d}  {:7d}  {:12.3f}  {:17.3f}  {:22.3f}'.format(
          n, m, float(r['reward'][m]), float(r['perf'][m]), float(r['greedy_return'][m])))
