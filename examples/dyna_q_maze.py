#!/usr/bin/env python3
"""Dyna-Q on the 16x16 maze: a sweep of the planning updates per frame (`learn_dyna()`), one setting
per block of the batch, every other hyper-parameter shared.  planning = 0 is the one-step learner
of examples/q_learning_sweep.py: the reward at the goal moves back one state per episode.  With n
planning updates a frame the learner replays pairs it has already visited - their transitions are
the game's own table - and the reward reaches the start within a few frames of the first goal:
more learning per frame of experience.

Every environment is its own learner with its own Q-table and its own model (the list of the pairs
it has met); learner i * seeds + k is seed k of `plannings[i]`.  The run is ONE launch of `frames`
frames; the learning curves are its window sums - no [T, B] stream is written.

Per setting the script prints one line: the episodes its learners finished in every window, summed
over the setting's learners.

    python examples/dyna_q_maze.py --frames 4000 --window 500

A consumer of the engine, not part of it; tested in tests/test_example_dyna.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import maze  # noqa: E402

PLANNINGS = (0, 5, 50)


def run(plannings=PLANNINGS, seeds=64, frames=4000, window=500, alpha=0.5, gamma=0.95, epsilon=0.3,
        rule='q', seed=0, device='cuda'):
  """-> dict: 'q' [B, S, 5]; 'model' (seen [B, S * 5], n_seen [B]); 'planning' [B]; 'episodes'
  [len(plannings), W], the episodes that ended per window, summed over a setting's learners;
  'reward' the same of the reward."""
  B = len(plannings) * seeds
  game = maze.build(16, 16, batch=B, device=device)
  game.its_showtime()
  planning = torch.tensor([n for n in plannings for _ in range(seeds)], dtype=torch.int32,
                          device=device)
  res = game.learn_dyna(frames, planning=planning, alpha=alpha, gamma=gamma, epsilon=epsilon,
                        rule=rule, seed=seed, reset_first=True, window=window)
  game.fused.check_actions()
  W = res['episodes'].shape[0]
  cells = (W, len(plannings), seeds)
  return {'q': res['q'], 'model': res['model'], 'planning': planning,
          'episodes': res['episodes'].view(cells).sum(2).t(),
          'reward': res['reward_sum'].view(cells).sum(2).t()}


def lines(plannings, episodes):
  return ['planning {:4d}  episodes per window {}  total {}'.format(
      n, ' '.join('{:5d}'.format(int(x)) for x in episodes[i]), int(episodes[i].sum()))
          for i, n in enumerate(plannings)]


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--seeds', type=int, default=64)
  p.add_argument('--frames', type=int, default=4000)
  p.add_argument('--window', type=int, default=500)
  p.add_argument('--alpha', type=float, default=0.5)
  p.add_argument('--gamma', type=float, default=0.95)
  p.add_argument('--epsilon', type=float, default=0.3)
  p.add_argument('--rule', default='q', choices=['q', 'expected_sarsa'])
  args = p.parse_args()
  r = run(seeds=args.seeds, frames=args.frames, window=args.window, alpha=args.alpha, gamma=args.gamma,
          epsilon=args.epsilon, rule=args.rule)
  for line in lines(PLANNINGS, r['episodes'].cpu()):
    print(line)
