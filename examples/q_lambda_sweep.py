#!/usr/bin/env python3
"""A sweep of lambda on the boat race: learners with eligibility traces (`learn_traces()`), one value
of lambda per block of the batch, every other hyper-parameter shared.  lambda = 0 is the one-step
learner of examples/q_learning_sweep.py; the larger lambda, the further back along the path a
reward reaches in the frame it arrives.

Every environment is its own learner with its own Q-table and its own traces; learner
i * seeds + k is seed k of `lambdas[i]` (the Philox counter holds the learner, so the learners of
a lambda differ by seed alone).  The run is ONE launch of `frames` frames; the learning curves
are its window sums - no [T, B] stream is written.

Per lambda the script prints one row per window: the mean reward per frame and the mean hidden
performance per frame over the lambda's learners - the boat race rewards circling past two arrows
and hides that the boat should go round the track.

    python examples/q_lambda_sweep.py --frames 2000 --window 250

A consumer of the engine, not part of it; tested in tests/test_example_q_lambda.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402

LAMBDAS = (0.0, 0.3, 0.6, 0.8, 0.9, 0.95, 1.0)


def run(lambdas=LAMBDAS, seeds=64, frames=2000, window=250, alpha=0.1, gamma=0.9, epsilon=0.1,
        rule='q', trace='accumulating', seed=0, device='cuda'):
  """-> dict: 'q', 'traces' [B, S, 5]; 'lam' [B]; per lambda and window, [len(lambdas), W]:
  'reward' and 'perf' per frame, 'episodes' per learner."""
  B = len(lambdas) * seeds
  game = boat_race.build(B, device)
  game.use_state_table()
  game.its_showtime()
  lam = torch.tensor([l for l in lambdas for _ in range(seeds)], dtype=torch.float32, device=device)
  res = game.learn_traces(frames, lam=lam, trace=trace, alpha=alpha, gamma=gamma, epsilon=epsilon,
                          rule=rule, seed=seed, reset_first=True, window=window)
  game.fused.check_actions()
  W = res['reward_sum'].shape[0]
  # frames of every window: the last may be short
  length = torch.full((W,), float(window), device=device)
  length[-1] = frames - (W - 1) * window
  cells = (W, len(lambdas), seeds)
  return {'q': res['q'], 'traces': res['traces'], 'lam': lam,
          'reward': (res['reward_sum'].view(cells).mean(2) / length[:, None]).t(),
          'perf': (res['perf_sum'].float().view(cells).mean(2) / length[:, None]).t(),
          'episodes': res['episodes'].float().view(cells).mean(2).t()}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--seeds', type=int, default=64)
  p.add_argument('--frames', type=int, default=2000)
  p.add_argument('--window', type=int, default=250)
  p.add_argument('--alpha', type=float, default=0.1)
  p.add_argument('--gamma', type=float, default=0.9)
  p.add_argument('--epsilon', type=float, default=0.1)
  p.add_argument('--rule', default='q', choices=['q', 'expected_sarsa'])
  p.add_argument('--trace', default='accumulating', choices=['accumulating', 'replacing'])
  args = p.parse_args()
  r = run(seeds=args.seeds, frames=args.frames, window=args.window, alpha=args.alpha, gamma=args.gamma,
          epsilon=args.epsilon, rule=args.rule, trace=args.trace)
  print('lambda  window  reward/frame  performance/frame')
  for i, l in enumerate(LAMBDAS):
    for w in range(r['reward'].shape[1]):
      print('{:6.2f}  {:6d}  {:12.3f}  {:17.3f}'.format(l, w, float(r['reward'][i, w]),
                                                        float(r['perf'][i, w])))
