#!/usr/bin/env python3
"""Reward design on the boat race, exactly and in two launches.  The game pays a reward r for
crossing checkpoints and hides a performance that counts whole clockwise laps; the policy that r
points to shuttles across one checkpoint and never laps.  Which reward would have pointed to the
policy the designer wanted?  Take K candidates `rewards[k] = r + lambda_k * perf` (None counts
as 0) and

    value_iteration_population(rewards=...)        K + 1 greedy policies in ONE launch - the last
                                                   member's reward is perf alone: the best that the
                                                   hidden measure allows
    evaluate_population(one_hot(greedy),           every one of those policies' exact hidden
                        rewards=perf tiled)        performance, in ONE more

and print the smallest lambda whose reward-optimal policy is also performance-optimal: its hidden
performance from the reset state equals the last member's.  Nothing is sampled; a loop of
`value_iteration(reward=rewards[k])` and `evaluate_policy(..., reward=perf)` calls gives the same
bits at 2 K + 2 launches.

    python examples/reward_design_sweep.py --candidates 33 --largest 4

A consumer of the engine, not part of it; smoke-tested in tests/test_example_reward_design.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402


def run(candidates=33, largest=4.0, sweeps=100, gamma=0.99, device='cuda'):
  """-> dict: 'lambdas' float32 [K]; 'rewards' [K + 1, S, 5] (the last row perf alone); 'greedy'
  int8 [K + 1, S]; 'value' [K + 1], each member's optimal value of ITS reward at the reset state;
  'performance' [K + 1], its greedy policy's exact hidden performance there; 'smallest', the
  smallest lambda whose policy reaches the last member's performance (None if none does)."""
  K = int(candidates)
  game = boat_race.build(1, device)
  game.use_state_table()
  game.its_showtime()
  table = game.table_arrays()
  r, perf = torch.nan_to_num(table['reward'], nan=0.0), table['perf'].float()
  lambdas = torch.linspace(0.0, float(largest), K, device=device)
  rewards = torch.cat([r[None] + lambdas[:, None, None] * perf[None], perf[None]]).contiguous()
  solved = game.value_iteration_population(gamma, sweeps, rewards=rewards)
  policies = torch.nn.functional.one_hot(solved['greedy'].long(), 5).float().contiguous()
  hidden = game.evaluate_population(policies, gamma, sweeps,
                                    rewards=perf.expand(K + 1, -1, -1).contiguous())
  performance = hidden['values'][:, 0]
  reached = (performance[:K] >= performance[K]).nonzero()
  game.fused.check_actions()
  return {'lambdas': lambdas, 'rewards': rewards, 'greedy': solved['greedy'],
          'value': solved['values'][:, 0].clone(), 'performance': performance.clone(),
          'smallest': float(lambdas[int(reached[0])]) if len(reached) else None}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--candidates', type=int, default=33)
  p.add_argument('--largest', type=float, default=4.0)
  p.add_argument('--sweeps', type=int, default=100)
  p.add_argument('--gamma', type=float, default=0.99)
  args = p.parse_args()
  res = run(args.candidates, args.largest, args.sweeps, args.gamma)
  K = args.candidates
  for k in range(K):
    print('lambda {:6.3f}: optimal value of its reward {:9.4f}   hidden performance of its policy '
          '{:9.4f}'.format(float(res['lambdas'][k]), float(res['value'][k]), float(res['performance'][k])))
  print('the best hidden performance any policy reaches: {:9.4f}'.format(float(res['performance'][K])))
  if res['smallest'] is None:
    print('no lambda up to {} makes the reward-optimal policy performance-optimal'.format(args.largest))
  else:
    print('smallest lambda whose reward-optimal policy is also performance-optimal: {:.3f}'.format(
        res['smallest']))
