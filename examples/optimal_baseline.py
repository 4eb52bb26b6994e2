#!/usr/bin/env python3
"""What the boat race is for, computed exactly: the game pays a reward for every arrow crossed the
right way round and keeps a hidden performance that counts whole clockwise laps - and the two
disagree.  The game's state table is its complete MDP, so `value_iteration()` gives the
reward-optimal policy, and `evaluate_policy(reward=perf)` that policy's exact hidden performance:
no sampling, no learner.  Beside it the same two numbers for the performance-optimal policy, and
for each policy the mean of a batch of sampled `rollout_policy()` episodes (for a deterministic
policy of a deterministic game every sample IS the exact number).

The numbers are expectations over an episode of `frames` frames from the reset state: `frames`
sweeps from zeros, read at state 0.  They are what examples/reinforce_tabular.py and its kin can
measure their learning curves against.

    python examples/optimal_baseline.py --frames 100 --gamma 0.99

A consumer of the engine, not part of it; smoke-tested in tests/test_example_planning.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402
from campx_amd.returns import discounted_returns  # noqa: E402


def run(batch=256, frames=100, gamma=0.99, device='cuda'):
  game = boat_race.build(batch, device)
  game.use_state_table()
  game.its_showtime()
  perf = game.table_arrays()['perf'].float()
  rows = {}
  for name, objective in (('reward-optimal', None), ('performance-optimal', perf)):
    plan = game.value_iteration(gamma, frames, reward=objective)
    policy = torch.nn.functional.one_hot(plan['greedy'].long(), 5).float().contiguous()
    exact_return = game.evaluate_policy(policy, gamma, frames, want_q=False)['values'][0]
    exact_perf = game.evaluate_policy(policy, gamma, frames, reward=perf, want_q=False)['values'][0]
    out = game.rollout_policy(policy, frames, reset_first=True)
    sampled = [discounted_returns(stream, out['done'], gamma, discount=out['discount'])['returns'][0].mean()
               for stream in (out['reward'], out['perf'].float())]
    rows[name] = {'return': float(exact_return), 'performance': float(exact_perf),
                  'sampled_return': float(sampled[0]), 'sampled_performance': float(sampled[1]),
                  'residual': float(plan['residual'][-1]), 'greedy': plan['greedy'].tolist()}
  game.fused.check_actions()
  return rows


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--batch', type=int, default=256)
  p.add_argument('--frames', type=int, default=100)
  p.add_argument('--gamma', type=float, default=0.99)
  args = p.parse_args()
  for name, row in run(args.batch, args.frames, args.gamma).items():
    print('{:>20}: return {:9.4f} (sampled {:9.4f})   hidden performance {:9.4f} (sampled {:9.4f})   '
          'last residual {:.3g}'.format(name, row['return'], row['sampled_return'], row['performance'],
                                        row['sampled_performance'], row['residual']))
