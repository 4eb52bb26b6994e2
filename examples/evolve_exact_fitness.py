#!/usr/bin/env python3
"""An evolution strategy on the boat race whose fitness is EXACT: each generation perturbs a table
of logits P times, and `evaluate_population()` gives every candidate's exact expected return from
the reset state - `frames` sweeps from zeros, read at state 0 - in one launch.  Nothing is sampled
anywhere: no rollout, no noise in the selection, and a run repeats bit for bit.

The strategy is the plainest there is - keep the best `elite` candidates, move the mean to their
average, shrink nothing - because the point is the inner loop: P exact evaluations per generation
cost one launch, not P.  The winner's hidden performance (the boat race counts whole clockwise
laps, which its reward does not pay for) is reported the same way, through
`reward=table_arrays()['perf'].float()`.

    python examples/evolve_exact_fitness.py --population 256 --generations 30

A consumer of the engine, not part of it; smoke-tested in tests/test_example_population_planning.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402


def run(population=256, generations=30, frames=50, gamma=0.99, sigma=0.5, elite=None, seed=0,
        device='cuda', keep_fitness=False):
  """-> a list of one dict per generation: 'best' and 'mean' fitness, the best candidate's exact
  'performance' and - `keep_fitness` - 'fitness', the float32 [P] vector itself, and 'policies',
  the [P, n_states, 5] weights it was computed from."""
  P = int(population)
  elite = max(1, P // 4) if elite is None else int(elite)
  game = boat_race.build(1, device)
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  perf = game.table_arrays()['perf'].float()
  rng = torch.Generator(device='cpu').manual_seed(seed)
  mean = torch.zeros((S, 5), device=device)                  # logits: the uniform policy
  out = game.population_sweep_buffers(P, frames)
  one = game.population_sweep_buffers(1, frames)
  history = []
  for _ in range(generations):
    noise = torch.randn((P, S, 5), generator=rng).to(device)
    noise[0] = 0                                             # (the mean itself is a candidate)
    logits = mean + sigma * noise
    policies = torch.softmax(logits, dim=2).contiguous()
    fitness = game.evaluate_population(policies, gamma, frames, out=out)['values'][:, 0]
    order = torch.argsort(fitness, descending=True, stable=True)
    best = int(order[0])
    hidden = game.evaluate_population(policies[best:best + 1], gamma, frames, reward=perf, out=one)
    row = {'best': float(fitness[best]), 'mean': float(fitness.mean()),
           'performance': float(hidden['values'][0, 0])}
    if keep_fitness:
      row['fitness'], row['policies'] = fitness.clone(), policies
    history.append(row)
    mean = logits[order[:elite]].mean(0)
  game.fused.check_actions()
  return history


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--population', type=int, default=256)
  p.add_argument('--generations', type=int, default=30)
  p.add_argument('--frames', type=int, default=50)
  p.add_argument('--gamma', type=float, default=0.99)
  p.add_argument('--sigma', type=float, default=0.5)
  args = p.parse_args()
  rows = run(args.population, args.generations, args.frames, args.gamma, args.sigma)
  for g, row in enumerate(rows):
    print('generation {:3d}: best exact return {:9.4f}   mean {:9.4f}   the best one\'s hidden '
          'performance {:9.4f}'.format(g, row['best'], row['mean'], row['performance']))
