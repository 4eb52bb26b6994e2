"""Smoke test of examples/evolve_exact_fitness.py: three generations of an evolution strategy on
the boat race at P = 16 whose fitness is `evaluate_population(...)['values'][:, 0]` - which has to
be, bit for bit, what a loop of `evaluate_policy()` over the candidates gives."""

import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_the_fitness_vector_is_a_loop_of_evaluate_policy_bit_for_bit():
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import evolve_exact_fitness
  from campx_amd.games import boat_race
  frames, gamma = 20, 0.99
  rows = evolve_exact_fitness.run(population=16, generations=3, frames=frames, gamma=gamma,
                                  keep_fitness=True)
  assert len(rows) == 3
  game = boat_race.build(1, 'cuda')
  game.use_state_table()
  game.its_showtime()
  perf = game.table_arrays()['perf'].float()
  for row in rows:
    fitness, policies = row['fitness'], row['policies']
    assert tuple(fitness.shape) == (16,) and tuple(policies.shape) == (16, 8, 5)
    loop = [game.evaluate_policy(policies[m], gamma, frames, want_q=False)['values'][0].item()
            for m in range(16)]
    got = fitness.cpu().numpy()
    assert np.array_equal(got.view(np.int32), np.array(loop, np.float32).view(np.int32))
    best = int(got.argmax())
    assert row['best'] == float(got[best]) and row['best'] >= row['mean']
    hidden = game.evaluate_policy(policies[best], gamma, frames, reward=perf, want_q=False)['values'][0]
    assert row['performance'] == float(hidden)
    assert all(math.isfinite(row[k]) for k in ('best', 'mean', 'performance'))
    assert -20.0 <= row['best'] <= 40.0          # 20 frames at -1 .. +2 per frame
  again = evolve_exact_fitness.run(population=16, generations=3, frames=frames, gamma=gamma)
  assert [r['best'] for r in again] == [r['best'] for r in rows]
