"""Smoke test of examples/reward_design_sweep.py: K = 9 rewards `r + lambda * perf` on the boat
race, whose K + 1 greedy policies come from one `value_iteration_population()` and whose hidden
performances from one `evaluate_population(rewards=...)` - which have to be, bit for bit, what the
loop of `value_iteration(reward=...)` and `evaluate_policy(..., reward=perf)` calls gives."""

import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
  x = t.detach().cpu().numpy()
  return x.view(np.int32) if x.dtype == np.float32 else x


@pytest.mark.gpu
def test_the_sweep_is_the_loop_of_single_calls_bit_for_bit():
  import torch
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import reward_design_sweep
  from campx_amd.games import boat_race
  K, sweeps, gamma = 9, 40, 0.99
  res = reward_design_sweep.run(candidates=K, largest=4.0, sweeps=sweeps, gamma=gamma)
  game = boat_race.build(1, 'cuda')
  game.use_state_table()
  game.its_showtime()
  perf = game.table_arrays()['perf'].float()
  assert tuple(res['rewards'].shape) == (K + 1, 8, 5) and tuple(res['greedy'].shape) == (K + 1, 8)
  assert torch.equal(res['rewards'][K], perf) and float(res['lambdas'][0]) == 0.0
  for k in range(K + 1):
    alone = game.value_iteration(gamma, sweeps, reward=res['rewards'][k], want_q=False)
    assert np.array_equal(_bits(res['greedy'][k]), _bits(alone['greedy'])), k
    assert np.array_equal(_bits(res['value'][k]), _bits(alone['values'][0])), k
    policy = torch.nn.functional.one_hot(alone['greedy'].long(), 5).float()
    hidden = game.evaluate_policy(policy, gamma, sweeps, reward=perf, want_q=False)['values'][0]
    assert np.array_equal(_bits(res['performance'][k]), _bits(hidden)), k
  performance = res['performance'].cpu().numpy()
  best = performance[K]
  assert (performance[:K] <= best).all()         # perf's own optimal policy is the best by perf
  assert performance[0] < best                   # the game's reward alone misses it: the point of the game
  reached = [k for k in range(K) if performance[k] >= best]
  assert reached and res['smallest'] == float(res['lambdas'][reached[0]]) and res['smallest'] > 0
