"""examples/actor_critic_sweep.py at a small batch: three actor step sizes x 4 seeds = 12 learners,
130 frames in windows of 50 (the last one short).  The learners' tables bit for bit against
tests/actor_critic_reference.py under the same arguments, the curves - [settings, windows] - against
the reference's window sums, the exact fitness against `evaluate_population()` called directly, and
one printed line per setting."""

import os
import sys

import numpy as np
import pytest

import actor_critic_reference as ac_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHAS, SEEDS, FRAMES, WINDOW = (0.0, 0.1, 0.8), 4, 130, 50


@pytest.mark.gpu
def test_the_sweep_learns_what_the_reference_learns_and_prints_a_line_per_setting():
  import torch
  from campx_amd import returns, tabulate
  from campx_amd.games import boat_race
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import actor_critic_sweep
  got = actor_critic_sweep.run(ALPHAS, SEEDS, FRAMES, WINDOW, seed=3, evaluate=2, sweeps=50)
  B, W = len(ALPHAS) * SEEDS, 3
  alpha_actor = np.repeat(np.array(ALPHAS, np.float32), SEEDS)
  assert np.array_equal(got['alpha_actor'].cpu().numpy(), alpha_actor)
  L = ac_ref.ActorCritics(tabulate.trace(boat_race.build()), B)
  want = L.learn(FRAMES, alpha_actor, 0.1, 0.9, seed=3, reset_first=True, window=WINDOW)
  prefs, values = got['prefs'].cpu().numpy(), got['values'].cpu().numpy()
  assert prefs.shape == (B, 8, 5) and np.array_equal(prefs.view(np.uint32), L.prefs.view(np.uint32))
  assert np.array_equal(values.view(np.uint32), L.values.view(np.uint32))
  assert not prefs[:SEEDS].any() and prefs[SEEDS:].any()          # alpha_actor = 0 keeps the uniform policy
  frames = np.array([50, 50, 30], np.float64)
  for k, sums in (('reward', want['reward_sum']), ('perf', want['perf_sum'])):
    assert tuple(got[k].shape) == (len(ALPHAS), W), k
    curve = sums.reshape(W, len(ALPHAS), SEEDS).astype(np.float64).mean(2) / frames[:, None]
    assert np.allclose(got[k].cpu().numpy(), curve.T, rtol=0, atol=1e-4), k
  # exact fitness: the first two learners of every setting, evaluated directly
  picked = got['prefs'].view(len(ALPHAS), SEEDS, 8, 5)[:, :2].reshape(6, 8, 5).contiguous()
  game = boat_race.build(1, 'cuda')
  game.use_state_table()
  game.its_showtime()
  direct = game.evaluate_population(returns.softmax_weights(picked), 0.9, 50)['values'][:, 0]
  assert tuple(got['fitness'].shape) == (3, 2) and tuple(got['hidden'].shape) == (3, 2)
  assert torch.equal(got['fitness'].reshape(-1), direct)
  # the uniform policy's exact value does not depend on the seed
  assert float(got['fitness'][0, 0]) == float(got['fitness'][0, 1]) < 0
  printed = actor_critic_sweep.lines(ALPHAS, {k: v.cpu() for k, v in got.items()})
  assert len(printed) == 3
  for a, line in zip(ALPHAS, printed):
    assert line.startswith('alpha_actor {:5.2f}  reward/frame '.format(a)) and 'exact hidden value' in line
