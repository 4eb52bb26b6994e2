"""examples/a2c_parallel_actors.py at a small size: 3 learners of 16 actors, 240 frames in windows
of 80.  The learners' tables bit for bit against the numpy learners of
tests/shared_actor_reference.py, the printed curves against its window sums, the exact returns
against the planner's own `evaluate_policy()` one policy at a time - and every learner's return
above the uniform policy's."""

import os
import sys

import numpy as np
import pytest

import shared_actor_reference as sa_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARNERS, ACTORS, FRAMES, WINDOW = 3, 16, 240, 80
KW = dict(alpha_critic=0.2, gamma=0.9, seed=5)


@pytest.mark.gpu
def test_the_learners_learn_what_the_reference_learns_and_beat_the_uniform_policy():
  import torch
  from campx_amd import returns, tabulate
  from campx_amd.games import boat_race
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import a2c_parallel_actors as example
  steps = example.step_sizes(LEARNERS)
  assert np.allclose(steps, [0.01, 0.01 * 50 ** 0.5, 0.5])
  r = example.run(learners=LEARNERS, actors=ACTORS, frames=FRAMES, window=WINDOW, **KW)
  g = tabulate.trace(boat_race.build())
  S = g.n_states
  alpha_actor = r['alpha_actor'].cpu().numpy()
  assert alpha_actor.dtype == np.float32 and np.allclose(alpha_actor, steps)
  L = sa_ref.SharedActorCritics(g, LEARNERS * ACTORS, np.zeros((LEARNERS, S, 5), np.float32),
                                np.zeros((LEARNERS, S), np.float32))
  want = L.learn(FRAMES, alpha_actor, reset_first=True, window=WINDOW, **KW)
  prefs, values = r['prefs'].cpu().numpy(), r['values'].cpu().numpy()
  assert np.array_equal(prefs.view(np.uint32), L.prefs.view(np.uint32)) and np.abs(prefs).max() > 0
  assert np.array_equal(values.view(np.uint32), L.values.view(np.uint32))
  assert r['clamped'].tolist() == [0] * LEARNERS
  W = FRAMES // WINDOW
  curve = want['reward_sum'].reshape(W, LEARNERS, ACTORS).astype(np.float64).mean(2) / WINDOW
  assert np.allclose(r['curve'].cpu().numpy(), curve, rtol=0, atol=1e-5)
  curve = want['perf_sum'].reshape(W, LEARNERS, ACTORS).astype(np.float64).mean(2) / WINDOW
  assert np.allclose(r['perf'].cpu().numpy(), curve, rtol=0, atol=1e-5)
  planner = boat_race.build(1, 'cuda')
  planner.use_state_table()
  planner.its_showtime()
  weights = returns.softmax_weights(r['prefs'])
  for m in range(LEARNERS):
    alone = planner.evaluate_policy(weights[m], KW['gamma'], 400)['values']
    assert torch.equal(alone[0].view(torch.int32), r['return'][m].view(torch.int32)), m
  uniform = planner.evaluate_policy(torch.ones((S, 5), device='cuda'), KW['gamma'], 400)['values'][0]
  assert torch.equal(uniform.view(torch.int32), r['uniform_return'].view(torch.int32))
  # every step size of the sweep learnt something: the exact return rose above the uniform policy's
  assert float(uniform) < -5 and (r['return'] > uniform + 1).all(), (r['return'], uniform)
  # ... and the curves rose with it
  assert (r['curve'][-1] > r['curve'][0]).all()
