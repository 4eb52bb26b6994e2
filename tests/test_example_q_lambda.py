"""examples/q_lambda_sweep.py at a small B and T: three lambdas x 8 seeds = 24 learners, 130 frames
in windows of 50 (the last one short).  The learners' tables and traces bit for bit against
tests/trace_learner_reference.py under the same arguments, and the curves - [lambdas, windows],
per frame - against the reference's window sums."""

import os
import sys

import numpy as np
import pytest

import trace_learner_reference as trace_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS, SEEDS, FRAMES, WINDOW = (0.0, 0.5, 0.9), 8, 130, 50


@pytest.mark.gpu
@pytest.mark.parametrize('rule,kind', [('q', 'accumulating'), ('expected_sarsa', 'replacing')])
def test_the_sweep_learns_what_the_reference_learns_and_its_curves_have_the_documented_shapes(rule, kind):
  from campx_amd import tabulate
  from campx_amd.games import boat_race
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import q_lambda_sweep
  got = q_lambda_sweep.run(LAMBDAS, SEEDS, FRAMES, WINDOW, rule=rule, trace=kind, seed=3)
  B, W = len(LAMBDAS) * SEEDS, 3
  lam = np.repeat(np.array(LAMBDAS, np.float32), SEEDS)
  assert np.array_equal(got['lam'].cpu().numpy(), lam)
  L = trace_ref.TraceLearners(tabulate.trace(boat_race.build()), B)
  want = L.learn_traces(FRAMES, lam, kind, 0.1, 0.9, 0.1, rule, seed=3, reset_first=True, window=WINDOW)
  q, z = got['q'].cpu().numpy(), got['traces'].cpu().numpy()
  assert q.shape == z.shape == (B, 8, 5)
  assert np.array_equal(q.view(np.uint32), L.q.view(np.uint32))
  assert np.array_equal(z.view(np.uint32), L.z.view(np.uint32))
  length = np.array([50, 50, 30], np.float64)
  for k, sums in (('reward', want['reward_sum']), ('perf', want['perf_sum'])):
    assert tuple(got[k].shape) == (len(LAMBDAS), W), k
    curve = sums.reshape(W, len(LAMBDAS), SEEDS).astype(np.float64).mean(2) / length[:, None]
    assert np.allclose(got[k].cpu().numpy(), curve.T, rtol=0, atol=1e-5), k
  assert tuple(got['episodes'].shape) == (len(LAMBDAS), W)
  # the learners of one lambda differ by seed alone, and lambda matters
  assert not np.array_equal(L.q[0], L.q[1]) and not np.array_equal(L.q[:SEEDS], L.q[SEEDS:2 * SEEDS])
