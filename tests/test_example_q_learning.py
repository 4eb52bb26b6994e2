"""examples/q_learning_sweep.py on a small grid: the learners' tables bit for bit against the numpy
learners of tests/learner_reference.py under the same schedule, and their greedy actions against
`value_iteration()`'s in every state where q* decides.

The configuration: epsilon 0.6 and 1.0 x alpha 0.2 and 0.5 x 4 seeds = 16 learners, gamma 0.5,
3 calls of T = 500 frames, epsilon times 0.8 from call to call, seed 0, both rules.  q* of the boat
race at gamma 0.5 decides states 0, 3, 4 and 7 (best minus second-best = 2.0 there; in the other
four every action costs the same -1 and several tie exactly) - the only states left out.  The
numpy reference ALONE, run on the CPU, meets the greedy-action check for all 16 learners of both
rules; its smallest gap between a learner's best and second-best action in a decided state is 1.91
(Q-learning) and 1.84 (expected SARSA), against differences of 2.0 in q*.  (At gamma 0.9 and these
1 500 frames Q-learning does not get there: 13 to 16 of 16 learners, gaps down to 0.03.)"""

import os
import sys

import numpy as np
import pytest

import learner_reference as learn_ref
import planning_reference as plan_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPSILONS, ALPHAS, SEEDS, CALLS, FRAMES, GAMMA, DECAY = (0.6, 1.0), (0.2, 0.5), 4, 3, 500, 0.5, 0.8
DECIDED = [True, False, False, True, True, False, False, True]

_REFERENCE = {}


def _reference(rule):
  """The schedule of examples/q_learning_sweep.py, restated: computed once per rule."""
  if rule not in _REFERENCE:
    from campx_amd import tabulate
    from campx_amd.games import boat_race
    g = tabulate.trace(boat_race.build())
    eps = [e for e in EPSILONS for _ in ALPHAS for _ in range(SEEDS)]
    alpha = np.array([a for _ in EPSILONS for a in ALPHAS for _ in range(SEEDS)], np.float32)
    L = learn_ref.Learners(g, len(eps))
    for call in range(CALLS):
      now = np.array([e * DECAY ** call for e in eps], np.float32)
      last = L.learn(FRAMES, alpha, np.float32(GAMMA), now, rule=rule, seed=0, reset_first=call == 0)
    best = plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, GAMMA, 400)
    _REFERENCE[rule] = L, last, best
  return _REFERENCE[rule]


@pytest.mark.parametrize('rule', learn_ref.RULES)
def test_the_numpy_learners_alone_reach_the_reward_optimal_greedy_actions(rule):
  L, _, best = _reference(rule)
  assert best['residual'][-1] == 0.0                     # q* has converged to the last bit
  top = np.sort(best['q'], axis=1)
  decided = top[:, -1] != top[:, -2]
  assert decided.tolist() == DECIDED and (top[decided, -1] - top[decided, -2] == 2.0).all()
  greedy = plan_ref.reduce_greedy(L.q.reshape(-1, 5))[1].reshape(16, 8)
  assert (greedy[:, decided] == best['greedy'][decided]).all()
  gaps = np.sort(L.q, axis=2)[:, decided]
  assert (gaps[:, :, -1] - gaps[:, :, -2]).min() > 1.8


@pytest.mark.gpu
@pytest.mark.parametrize('rule', learn_ref.RULES)
def test_the_sweep_learns_what_the_reference_learns_and_ends_reward_optimal(rule):
  import torch
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import q_learning_sweep
  got = q_learning_sweep.run(EPSILONS, ALPHAS, SEEDS, CALLS, FRAMES, GAMMA, DECAY, rule=rule, seed=0)
  L, last, best = _reference(rule)
  q = got['q'].cpu().numpy()
  assert q.shape == (16, 8, 5) and np.array_equal(q.view(np.uint32), L.q.view(np.uint32))
  # q* and what it decides are the planner's
  assert got['decided'].tolist() == DECIDED
  assert np.array_equal(got['optimal'].cpu().numpy(), best['greedy'].astype(np.int64))
  # every learner's greedy action is the reward-optimal one wherever q* decides
  greedy = got['q'].argmax(2)
  decided = got['decided']
  assert bool((greedy[:, decided] == got['optimal'][decided]).all())
  assert bool(got['agrees'].all()) and torch.equal(got['share'], torch.ones((2, 2), device='cuda'))
  # the curves of the last call: one window of FRAMES frames, means over a cell's four seeds
  want = last['reward_sum'][0].reshape(2, 2, SEEDS).astype(np.float64).mean(2) / FRAMES
  assert np.allclose(got['reward'].cpu().numpy(), want, rtol=0, atol=1e-6)
  want = last['perf_sum'][0].reshape(2, 2, SEEDS).astype(np.float64).mean(2) / FRAMES
  assert np.allclose(got['perf'].cpu().numpy(), want, rtol=0, atol=1e-6)
