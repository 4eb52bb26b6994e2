"""Smoke test of examples/reinforce_population.py: four REINFORCE learners with different learning
rates in one process - rollout_population() -> discounted_returns() -> sum_by_state(P * S) -> one
step on logits[P, S, 5] - whose runs repeat bit for bit."""

import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_population_reinforce_example_runs_learns_and_repeats():
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import reinforce_population
  lrs = (0.0, 0.1, 0.3, 1.0)
  history = reinforce_population.run(batch=1024, lrs=lrs, episodes=12, frames=20)
  assert len(history) == 12 and all(len(row) == 4 for row in history)
  # 20 frames at -1 .. +2 per frame
  assert all(-20.0 <= r <= 40.0 for row in history for r in row)
  # the learners are apart: a learning rate of 0 stays the uniform policy it started as, the others
  # learn - returns go up, and beyond the one that does not learn
  assert all(history[-1][m] > history[0][m] for m in (1, 2, 3))
  assert all(history[-1][m] > history[-1][0] for m in (1, 2, 3))
  # fixed-point sums: the same seeds give the same numbers on every run
  assert reinforce_population.run(batch=1024, lrs=lrs, episodes=12, frames=20) == history
