"""Smoke test of examples/optimal_baseline.py: the boat race's reward-optimal and
performance-optimal policies from its state table, each with its exact return and exact hidden
performance (value_iteration() -> evaluate_policy(reward=perf)), beside a sampled batch."""

import math
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_optimal_baseline_example_runs_and_orders_the_two_policies():
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import optimal_baseline
  rows = optimal_baseline.run(batch=64, frames=20, gamma=0.99)
  assert sorted(rows) == ['performance-optimal', 'reward-optimal']
  by_reward, by_perf = rows['reward-optimal'], rows['performance-optimal']
  for row in rows.values():
    assert all(math.isfinite(row[k]) for k in ('return', 'performance', 'sampled_return',
                                               'sampled_performance', 'residual'))
    assert len(row['greedy']) == 8 and all(0 <= a <= 4 for a in row['greedy'])
    # 20 frames at -1 .. +2 per frame
    assert -20.0 <= row['return'] <= 40.0
  # each policy is the best at what it was planned for - and the two objectives disagree
  assert by_reward['return'] >= by_perf['return']
  assert by_perf['performance'] >= by_reward['performance']
  assert by_reward['return'] > 0
  assert optimal_baseline.run(batch=64, frames=20, gamma=0.99) == rows
