"""Smoke test of examples/reinforce_by_state.py: tabular REINFORCE whose learner is arithmetic on
`[n_states, 5]` (rollout_policy() -> discounted_returns() -> sum_by_state() -> CSV log), and whose
runs repeat bit for bit."""

import csv
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_by_state_reinforce_example_runs_learns_and_repeats(tmp_path):
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import reinforce_by_state
  path = str(tmp_path / 'log.csv')
  history = reinforce_by_state.run(batch=512, episodes=12, frames=20, csv=path)
  assert len(history) == 12
  rows = list(csv.reader(open(path)))
  assert rows[0] == ['id', 'step', 't(s)', 'ep', 'L', 'R', 'R_av_5', 'P', 'P_av']
  assert len(rows) == 13 and [r[1] for r in rows[1:4]] == ['20', '40', '60']
  # 20 frames at -1 .. +2 per frame; and the table learns: returns go up
  assert all(-20.0 <= float(r[5]) <= 40.0 for r in rows[1:])
  assert history[-1][1] > history[0][1]
  # fixed-point sums: the same seed gives the same numbers on every run
  assert reinforce_by_state.run(batch=512, episodes=12, frames=20) == history
