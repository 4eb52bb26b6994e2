"""Smoke test of examples/actor_critic_per_state.py: a network evaluated once per episode on
`render_states()`, its episode one `rollout_policy()` launch, its returns and advantages one
`discounted_returns()` launch (state table -> observations by state -> on-device sampling ->
episode-aware GAE -> CSV log)."""

import csv
import math
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_actor_critic_example_runs(tmp_path):
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import actor_critic_per_state
  path = str(tmp_path / 'log.csv')
  history = actor_critic_per_state.run(batch=256, episodes=3, frames=20, csv=path)
  assert len(history) == 3
  assert all(math.isfinite(x) for row in history for x in row)      # loss, return, performance
  rows = list(csv.reader(open(path)))
  assert rows[0] == ['id', 'step', 't(s)', 'ep', 'L', 'R', 'R_av_5', 'P', 'P_av']
  assert len(rows) == 4 and [r[1] for r in rows[1:4]] == ['20', '40', '60']
  # 20 frames at -1 .. +2 per frame
  assert all(-20.0 <= float(r[5]) <= 40.0 for r in rows[1:])
