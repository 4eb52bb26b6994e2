"""Smoke test of examples/impala_tabular.py: one tabular learner fed by four stale snapshots of its
own policy - rollout_population() -> table_lookup() -> vtrace_returns() in table mode ->
sum_by_state(P * S) -> a step - run small, in-process, through its `main`."""

import math
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_impala_example_runs_and_prints_finite_exact_returns(capsys):
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import impala_tabular
  history = impala_tabular.main(['--batch', '1024', '--members', '4', '--iterations', '6', '--frames', '20',
                                 '--sweeps', '64'])
  printed = re.findall(r'^it: (\d+), exact return of the learner: (\S+)$', capsys.readouterr().out, flags=re.M)
  assert [int(i) for i, _ in printed] == list(range(6))
  values = [float(v) for _, v in printed]
  assert len(history) == 6 and all(math.isfinite(v) for v in values + history)
  assert all(abs(a - b) < 1e-3 for a, b in zip(values, history))
  # the uniform policy it starts as has one exact value, and the updates move the learner off it
  assert len(set(history)) > 1
