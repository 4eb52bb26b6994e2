"""Smoke test of examples/exact_policy_gradient.py: a softmax policy on the boat race climbs to
`value_iteration()`'s optimum by the exact gradient (`state_visitation()` for d_gamma,
`evaluate_policy()` for q).

The iteration count and the margin come from the same loop run on the CPU with the two numpy
references (tests/visitation_reference.py, tests/planning_reference.py), lr 4, 64 frames, gamma
0.9: after 30 iterations v[0] = 5.77050 against the optimum 5.78265, a gap of 0.01215.  The margin
is twice that gap."""

import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ITERATIONS = 30
MARGIN = 2 * 0.01215


@pytest.mark.gpu
def test_exact_policy_gradient_example_climbs_to_the_optimum():
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import exact_policy_gradient
  lines = []
  res = exact_policy_gradient.run(iterations=ITERATIONS, frames=64, gamma=0.9, lr=4.0, log=lines.append)
  values, optimum = res['values'], res['optimum']
  print('first v[0] %.5f last v[0] %.5f optimum %.5f gap %.5f' % (values[0], values[-1], optimum,
                                                                  optimum - values[-1]))
  assert len(values) == ITERATIONS + 1 == len(lines) and 'optimum' in lines[0]
  assert values[0] < 0 < values[-1]                       # the uniform policy loses reward
  assert values[-1] <= optimum + 1e-4                     # no policy beats the optimum
  assert optimum - values[-1] <= MARGIN
  assert tuple(res['policy'].shape) == (8, 5)
