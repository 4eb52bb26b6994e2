"""Smoke test of examples/exact_gradient_population.py: three softmax learners on the boat race,
each with its own learning rate, climb the exact policy gradient - one `evaluate_population()` and
one `visit_population()` per step for all of them.

Gradient ascent with a small enough step does not lose ground: the member with the smallest
learning rate (0.25, a sixteenth of the rate examples/exact_policy_gradient.py runs at) must never
see its exact return fall from one step to the next.  The members start equal and must not stay
so."""

import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = 6


@pytest.mark.gpu
def test_exact_gradient_population_example_climbs_for_every_learning_rate():
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import exact_gradient_population
  lines = []
  res = exact_gradient_population.run(members=3, steps=STEPS, frames=64, gamma=0.9, lr_min=0.25, lr_max=4.0,
                                      log=lines.append)
  values, lr = res['values'], res['lr']
  for line in lines:
    print(line)
  assert len(values) == STEPS + 1 == len(lines) and all(len(row) == 3 for row in values)
  assert lr[0] == min(lr) == 0.25 and abs(lr[1] - 1.0) < 1e-12 and abs(lr[2] - 4.0) < 1e-12
  assert values[0][0] == values[0][1] == values[0][2] < 0          # the uniform policy, three times
  slowest = [row[0] for row in values]
  assert all(b >= a for a, b in zip(slowest, slowest[1:])), slowest
  assert slowest[-1] > slowest[0]
  assert len(set(values[-1])) == 3                                  # the members are not all equal
  assert tuple(res['policies'].shape) == (3, 8, 5)
