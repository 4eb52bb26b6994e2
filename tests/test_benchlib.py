"""tools/benchlib.py's timers on the device: they make the calls they say, every call runs there,
and what they return is a time."""
import math
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
if TOOLS not in sys.path:
  sys.path.insert(0, TOOLS)
import benchlib  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_timers_make_warm_plus_runs_calls_on_the_device():
  import torch
  x = torch.zeros((1,), device='cuda')
  calls = {'median': 0, 'a': 0, 'b': 0}

  def counted(name):
    def fn():
      calls[name] += 1
      x.add_(1)
    return fn

  ms = benchlib.median_ms(counted('median'), 7, warm=3)
  assert calls['median'] == 3 + 7 and math.isfinite(ms) and ms > 0
  spread = benchlib.alternating_ms({'a': counted('a'), 'b': counted('b')}, 5, 2)
  assert calls['a'] == calls['b'] == 2 + 5 and list(spread) == ['a', 'b']
  for median, low, high in spread.values():
    assert all(math.isfinite(v) and v > 0 for v in (median, low, high)) and low <= median <= high
  assert float(x) == sum(calls.values()) == 24                # every call ran on the device
