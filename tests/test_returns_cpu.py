"""`campx_returns_launch()` without a GPU: the validator refuses every bad argument before anything
is launched.  (tests/test_returns.py holds the kernel to tests/returns_reference.py on the GPU;
test_vtrace_cpu.py and test_state_sums_cpu.py do for their launchers what this does for this one.)"""

import ctypes

import pytest

from campx_amd import _hip

B, T = 65, 9
_NAN, _INF = float('nan'), float('inf')
_FLOATS = dict(reward=0x1000, discount=0x3000, values=0x4000, bootstrap=0x5000, returns=0x6000,
               advantages=0x7000)
_PITCHES = ('reward', 'done', 'discount', 'values', 'returns', 'advantages')


def _args(**change):
  """A CampxReturns whose pointers are fake but aligned, non-NULL addresses: every call below is
  refused by the validator, so none is ever dereferenced."""
  r = _hip.CampxReturns()
  r.done = 0x2001
  for k, address in _FLOATS.items():
    setattr(r, k, address)
  for k in _PITCHES:
    setattr(r, k + '_pitch', B)
  r.gamma, r.lam = 0.99, 0.95
  for k, x in change.items():
    if k not in ('B', 'T'):
      setattr(r, k, x)
  return _hip.lib.campx_returns_launch(ctypes.byref(r), change.get('B', B), change.get('T', T), None)


def _cases():
  cases = [dict(reward=None), dict(done=None), dict(returns=None)]
  cases += [dict(values=None), dict(advantages=None)]           # one of the pair without the other
  cases += [{k: address + off} for k, address in _FLOATS.items() for off in (1, 2)]
  cases += [{k + '_pitch': p} for k in _PITCHES for p in (64, -1, (1 << 40) // T + 1)]
  cases += [dict(B=0), dict(B=-1), dict(B=(1 << 31) + 1), dict(T=0), dict(T=-1)]
  cases += [{k: x} for k in ('gamma', 'lam') for x in (_NAN, _INF, -_INF)]
  return cases


@pytest.mark.parametrize('change', _cases(), ids=lambda c: ','.join('{}={}'.format(*kv) for kv in c.items()))
def test_the_launch_validator_refuses_a_bad_argument_before_anything_is_launched(change):
  assert _args(**change) == -1


def test_the_launch_validator_refuses_a_null_struct():
  assert _hip.lib.campx_returns_launch(None, B, T, None) == -1


def test_the_entry_point_is_exported():
  assert 'campx_returns_launch' in _hip.EXPORTS and hasattr(_hip.lib, 'campx_returns_launch')
