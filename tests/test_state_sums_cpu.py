"""The fixed-point rule of `sum_by_state()` without a GPU: tests/state_sums_reference.py (the rule
of include/campx_hip.h in numpy) is order-independent, accurate to the derived bound and treats
the corner cases as the header says; and `campx_state_sums_plan()`, pure host code, chooses the
accumulation path by the arithmetic the header describes."""

import ctypes
import math

import numpy as np
import pytest

import state_sums_reference as ref
from campx_amd import _hip


def test_the_sums_do_not_depend_on_the_order_of_the_frames():
  T, B, S, A, K = 9, 257, 8, 5, 4
  x = ref.inputs(T, B, S, A, K, dirty=True)
  want = ref.state_sums(x['states'], x['actions'], x['values'], S, A)
  assert want['skipped'] > 0 and want['clamped'] > 0
  perm = np.random.RandomState(3).permutation(T * B)
  shuffled = lambda a: a.reshape(-1)[perm].reshape(T, B)
  got = ref.state_sums(shuffled(x['states']), shuffled(x['actions']),
                       [shuffled(v) for v in x['values']], S, A)
  assert np.array_equal(got['raw'], want['raw'])
  assert (got['skipped'], got['clamped']) == (want['skipped'], want['clamped'])
  # and not by accident of the values: float32 sums of the same two orders do differ
  v = x['values'][1].reshape(-1)
  keep = np.isfinite(v) & (np.abs(v) < 10)
  a = np.cumsum(v[keep], dtype=np.float32)[-1]
  b = np.cumsum(v[keep][::-1], dtype=np.float32)[-1]
  assert a != b


@pytest.mark.parametrize('frac_bits', [0, 10, 24, 40])
def test_the_float_sums_are_within_half_a_quantum_per_contribution(frac_bits):
  """Each contribution is rounded once, by at most half a quantum: per bin
  |raw * 2^-f - exact| <= n_bin * 2^-(f + 1), the exact sum by math.fsum on doubles."""
  T, B, S, A, K = 9, 257, 8, 5, 4
  x = ref.inputs(T, B, S, A, K)
  got = ref.state_sums(x['states'], x['actions'], x['values'], S, A, frac_bits=frac_bits)
  assert got['clamped'] == 0 and got['skipped'] == 0
  bins = x['states'].astype(np.int64).reshape(-1) * A + x['actions'].reshape(-1)
  assert got['raw'][0].sum() == T * B
  for k in range(K):
    v = x['values'][k].astype(np.float64).reshape(-1)
    for b in range(S * A):
      n = int(got['raw'][0][b])
      assert n == int((bins == b).sum())
      exact = math.fsum(v[bins == b])
      # raw is below 2^53 here, so the product is exact
      assert abs(float(got['raw'][1 + k][b]) * 2.0 ** -frac_bits - exact) <= n * 2.0 ** -(frac_bits + 1)


def test_corner_cases_clamp_and_skip_and_are_counted():
  S, A, f = 3, 5, 24
  N = 16                                           # n2 = 4, lim = 2^58 quanta = 2^34 in value
  n2, lim = ref.limits(N)
  assert (n2, lim) == (4, 1 << 58) and ref.limits(1) == (0, 1 << 62) and ref.limits(17)[0] == 5
  edge = np.float32(2.0 ** 34)
  values = np.array([[1.5, np.nan, np.inf, -np.inf, 3e30, -3e30, edge, -edge,
                      np.nextafter(edge, np.float32(np.inf)), 0.25, 2.0 ** -25, 3 * 2.0 ** -25,
                      2.0 ** -26, 7.0, 7.0, 7.0]], dtype=np.float32)
  states = np.array([[0] * 13 + [-1, 3, 1]], dtype=np.int32)
  actions = np.array([[0] * 12 + [5, 0, 0, -1]], dtype=np.int8)
  got = ref.state_sums(states, actions, [values], S, A, frac_bits=f)
  assert got['skipped'] == 4                       # action 5, state -1, state 3, action -1
  assert got['clamped'] == 6                       # NaN, +-Inf, +-3e30, the value just past the limit
  assert got['raw'][0][0] == 12 and got['raw'][0].sum() == 12
  # 1.5; NaN -> 0; +lim - lim twice; +-edge are exactly +-lim and not clamped; the value past it -> lim;
  # 0.25; ties to even: 2^-25 -> 0, 3 * 2^-25 -> 2; 2^-26 -> 0
  want = int(1.5 * 2 ** f) + 0 + lim - lim + lim - lim + lim - lim + lim + (1 << (f - 2)) + 0 + 2 + 0
  assert int(got['raw'][1][0]) == want
  assert not got['raw'][1][1:].any()
  # per state, without an action stream
  per_state = ref.state_sums(states, None, [values], S, frac_bits=f)
  assert per_state['raw'].shape == (2, S) and per_state['skipped'] == 2
  assert list(per_state['raw'][0]) == [13, 1, 0]
  # N additions of lim stay inside an int64
  full = ref.state_sums(np.zeros((1, N), np.int32), None, [np.full((1, N), np.inf, np.float32)], 1,
                        frac_bits=f)
  assert int(full['raw'][1][0]) == 1 << 62 and full['clamped'] == N


def _plan(S, A, K, B, T, frac_bits=24, path=0):
  out = (ctypes.c_int64 * 8)()
  code = _hip.lib.campx_state_sums_plan(S, A, K, B, T, frac_bits, path, out)
  keys = ('path', 'copies', 'grid_b', 'grid_t', 'frames', 'lds_bytes', 'n2', 'lim_bits')
  return code, dict(zip(keys, (int(v) for v in out)))


def test_the_plan_is_exported():
  assert 'campx_state_sums_plan' in _hip.EXPORTS and 'campx_state_sums_launch' in _hip.EXPORTS
  assert 'campx_table_lookup_launch' in _hip.EXPORTS
  assert 'state_sums' in _hip.OP_NAMES and 'table_lookup' in _hip.OP_NAMES


@pytest.mark.parametrize('B', [4096, 65536])
def test_a_boat_race_plans_the_lds_path_with_several_copies(B):
  for K in (0, 1, 4):
    code, p = _plan(8, 5, K, B, 100)
    assert code == 0
    assert p['path'] == 1 and p['copies'] > 1 and p['copies'] & (p['copies'] - 1) == 0
    assert p['lds_bytes'] == 40 * (K + 1) * p['copies'] * 8 <= _hip.SUMS_LDS_BUDGET
    assert p['grid_b'] == B // 256 and p['frames'] % 8 == 0
    assert (p['grid_t'] - 1) * p['frames'] < 100 <= p['grid_t'] * p['frames']
    assert p['n2'] == ref.limits(100 * B)[0] and p['lim_bits'] == 62 - p['n2']


def test_accumulators_too_large_for_lds_plan_the_global_path():
  for S, A, K in ((4400000, 5, 1), (1940, 5, 0), (70000, 1, 0), (16, 128, 4)):
    assert S * A * (K + 1) * 8 > _hip.SUMS_LDS_BUDGET
    code, p = _plan(S, A, K, 65536, 100)
    assert code == 0 and p['path'] == 2 and p['copies'] == 1 and p['lds_bytes'] == 0
    assert _plan(S, A, K, 65536, 100, path=1)[0] != 0          # and cannot be forced into LDS
    assert _plan(S, A, K, 65536, 100, path=2)[1]['path'] == 2
  # a table that fits but whose flush would not be small against a workgroup's frames: global,
  # unless forced
  code, p = _plan(1940, 1, 0, 257, 9)
  assert code == 0 and p['path'] == 2
  code, p = _plan(1940, 1, 0, 257, 9, path=1)
  assert code == 0 and p['path'] == 1 and p['copies'] >= 1 and p['lds_bytes'] == 1940 * 8 * p['copies']


def test_the_planned_lds_never_exceeds_the_budget():
  sizes = sorted(set([1, 2, 3, 5, 7, 8, 9, 40, 153, 154, 191, 192, 193, 767, 768, 769, 1228, 1229,
                      1940, 3071, 3072, 3073, 6143, 6144, 6145, 70000, 1 << 20, (1 << 24) - 1,
                      1 << 24] + [1 << i for i in range(25)]
                     + [int(v) for v in np.random.RandomState(0).randint(1, 1 << 24, size=200)]))
  for S in sizes:
    for A in (1, 5):
      for K in range(5):
        for B, T in ((257, 9), (4096, 100), (65536, 100)):
          for path in (0, 1, 2):
            code, p = _plan(S, A, K, B, T, path=path)
            fits = S * A * (K + 1) * 8 <= _hip.SUMS_LDS_BUDGET
            if path == 1 and not fits:
              assert code != 0
              continue
            assert code == 0, (S, A, K, B, T, path)
            assert 0 <= p['lds_bytes'] <= _hip.SUMS_LDS_BUDGET
            assert p['path'] in (1, 2) and (path == 0 or p['path'] == path)
            if p['path'] == 1:
              assert fits and p['lds_bytes'] == S * A * (K + 1) * 8 * p['copies']
              assert 1 <= p['copies'] <= 64
            else:
              assert p['lds_bytes'] == 0 and p['copies'] == 1
            assert 1 <= p['grid_t'] <= 65535 and p['grid_b'] == (B + 255) // 256


def test_the_plan_refuses_what_the_rule_cannot_hold():
  # N = 100 * 65536 < 2^23: n2 = 23, frac_bits up to 39
  assert _plan(8, 5, 1, 65536, 100, frac_bits=39)[0] == 0
  assert _plan(8, 5, 1, 65536, 100, frac_bits=40)[0] != 0
  assert _plan(8, 5, 1, 1, 1, frac_bits=62)[0] == 0 and _plan(8, 5, 1, 1, 1, frac_bits=63)[0] != 0
  assert _plan(8, 5, 1, 1 << 31, 0x7fffffff, frac_bits=0)[0] == 0      # n2 = 62
  assert _plan(8, 5, 1, 1 << 31, 0x7fffffff, frac_bits=1)[0] != 0
  for bad in (dict(S=0), dict(S=1 << 31), dict(A=0), dict(A=129), dict(K=-1), dict(K=5), dict(B=0),
              dict(B=(1 << 31) + 1), dict(T=0), dict(frac_bits=-1), dict(path=3), dict(path=-1)):
    args = dict(dict(S=8, A=5, K=1, B=4096, T=100, frac_bits=24, path=0), **bad)
    assert _plan(**args)[0] != 0, bad
  assert _hip.lib.campx_state_sums_plan(8, 5, 1, 4096, 100, 24, 0, None) != 0


def _sums_args(**change):
  """A CampxStateSums whose pointers are fake but aligned, non-NULL addresses: every call below is
  refused by the validator, so none is ever dereferenced."""
  B, T = 65, 9
  s = _hip.CampxStateSums()
  s.states, s.actions, s.acc, s.skipped, s.clamped = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
  s.values[0] = 0x6000
  s.states_pitch = s.actions_pitch = B
  s.values_pitch[0] = B
  s.n_states, s.n_actions, s.n_values, s.frac_bits = 8, 5, 1, 24
  for k, v in change.items():
    if k == 'values0':
      s.values[0] = v
    elif k == 'values_pitch0':
      s.values_pitch[0] = v
    elif k not in ('B', 'T'):
      setattr(s, k, v)
  return s, change.get('B', B), change.get('T', T)


def test_the_launch_validators_refuse_bad_arguments_before_anything_is_launched():
  bad = [dict(states=None), dict(acc=None), dict(skipped=None), dict(clamped=None), dict(values0=None),
         dict(states=0x1002), dict(acc=0x3004), dict(skipped=0x4004), dict(clamped=0x5001),
         dict(values0=0x6002), dict(states_pitch=64), dict(actions_pitch=64), dict(values_pitch0=64),
         dict(states_pitch=1 << 40), dict(n_states=0), dict(n_states=1 << 31), dict(n_actions=0),
         dict(n_actions=129), dict(actions=None), dict(n_values=5), dict(n_values=-1),
         dict(frac_bits=-1), dict(frac_bits=62 - 10 + 1), dict(path=3), dict(path=1, n_states=70000),
         dict(B=0), dict(T=0), dict(B=(1 << 31) + 1)]
  for change in bad:
    s, B, T = _sums_args(**change)
    assert _hip.lib.campx_state_sums_launch(ctypes.byref(s), B, T, None) == -1, change
  assert _hip.lib.campx_state_sums_launch(None, 65, 9, None) == -1
  # 9 * 65 = 585 frames: n2 = 10, so frac_bits 52 is the last the plan takes
  assert _plan(8, 5, 1, 65, 9, frac_bits=52)[0] == 0 and _plan(8, 5, 1, 65, 9, frac_bits=53)[0] != 0

  def lookup(**change):
    l = _hip.CampxTableLookup()
    l.table, l.states, l.actions, l.out, l.bad_count = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    l.states_pitch = l.actions_pitch = l.out_pitch = 65
    l.n_states, l.n_actions = 8, 5
    for k, v in change.items():
      if k not in ('B', 'T'):
        setattr(l, k, v)
    return _hip.lib.campx_table_lookup_launch(ctypes.byref(l), change.get('B', 65), change.get('T', 9), None)
  for change in [dict(table=None), dict(states=None), dict(out=None), dict(table=0x1002),
                 dict(states=0x2001), dict(out=0x4002), dict(bad_count=0x5004), dict(states_pitch=64),
                 dict(actions_pitch=64), dict(out_pitch=64), dict(out_pitch=1 << 40), dict(n_states=0),
                 dict(n_states=1 << 31), dict(n_actions=0), dict(n_actions=129), dict(actions=None),
                 dict(B=0), dict(T=0)]:
    assert lookup(**change) == -1, change
  assert _hip.lib.campx_table_lookup_launch(None, 65, 9, None) == -1
