"""The V-trace rule of `vtrace_returns()` without a GPU: tests/vtrace_reference.py (the rule of
include/campx_hip.h in numpy float32) reduces to `discounted_returns()`'s advantages on policy,
to the one-step error under c_bar = 0, stops at a `done`, ignores NaN rewards and differs from two
deliberately wrong variants; `campx_vtrace_launch()` refuses every bad argument before anything is
launched and `campx_vtrace_plan()`, pure host code, places the tables by `table_lookup()`'s rule."""

import ctypes

import numpy as np
import pytest

import returns_reference as returns_ref
import vtrace_reference as ref
from campx_amd import _hip

F = np.float32
GAMMA = 0.99
T, B = 100, 257


def _x():
  return ref.inputs(T, B)


@pytest.mark.parametrize('lam', [1.0, 0.95, 0.0])
@pytest.mark.parametrize('with_discount', [True, False])
def test_on_policy_it_is_the_returns_rule_bit_for_bit(lam, with_discount):
  """w == 1 and bars of 1: a multiplication by 1.0 is exact, so D is `discounted_returns()`'s A and
  vs is values + A in float32."""
  x = _x()
  discount = x['discount'] if with_discount else None
  got = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], np.ones((T, B), F), discount=discount,
                   bootstrap=x['bootstrap'], lam=lam)
  _, A = returns_ref.returns(x['reward'], x['done'], GAMMA, discount, x['values'], x['bootstrap'], lam)
  assert ref.same_bits(got['D'], A)
  assert ref.same_bits(got['vs'], np.add(x['values'], A))
  assert not np.isnan(got['vs']).any() and not np.isnan(got['advantages']).any()


def test_c_bar_zero_leaves_the_one_step_error():
  """cs = 0 for every frame: D == delta = rho * (q - v).  Compared as numbers: the sum
  delta + 0 * D[t+1] turns a delta of -0.0 (rho = 0 times a negative error) into +0.0."""
  x = _x()
  w = ref.ratios(T, B)
  got = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], w, discount=x['discount'],
                   bootstrap=x['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.0, pg_rho_bar=3.0)
  assert np.array_equal(got['D'], got['delta']) and not np.isnan(got['D']).any()
  # ... and delta is what the rule says, restated without the loop
  r = np.where(np.isnan(x['reward']), F(0), x['reward'])
  c = np.multiply(F(GAMMA), x['discount'])
  v_next = np.concatenate([x['values'][1:], x['bootstrap'][None]])
  q = np.where(x['done'] != 0, r, np.add(r, np.multiply(c, v_next)))
  rho = np.where(w > 0, w, F(0))
  rho = np.where(rho < F(2.0), rho, F(2.0)).astype(F)
  assert ref.same_bits(got['delta'], np.multiply(rho, np.subtract(q, x['values'])))
  # a ratio of NaN, -1 or 0 has rho = 0: vs is the value itself
  dead = np.isnan(w) | (w <= 0)
  assert dead.sum() > T * B // 8 and np.array_equal(got['vs'][dead], x['values'][dead])


def test_done_nan_rewards_and_the_forced_columns():
  x = _x()
  w = ref.ratios(T, B)
  kw = dict(discount=x['discount'], lam=0.95, rho_bar=2.0, c_bar=0.5, pg_rho_bar=3.0)
  got = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], w, bootstrap=x['bootstrap'], **kw)
  assert np.isnan(x['reward']).any() and np.isnan(w).any() and np.isinf(w).any() and (w < 0).any()
  for k in ('vs', 'advantages', 'D'):
    assert not np.isnan(got[k]).any(), k
  f = x['forced']
  r = np.where(np.isnan(x['reward']), F(0), x['reward'])
  wc = np.where(w > 0, w, F(0))
  rho = np.where(wc < F(2.0), wc, F(2.0)).astype(F)
  rpg = np.where(wc < F(3.0), wc, F(3.0)).astype(F)
  # the all-done column: every frame is its own episode, D = rho * (r - v), adv = rpg * (r - v)
  e = f['all']
  err = np.subtract(r[:, e], x['values'][:, e])
  assert ref.same_bits(got['D'][:, e], np.multiply(rho[:, e], err))
  assert ref.same_bits(got['advantages'][:, e], np.multiply(rpg[:, e], err))
  # the bootstrap reaches no frame of the column whose last frame is done, and frame T - 1 of the
  # never-done column unless its discount is 0
  without = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], w, bootstrap=None, **kw)
  for k in ('vs', 'advantages'):
    assert ref.same_bits(got[k][:, f['last']], without[k][:, f['last']]), k
  e = f['never']
  if x['discount'][T - 1, e] != 0 and x['bootstrap'][e] != 0 and rpg[T - 1, e] > 0:
    assert not ref.same_bits(got['advantages'][-1:, e], without['advantages'][-1:, e])
  # nothing is carried across a done: what follows frame 0 of the first-done column leaves it alone
  e = f['first']
  assert ref.same_bits(got['D'][0, e], got['delta'][0, e])
  # +inf is clipped to the bars, like any ratio above them
  big = np.isinf(w)
  assert np.array_equal(rho[big], np.full(big.sum(), 2.0, F)) and np.array_equal(rpg[big], np.full(big.sum(), 3.0, F))


@pytest.mark.parametrize('variant', ['clip_after_product', 'carry_across_done'])
def test_a_wrong_variant_differs(variant):
  x = _x()
  w = ref.ratios(T, B)
  kw = dict(discount=x['discount'], bootstrap=x['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.5, pg_rho_bar=3.0)
  good = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], w, **kw)
  wrong = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], w, variant=variant, **kw)
  differs = good['vs'].view(np.uint32) != wrong['vs'].view(np.uint32)
  assert differs.mean() > 0.05
  if variant == 'carry_across_done':
    assert not differs[:, x['forced']['never']].any()       # (no done, nothing to carry across)


def test_the_table_ratio_is_the_quotient_of_the_two_tables():
  Nt, Nb, A = 8, 24, 5
  target, behaviour = ref.tables(Nt, Nb)
  states, actions = ref.ids(9, 65, Nb)
  states[0, :3], actions[1, :3] = [-1, Nb, 2 ** 31 - 1], [-1, 5, 127]
  w0, bad = ref.table_ratio(target, behaviour, states, actions)
  assert bad == 6 and not w0[0, :3].any() and not w0[1, :3].any()
  assert w0[5, 7] == F(target[states[5, 7] % Nt, actions[5, 7]]) / F(behaviour[states[5, 7], actions[5, 7]])
  assert (w0 > 2.0).any() and ((w0 > 0) & (w0 < 0.5)).any()


# ------------------------------------------------------------------ the C ABI, host side

def _plan(Nt, Nb, A, B, T, path=0):
  out = (ctypes.c_int64 * 3)()
  code = _hip.lib.campx_vtrace_plan(Nt, Nb, A, B, T, path, out)
  return code, dict(zip(('path', 'lds_bytes', 'grid'), (int(v) for v in out)))


def test_the_entry_points_are_exported():
  assert 'campx_vtrace_launch' in _hip.EXPORTS and 'campx_vtrace_plan' in _hip.EXPORTS
  assert hasattr(_hip.lib, 'campx_vtrace_launch') and hasattr(_hip.lib, 'campx_vtrace_plan')
  assert 'vtrace' in _hip.OP_NAMES


def test_the_plan_stages_the_tables_on_both_sides_of_both_bounds():
  budget = _hip.SUMS_LDS_BUDGET
  # the boat race: 8 states, P = 1 and P = 16
  for Nb in (8, 128):
    code, p = _plan(8, Nb, 5, 4096, 100)
    assert code == 0 and p == dict(path=1, lds_bytes=(8 + Nb) * 5 * 4, grid=16)
  # the budget: (Nt + Nb) * A * 4 <= 49152, i.e. 12288 entries
  assert budget == 49152
  code, p = _plan(1024, 2048, 4, 65536, 100)               # 12288 entries: fits
  assert code == 0 and p['path'] == 1 and p['lds_bytes'] == budget and p['grid'] == 256
  code, p = _plan(1, 12288, 1, 65536, 100)                 # 12289 entries: one too many
  assert code == 0 and p['path'] == 2 and p['lds_bytes'] == 0
  assert _plan(1, 12288, 1, 65536, 100, path=1)[0] == -1   # and cannot be forced into LDS
  assert _plan(1024, 2048, 4, 65536, 100, path=2)[1]['path'] == 2
  # the entries against the frames a workgroup looks up, 256 * T
  code, p = _plan(128, 128, 5, 257, 5)                     # 1280 entries = 256 * 5
  assert code == 0 and p['path'] == 1 and p['grid'] == 2
  code, p = _plan(128, 128, 5, 257, 4)                     # 1280 > 1024: through the caches ...
  assert code == 0 and p['path'] == 2
  code, p = _plan(128, 128, 5, 257, 4, path=1)             # ... unless forced
  assert code == 0 and p['path'] == 1 and p['lds_bytes'] == 1280 * 4
  # 2 500 states twice pass the budget
  assert _plan(2500, 2500, 5, 257, 9)[1]['path'] == 2 and _plan(2500, 2500, 5, 257, 9, path=1)[0] == -1


def test_the_plan_refuses_bad_sizes():
  good = dict(Nt=8, Nb=24, A=5, B=4096, T=100, path=0)
  assert _plan(**good)[0] == 0
  for bad in (dict(Nt=0), dict(Nt=-1), dict(Nb=0), dict(Nb=25), dict(Nb=4), dict(Nt=1 << 31, Nb=1 << 31),
              dict(Nt=1, Nb=1 << 31), dict(A=0), dict(A=129), dict(B=0), dict(B=(1 << 31) + 1), dict(T=0),
              dict(path=-1), dict(path=3)):
    assert _plan(**dict(good, **bad))[0] == -1, bad
  assert _plan(1, (1 << 31) - 1, 128, 1 << 31, 0x7fffffff)[0] == 0
  assert _hip.lib.campx_vtrace_plan(8, 24, 5, 4096, 100, 0, None) == -1


_NAN, _INF = float('nan'), float('inf')


def _args(mode, **change):
  """A CampxVtrace whose pointers are fake but aligned, non-NULL addresses: every call below is
  refused by the validator, so none is ever dereferenced."""
  B, T = 65, 9
  v = _hip.CampxVtrace()
  v.reward, v.done, v.discount, v.values, v.bootstrap = 0x1000, 0x2001, 0x3000, 0x4000, 0x5000
  v.vs, v.advantages, v.bad_count = 0x6000, 0x7000, 0x8000
  if mode == 'ratio':
    v.ratio = 0x9000
  else:
    v.target, v.behaviour, v.states, v.actions = 0xa000, 0xb000, 0xc000, 0xd001
    v.n_target_states, v.n_behaviour_states, v.n_actions = 8, 24, 5
  for k in ('reward', 'done', 'discount', 'values', 'ratio', 'states', 'actions', 'vs', 'advantages'):
    setattr(v, k + '_pitch', B)
  v.gamma, v.lam, v.rho_bar, v.c_bar, v.pg_rho_bar = 0.99, 0.95, 1.0, 1.0, 1.0
  for k, x in change.items():
    if k not in ('B', 'T'):
      setattr(v, k, x)
  return _hip.lib.campx_vtrace_launch(ctypes.byref(v), change.get('B', B), change.get('T', T), None)


def test_the_launch_validator_refuses_bad_arguments_before_anything_is_launched():
  both = [dict(reward=None), dict(done=None), dict(values=None), dict(vs=None), dict(advantages=None),
          dict(reward=0x1002), dict(discount=0x3001), dict(values=0x4002), dict(bootstrap=0x5002),
          dict(vs=0x6001), dict(advantages=0x7002), dict(bad_count=0x8004),
          dict(reward_pitch=64), dict(done_pitch=64), dict(discount_pitch=64), dict(values_pitch=64),
          dict(vs_pitch=64), dict(advantages_pitch=64), dict(vs_pitch=1 << 40), dict(reward_pitch=-1),
          dict(B=0), dict(B=-1), dict(B=(1 << 31) + 1), dict(T=0), dict(T=-1),
          dict(gamma=_NAN), dict(gamma=_INF), dict(lam=_NAN), dict(lam=-_INF),
          dict(rho_bar=_NAN), dict(rho_bar=_INF), dict(rho_bar=-0.5), dict(c_bar=_NAN), dict(c_bar=_INF),
          dict(c_bar=-1.0), dict(pg_rho_bar=_NAN), dict(pg_rho_bar=_INF), dict(pg_rho_bar=-2.0),
          dict(path=-1), dict(path=3)]
  ratio = [dict(ratio=None), dict(ratio=0x9002), dict(ratio_pitch=64),
           dict(target=0xa000), dict(states=0xc000), dict(target=0xa000, behaviour=0xb000),
           dict(target=0xa000, behaviour=0xb000, states=0xc000, actions=0xd001, n_target_states=8,
                n_behaviour_states=8, n_actions=5)]
  table = [dict(ratio=0x9000), dict(target=None), dict(behaviour=None), dict(states=None), dict(actions=None),
           dict(target=0xa002), dict(behaviour=0xb001), dict(states=0xc002), dict(states_pitch=64),
           dict(actions_pitch=64), dict(n_target_states=0), dict(n_target_states=-8),
           dict(n_behaviour_states=25), dict(n_behaviour_states=0), dict(n_behaviour_states=4),
           dict(n_target_states=1 << 31, n_behaviour_states=1 << 31),
           dict(n_target_states=1, n_behaviour_states=1 << 31), dict(n_actions=0), dict(n_actions=129),
           dict(path=1, n_target_states=2500, n_behaviour_states=2500)]
  for mode, cases in (('ratio', both + ratio), ('table', both + table)):
    for change in cases:
      assert _args(mode, **change) == -1, (mode, change)
  assert _hip.lib.campx_vtrace_launch(None, 65, 9, None) == -1


# ------------------------------------------------------------------ the Python call

def test_python_argument_errors_raise_value_error():
  """What can be refused without a device: the scalars, the mode, and tensors that are not on one
  (there is no CPU path).  tests/test_vtrace.py has the tensor contracts, on the GPU."""
  import torch
  from campx_amd.returns import vtrace_returns
  x = ref.inputs(9, 65)
  reward, done, values = (torch.from_numpy(x[k]) for k in ('reward', 'done', 'values'))
  ratio = torch.ones((9, 65))
  target, behaviour = (torch.from_numpy(t) for t in ref.tables(8, 8))
  states, actions = (torch.from_numpy(t) for t in ref.ids(9, 65, 8))
  good = dict(reward=reward, done=done, gamma=GAMMA, values=values, ratio=ratio)
  tabled = dict(good, ratio=None, target=target, behaviour=behaviour, states=states, actions=actions)
  bad = {
      'gamma nan': dict(good, gamma=_NAN), 'gamma inf': dict(good, gamma=_INF), 'gamma type': dict(good, gamma='0.99'),
      'lam nan': dict(good, lam=_NAN), 'lam bool': dict(good, lam=True),
      'rho_bar negative': dict(good, rho_bar=-1.0), 'rho_bar inf': dict(good, rho_bar=_INF),
      'c_bar nan': dict(good, c_bar=_NAN), 'c_bar type': dict(good, c_bar=None),
      'pg_rho_bar negative': dict(good, pg_rho_bar=-0.5), 'pg_rho_bar inf': dict(good, pg_rho_bar=_INF),
      'path 3': dict(good, path=3), 'path float': dict(good, path=1.0),
      'neither': dict(good, ratio=None), 'both': dict(tabled, ratio=ratio),
      'no target': dict(tabled, target=None), 'no behaviour': dict(tabled, behaviour=None),
      'no states': dict(tabled, states=None), 'no actions': dict(tabled, actions=None),
      'reward not a tensor': dict(good, reward=x['reward']), 'reward dtype': dict(good, reward=reward.double()),
      'reward rank': dict(good, reward=reward[0]),
      'no CPU path, ratio mode': good, 'no CPU path, table mode': tabled,
  }
  for what, kwargs in bad.items():
    with pytest.raises(ValueError):
      vtrace_returns(**kwargs)
      pytest.fail('no ValueError for: ' + what)
