"""The f32 rules at the edges of float32, on the GPU: `discounted_returns()` (csrc/k_returns.hip),
`evaluate_policy()` / `value_iteration()` (csrc/k_plan.hip), `rollout_policy()` and
`state_visitation()` (the row rule of csrc/wide_table.hip.h in csrc/k_policy.hip and
csrc/k_visit.hip) and `learn_tabular()` (csrc/k_learn.hip) against their numpy restatements on the
input sets of tests/float_edges.py - subnormals, signed zeros, overflow to infinity, `0 * inf`,
`inf - inf`, NaN.  Every float comparison is `same_bits_or_nan`: NaN in the same places, the same
bits everywhere else; there is no tolerance.  tests/test_float_edges_cpu.py shows, from the
references alone, that the sets reach those edges.

A difference here is a finding about a kernel or about `HIPCC_FLAGS` in campx_amd/build.py - a
flushed denormal, a fused or `mad`-style multiply-add, the sign of a zero lost in a select - not
about the test.
"""

import re
import types

import numpy as np
import pytest
import torch

import float_edges as fe
import learner_reference as learn_ref
from test_policy_rollout import _check_against_walk
from test_returns import _game as _boat_race, _padded, up16

pytestmark = pytest.mark.gpu

same = fe.same_bits_or_nan


def _wide(table, batch=1):
  from campx_amd import wide
  f = wide.WideGame(types.SimpleNamespace(rows=table.rows, cols=table.cols), batch, 'cuda', table)
  assert f.n_states == table.n_states
  return f


# ------------------------------------------------------------------ returns

def _returns_device(leg, layout):
  x = fe.returns_inputs(leg)
  T, B = fe.RETURNS_T, fe.RETURNS_B
  if layout == 'dense':
    return {k: torch.from_numpy(x[k]).cuda() for k in ('reward', 'done', 'discount', 'values', 'bootstrap')}
  bufs = _boat_race(B).rollout_trace_buffers(T)        # reward / discount / done: rows padded to 16
  assert bufs['reward'].stride(0) == up16(B)
  d = {}
  for k in ('reward', 'done', 'discount'):
    bufs[k].copy_(torch.from_numpy(x[k]))
    d[k] = bufs[k]
  d['values'] = _padded(x['values'], B + 7)
  d['bootstrap'] = torch.from_numpy(x['bootstrap']).cuda()
  return d


@pytest.mark.parametrize('layout', ['dense', 'padded'])
@pytest.mark.parametrize('leg', fe.RETURNS_LEGS)
def test_returns_and_advantages_at_the_edges(leg, layout):
  from campx_amd.returns import discounted_returns
  T, B = fe.RETURNS_T, fe.RETURNS_B
  d = _returns_device(leg, layout)
  runs = fe.returns_inputs(leg)['runs']
  for i, (gamma, lam) in enumerate(runs):
    for with_discount, with_values in fe.COMBOS:
      out = None
      if layout == 'padded':
        out = {'returns': torch.zeros((T, B + 3), dtype=torch.float32, device='cuda')[:, :B]}
        if with_values:
          out['advantages'] = torch.zeros((T, up16(B) + 16), dtype=torch.float32, device='cuda')[:, :B]
      got = discounted_returns(d['reward'], d['done'], gamma, discount=d['discount'] if with_discount else None,
                               values=d['values'] if with_values else None, bootstrap=d['bootstrap'],
                               lam=lam, out=out)
      G, A = fe.returns_want(leg, i, with_discount, with_values)
      what = (leg, layout, gamma, lam, with_discount, with_values)
      assert set(got) == ({'returns', 'advantages'} if with_values else {'returns'}), what
      assert same(got['returns'].cpu().numpy(), G), what
      if with_values:
        assert same(got['advantages'].cpu().numpy(), A), what


# ------------------------------------------------------------------ sweeps

def _fits(S, policy):
  import ctypes
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  return _hip.lib.campx_wide_sweeps_plan(S, policy, 1, _hip.config_get('wide_lds_max'), 1, out) == 0


def _check_sweeps(res, want, n, greedy, what):
  assert res['sweeps'] == n
  for k in ('values', 'q', 'residual'):
    assert same(res[k].cpu().numpy(), want[k]), (what, k)
  if greedy:
    assert np.array_equal(res['greedy'].cpu().numpy(), want['greedy']), (what, 'greedy')


@pytest.mark.parametrize('S', fe.SWEEP_SIZES)
@pytest.mark.parametrize('leg', sorted(fe.SWEEP_LEGS))
def test_sweeps_at_the_edges_on_both_paths(leg, S):
  g, x = fe.sweep_table(S), fe.sweep_inputs(leg, S)
  f = _wide(g)
  f.validate_actions = 'sync'
  gamma = x['gamma']
  reward = torch.from_numpy(x['reward']).cuda()
  values = torch.from_numpy(x['values']).cuda()
  w = fe.sweep_policy(leg, S)
  policy = torch.from_numpy(w).cuda()
  ran = 0
  for n in fe.SWEEP_COUNTS:
    # ---- the value of a policy
    want = fe.sweep_want(leg, S, n, True)
    n_bad = want['bad_rows']
    assert (n_bad >= 3) == (leg == 'rows')
    for path in ([1] if _fits(S, 1) else []) + [2]:
      what = (leg, S, n, 'policy', path)
      if n_bad:
        out = f.sweep_buffers(n, greedy=False)
        with pytest.raises(ValueError, match='^{} rows of the policy given to evaluate_policy'.format(n_bad)):
          f.evaluate_policy(policy, gamma, n, values=values, reward=reward, out=out, path=path)
        res = dict(out, sweeps=n)
      else:
        res = f.evaluate_policy(policy, gamma, n, values=values, reward=reward, path=path)
      _check_sweeps(res, want, n, False, what)
      ran += 1
    # ---- value iteration
    want = fe.sweep_want(leg, S, n, False)
    for path in ([1] if _fits(S, 0) else []) + [2]:
      res = f.value_iteration(gamma, n, values=values, reward=reward, path=path)
      _check_sweeps(res, want, n, True, (leg, S, n, 'greedy', path))
      ran += 1
  assert ran == 12                                      # path 1 fits all three sizes
  assert same(values.cpu().numpy(), x['values'])        # the values given are left as they are
  f.check_actions()


# ------------------------------------------------------------------ sampler

def test_rollout_policy_samples_the_edge_rows_as_the_reference_does():
  B, T = fe.SAMPLER_B, fe.SAMPLER_T
  g = fe.sweep_table(fe.SAMPLER_S)
  f = _wide(g, batch=B)
  f.showtime()
  walker, want = fe.sampler_want()
  assert want['bad'] > 0
  policy = torch.from_numpy(fe.edge_policy(fe.SAMPLER_S)).cuda()
  bufs = f.rollout_policy_buffers(T)
  with pytest.raises(ValueError, match='bad policy rows') as e:
    f.rollout_policy(policy, T, seed=fe.SAMPLER_SEED, first_frame=fe.SAMPLER_FIRST, reset_first=True, out=bufs)
    f.check_actions()
  count = int(re.match(r'(\d+) environment-frames of rollout_policy\(\) met bad policy rows',
                       str(e.value)).group(1))
  assert count == want['bad']
  torch.cuda.synchronize()
  _check_against_walk(f, bufs, want, walker)
  f.check_actions()


def test_state_visitation_counts_the_edge_rows_as_the_reference_does():
  g = fe.sweep_table(fe.SAMPLER_S)
  f = _wide(g)
  want = fe.visitation_want()
  policy = torch.from_numpy(fe.edge_policy(fe.SAMPLER_S)).cuda()
  message = '^{} rows of the policy given to state_visitation'.format(want['bad_rows'])
  for path in (1, 2):
    out = f.visitation_buffers(fe.SAMPLER_T, want_frames=True)
    try:                       # (lazily: from the call if the flag is up when it looks, else here)
      f.state_visitation(policy, fe.SAMPLER_T, want_frames=True, out=out, path=path)
    except ValueError as e:
      assert re.match(message, str(e))
    else:
      with pytest.raises(ValueError, match=message):
        f.check_actions()
    for k in ('counts', 'visits', 'finished', 'final', 'per_frame'):
      got = out[k].cpu().numpy()
      assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (path, k)
    f.check_actions()


# ------------------------------------------------------------------ learner

@pytest.mark.parametrize('path', [1, 2])
@pytest.mark.parametrize('rule', learn_ref.RULES)
def test_learners_at_the_edges(rule, path):
  B, T = fe.LEARN_B, fe.LEARN_T
  g, x = fe.learner_table(), fe.learner_inputs()
  f = _wide(g, batch=B)
  f.showtime()
  f.validate_actions = 'sync'
  q = torch.from_numpy(x['q']).cuda()
  res = f.learn_tabular(T, q, torch.from_numpy(x['alpha']).cuda(), torch.from_numpy(x['gamma']).cuda(),
                        torch.from_numpy(x['epsilon']).cuda(), rule, fe.LEARN_SEED, fe.LEARN_FIRST,
                        window=fe.LEARN_WINDOW, path=path)
  L, want = fe.learner_want(rule)
  assert res['q'] is q and same(q.cpu().numpy(), L.q), 'q'
  assert same(res['reward_sum'].cpu().numpy(), want['reward_sum']), 'reward_sum'
  assert np.array_equal(res['perf_sum'].cpu().numpy(), want['perf_sum']), 'perf_sum'
  assert np.array_equal(res['episodes'].cpu().numpy(), want['episodes']), 'episodes'
  assert np.array_equal(f.state.cpu().numpy(), L.state)
  assert np.array_equal(f.done.cpu().numpy(), L.over.astype(np.uint8))
  assert same(f.ret.cpu().numpy(), L.ret)
  f.check_actions()                                     # no learner is bad: every hyper-parameter is finite
