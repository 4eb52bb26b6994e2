"""The V-trace rule at the edges of float32, on the GPU: `vtrace_returns()` (csrc/k_vtrace.hip)
against tests/vtrace_reference.py on the input sets of tests/float_edges.py - the streams of its
returns legs: subnormals, signed zeros, overflow to infinity, `0 * inf`, NaN values and bootstraps
- with ratio streams and tables made of the same constants.  Every comparison is
`same_bits_or_nan`: NaN in the same places, the same bits everywhere else; there is no tolerance.
As in tests/test_float_edges.py a difference here is a finding about the kernel or the build's
flags - a flushed denormal, a fused multiply-add, a division that is not IEEE-rounded, the sign of
a zero lost in a select - not about the test."""

import functools

import numpy as np
import pytest
import torch

import float_edges as fe
import vtrace_reference as ref

pytestmark = pytest.mark.gpu

F = np.float32
same = fe.same_bits_or_nan
T, B = fe.RETURNS_T, fe.RETURNS_B
# rho_bar, c_bar, pg_rho_bar: ordinary; huge, above one, subnormal; zeros of both signs
BARS = ((1.0, 1.0, None), (float(fe.FLT_MAX), 2.0, 2.0 ** -140), (0.0, -0.0, 0.0))
RATIO_EDGES = [1.0, 0.5, 2.0, 0.0, -0.0, fe.SUB_MIN, fe.SUB_140, fe.SUB_MAX, fe.NORM_MIN, fe.FLT_MAX,
               fe.P127, fe.PINF, fe.NINF, fe.NAN, -1.0, -fe.SUB_MIN]
LEGS = tuple(leg for leg in fe.RETURNS_LEGS)


@functools.lru_cache(maxsize=None)
def _ratio(leg):
  rng = np.random.RandomState(4200 + fe.RETURNS_LEGS.index(leg))
  return fe._pick(rng, RATIO_EDGES, (T, B))


@functools.lru_cache(maxsize=None)
def _want(leg, run, with_discount, bars):
  x = fe.returns_inputs(leg)
  gamma, lam = x['runs'][run]
  return ref.vtrace(x['reward'], x['done'], gamma, x['values'], _ratio(leg),
                    discount=x['discount'] if with_discount else None, bootstrap=x['bootstrap'], lam=lam,
                    rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2])


def test_the_sets_reach_the_edges():
  """From the reference alone: subnormal, negative-zero, infinite and NaN outputs all occur, and
  no NaN of the outputs comes from a ratio."""
  seen = dict(subnormal=0, negative_zero=0, inf=0, nan=0)
  for leg in LEGS:
    x = fe.returns_inputs(leg)
    for run in range(len(x['runs'])):
      for bars in BARS:
        want = _want(leg, run, True, bars)
        for k in ('vs', 'advantages'):
          seen['subnormal'] += int(fe.subnormal(want[k]).sum())
          seen['negative_zero'] += int(fe.negative_zero(want[k]).sum())
          seen['inf'] += int(np.isinf(want[k]).sum())
          seen['nan'] += int(np.isnan(want[k]).sum())
  assert all(n > 100 for n in seen.values()), seen
  # the signed-zero leg holds no NaN and no infinity but in its ratios: its outputs hold none
  x = fe.returns_inputs('signed_zero')
  assert np.isnan(_ratio('signed_zero')).any() and np.isinf(_ratio('signed_zero')).any()
  for run in range(len(x['runs'])):
    want = _want('signed_zero', run, True, BARS[0])
    assert not np.isnan(want['vs']).any() and not np.isnan(want['advantages']).any()


@pytest.mark.parametrize('leg', LEGS)
def test_ratio_mode_at_the_edges(leg):
  from campx_amd.returns import vtrace_returns
  x = fe.returns_inputs(leg)
  d = {k: torch.from_numpy(x[k]).cuda() for k in ('reward', 'done', 'discount', 'values', 'bootstrap')}
  ratio = torch.from_numpy(_ratio(leg)).cuda()
  for run, (gamma, lam) in enumerate(x['runs']):
    for with_discount in (True, False):
      for bars in BARS:
        got = vtrace_returns(d['reward'], d['done'], gamma, d['values'], ratio=ratio,
                             discount=d['discount'] if with_discount else None, bootstrap=d['bootstrap'],
                             lam=lam, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2])
        want = _want(leg, run, with_discount, bars)
        for k in ('vs', 'advantages'):
          assert same(got[k].cpu().numpy(), want[k]), (leg, gamma, lam, with_discount, bars, k)


TABLE_EDGES = [1.0, 0.5, 0.25, 3.0, 0.0, -0.0, fe.SUB_MIN, fe.SUB_140, fe.SUB_MAX, fe.NORM_MIN, 2.0 ** -120,
               fe.P120, fe.FLT_MAX, fe.PINF, fe.NAN, -0.5]


@pytest.mark.parametrize('Nt,Nb', [(7, 21), (2500, 2500)], ids=['lds', 'global'])
def test_table_mode_divides_as_ieee_does_at_the_edges(Nt, Nb):
  """Tables of edge constants: quotients that are subnormal, that round to the smallest normal,
  that overflow, 0 / 0, x / 0, inf / inf.  The kernel's division against numpy's float32 one."""
  from campx_amd.returns import vtrace_returns
  rng = np.random.RandomState(4300 + Nt)
  target = fe._pick(rng, TABLE_EDGES, (Nt, 5))
  behaviour = fe._pick(rng, TABLE_EDGES, (Nb, 5))
  states, actions = ref.ids(T, B, Nb)
  w0, bad = ref.table_ratio(target, behaviour, states, actions)
  assert bad == 0 and fe.subnormal(w0).sum() > 50 and np.isinf(w0).sum() > 50 and np.isnan(w0).sum() > 50
  x = fe.returns_inputs('signed_zero')
  d = {k: torch.from_numpy(x[k]).cuda() for k in ('reward', 'done', 'discount', 'values', 'bootstrap')}
  bars = BARS[0]                                      # (below one: a subnormal quotient is rho itself)
  want = ref.vtrace(x['reward'], x['done'], 0.5, x['values'], w0, discount=x['discount'],
                    bootstrap=x['bootstrap'], lam=0.5, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2])
  assert not np.isnan(want['vs']).any()               # (no ratio reaches the outputs as a NaN)
  for path in ((0, 1, 2) if Nt == 7 else (0, 2)):
    got = vtrace_returns(d['reward'], d['done'], 0.5, d['values'], target=torch.from_numpy(target).cuda(),
                         behaviour=torch.from_numpy(behaviour).cuda(), states=torch.from_numpy(states).cuda(),
                         actions=torch.from_numpy(actions).cuda(), discount=d['discount'],
                         bootstrap=d['bootstrap'], lam=0.5, rho_bar=bars[0], c_bar=bars[1],
                         pg_rho_bar=bars[2], path=path)
    for k in ('vs', 'advantages'):
      assert same(got[k].cpu().numpy(), want[k]), (path, k)
