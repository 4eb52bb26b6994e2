"""A population of rewards and gammas at the edges of float32 (csrc/k_plan.hip,
`campx::wide_population_solve`): ONE table of S = 5 states and P = 4 members whose rewards, gammas
and start values are drawn from tests/float_edges.py's constants - subnormals, signed zeros,
overflow, infinities, NaN - through both forms and both paths.

Two comparisons.  Against `value_iteration()` / `evaluate_policy()` of the member alone on the same
device: `array_equal` on the int32 views, NaN payloads included - the same operations on the same
chip.  Against tests/planning_reference.py member by member: `float_edges.same_bits_or_nan`, the
project's comparison wherever arithmetic may generate a NaN (its payload is 0xffc00000 on x86 and
0x7fc00000 on the GPU and no rule defines it) - every other bit the same.
"""

import functools
import types

import numpy as np
import pytest
import torch

import float_edges as fe
import planning_reference as plan_ref
import wide_table_reference as ref

pytestmark = pytest.mark.gpu

S, P = 5, 4
F = np.float32
COUNTS = (1, 2, 7)


@functools.lru_cache(maxsize=None)
def _inputs():
  """Member 0 walks down into the subnormals, 1 is about signed zeros, 2 overflows, 3 holds
  infinities and NaN; every member's rewards also hold a None."""
  g = ref.make_table(7000 + S, 4, 4, 2, 1, S, dcodes=True)
  rng = np.random.RandomState(31)
  pick = lambda values, shape: np.asarray(values, F)[rng.choice(len(values), size=shape)]
  tiny = [fe.SUB_MIN, -fe.SUB_MIN, fe.SUB_140, -fe.SUB_140, fe.SUB_MAX, -fe.SUB_MAX, fe.NORM_MIN, -fe.NORM_MIN]
  rewards = np.stack([pick(tiny + [fe.PZERO, fe.NZERO], (S, 5)),
                      pick([fe.PZERO, fe.NZERO, F(1), F(-1), fe.SUB_MIN, -fe.SUB_MIN], (S, 5)),
                      pick([fe.P120, -fe.P120, fe.P127, fe.FLT_MAX, -fe.FLT_MAX], (S, 5)),
                      pick(list(fe.EDGES), (S, 5))]).astype(F)
  rewards[:, 1, 2] = fe.NAN
  rewards[3, 0, :3] = [fe.PINF, fe.NINF, fe.NAN]
  values = np.stack([pick(tiny, (S,)), pick([fe.PZERO, fe.NZERO], (S,)),
                     pick([fe.FLT_MAX, -fe.FLT_MAX, fe.P127, -fe.P127], (S,)),
                     pick(list(fe.EDGES), (S,))]).astype(F)
  values[3, :3] = [fe.PINF, fe.NAN, fe.NINF]
  gammas = np.array([0.5, -0.5, 2.0, 0.0], F)
  weights = np.stack([fe.edge_policy(S), fe.ordinary_policy(S), fe.ordinary_policy(S), fe.edge_policy(S)])
  return g, rewards, values, gammas, weights


def _game(g):
  from campx_amd import wide
  return wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), 1, 'cuda', g)


def _cuda(x):
  return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
  x = x.detach().cpu().numpy()
  return x.view(np.int32) if x.dtype == np.float32 else x


def test_the_inputs_reach_the_edges():
  g, rewards, values, gammas, weights = _inputs()
  assert fe.host_keeps_subnormals()
  assert fe.subnormal(rewards[0]).any() and fe.subnormal(values[0]).any()
  assert fe.negative_zero(rewards[1]).any() and fe.negative_zero(values[1]).any()
  assert np.isinf(rewards[3]).any() and np.isnan(rewards).any() and np.isnan(values[3]).any()
  with np.errstate(all='ignore'):
    want = [plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, gammas[m], 7, values=values[m],
                            reward_override=rewards[m]) for m in range(P)]
  assert fe.subnormal(want[0]['values']).any()
  assert np.isinf(want[2]['values']).any() or np.isnan(want[2]['values']).any()
  assert np.isinf(want[3]['q']).any()
  with np.errstate(all='ignore'):                # (the greedy maximum sheds the NaNs within a few sweeps)
    first = plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, gammas[3], 1, values=values[3],
                            reward_override=rewards[3])
  assert np.isnan(first['q']).any() and np.isnan(first['values']).any() and np.isnan(first['residual']).any()


@pytest.mark.parametrize('path', [1, 2])
@pytest.mark.parametrize('form', ['greedy', 'policy'])
def test_the_edges_member_by_member(form, path):
  g, rewards, values, gammas, weights = _inputs()
  f = _game(g)
  f.validate_actions = False                     # (the edge rows hold bad ones: counted elsewhere)
  r, v, w = _cuda(rewards), _cuda(values), _cuda(weights)
  keys = ('values', 'q', 'residual') + (('greedy',) if form == 'greedy' else ())
  for n in COUNTS:
    for gamma in (_cuda(gammas), 0.5):
      if form == 'greedy':
        res = f.value_iteration_population(gamma, n, rewards=r, values=v, want_q=True, path=path)
      else:
        res = f.evaluate_population(w, gamma, n, rewards=r, values=v, want_q=True, path=path)
      res = {k: res[k].clone() for k in keys}
      for m in range(P):
        gm = float(gammas[m]) if torch.is_tensor(gamma) else gamma
        if form == 'greedy':
          alone = f.value_iteration(gm, n, values=v[m], reward=r[m], path=path)
        else:
          alone = f.evaluate_policy(w[m], gm, n, values=v[m], reward=r[m], path=path)
        with np.errstate(all='ignore'):
          want = plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, F(gm), n,
                                 policy=None if form == 'greedy' else weights[m], values=values[m],
                                 reward_override=rewards[m])
        for k in keys:
          got = res[k][:, m] if k == 'residual' else res[k][m]
          assert np.array_equal(_bits(got), _bits(alone[k])), (form, path, n, m, k, 'the member alone')
          if k == 'greedy':
            assert np.array_equal(got.cpu().numpy(), want[k]), (form, path, n, m, k)
          else:
            assert fe.same_bits_or_nan(got.cpu().numpy(), want[k]), (form, path, n, m, k)
