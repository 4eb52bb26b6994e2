"""`evaluate_population()` (csrc/k_plan.hip) at the edges of float32, in the manner of
tests/test_float_edges.py: one small table (S = 5, P = 4) whose weights, rewards, gammas and start
values hold subnormals, signed zeros, values that overflow, infinities and NaN, on both paths,
against tests/planning_reference.py run member by member.  Every comparison is
`float_edges.same_bits_or_nan`: NaN in the same places, the same bits everywhere else - the payload
of a generated NaN is the one thing no rule defines.  (Four members are one to a workgroup on a
chip of 256 compute units; tests/test_population_planning.py packs several.)"""

import types

import numpy as np
import pytest
import torch

import float_edges as fe
import planning_reference as plan_ref
import wide_table_reference as table_ref

pytestmark = pytest.mark.gpu

F = np.float32
S, P = 5, 4
COUNTS = (1, 2, 7)
same = fe.same_bits_or_nan

# member m's weights: the edge rows of tests/float_edges.py, shifted by m so that every state
# meets every kind; member 3 also holds a row with a NaN and a row of zeros
KINDS = ('subnormal', 'one_max', 'two_max', 'negative_zero', 'tiny')


def _weights():
  w = np.stack([np.array([fe.EDGE_ROWS[KINDS[(s + m) % 5]] for s in range(S)], F) for m in range(P)])
  w[3, 1] = [1.0, fe.NAN, 1.0, 1.0, 1.0]
  w[3, 4] = 0
  w[2] = np.random.RandomState(7).uniform(0.5, 2.0, size=(S, 5)).astype(F)     # an ordinary member among them
  w[2, 0, 2] = fe.NZERO
  return w


LEGS = {
    # rewards at and below the smallest normal; the gammas keep products subnormal or flush them to a signed zero
    'underflow': dict(
        reward=[fe.SUB_MIN, -fe.SUB_MIN, fe.SUB_140, -fe.SUB_140, fe.SUB_MAX, -fe.SUB_MAX, fe.NORM_MIN,
                -fe.NORM_MIN, fe.PZERO, fe.NZERO, fe.NAN, F(2.0 ** -120), F(-2.0 ** -120)],
        gammas=[0.5, fe.SUB_140, -0.0, 1.0],
        values=[fe.SUB_MIN, -fe.SUB_MIN, fe.SUB_MAX, -fe.SUB_MAX, fe.NORM_MIN, fe.PZERO, fe.NZERO]),
    # rewards whose sums pass FLT_MAX; inf - inf and 0 * inf on the way; a gamma of inf and one of NaN
    'overflow': dict(
        reward=[fe.P120, -fe.P120, fe.P127, -fe.P127, fe.FLT_MAX, -fe.FLT_MAX, fe.PINF, fe.NINF, fe.NAN,
                fe.PZERO, fe.NZERO, F(1.0)],
        gammas=[1.0, 2.0, fe.PINF, fe.NAN],
        values=[fe.FLT_MAX, -fe.FLT_MAX, fe.P127, fe.PINF, fe.NINF, fe.NAN, fe.PZERO, F(1.0)]),
}


def _inputs(leg):
  rng = np.random.RandomState(40 + len(leg))
  x = LEGS[leg]
  pick = lambda values, shape: np.asarray(values, F)[rng.choice(len(values), size=shape)]
  reward, values = pick(x['reward'], (S, 5)), pick(x['values'], (P, S))
  reward.reshape(-1)[:len(x['reward'])] = np.asarray(x['reward'], F)           # every edge is there
  values.reshape(-1)[:len(x['values'])] = np.asarray(x['values'], F)
  return reward, np.asarray(x['gammas'], F), values


def _wide(table):
  from campx_amd import wide
  f = wide.WideGame(types.SimpleNamespace(rows=table.rows, cols=table.cols), 1, 'cuda', table)
  assert f.n_states == table.n_states == S
  return f


def test_the_inputs_hold_the_edges():
  w = _weights()
  assert fe.subnormal(w).any() and fe.negative_zero(w).any() and (w == fe.FLT_MAX).any() and np.isnan(w).any()
  for leg in LEGS:
    reward, gammas, values = _inputs(leg)
    pool = np.concatenate([reward.ravel(), gammas, values.ravel()])
    assert fe.negative_zero(pool).any() and np.isnan(pool).any(), leg
    assert (fe.subnormal(pool).any() if leg == 'underflow' else np.isinf(pool).any()), leg


@pytest.mark.parametrize('leg', sorted(LEGS))
def test_population_sweeps_at_the_edges_on_both_paths(leg):
  g = table_ref.make_table(7000 + S, 4, 4, 2, 1, S, dcodes=True)
  f = _wide(g)
  f.validate_actions = 'sync'
  w = _weights()
  reward, gammas, values = _inputs(leg)
  dev = lambda a: torch.from_numpy(a).cuda()
  policies, reward_d, gammas_d, values_d = dev(w), dev(reward), dev(gammas), dev(values)
  met = dict(nan=False, inf=False, sub=False)
  for n in COUNTS:
    each = [plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, gammas[m], n, policy=w[m],
                            values=values[m], reward_override=reward) for m in range(P)]
    want = dict(values=np.stack([e['values'] for e in each]), q=np.stack([e['q'] for e in each]),
                residual=np.stack([e['residual'] for e in each], axis=1))
    n_bad = sum(e['bad_rows'] for e in each)
    assert n_bad == 4                             # the two_max rows of members 0 and 1, member 3's NaN row and zero row
    for path in (1, 2):
      out = f.population_sweep_buffers(P, n, want_q=True)
      with pytest.raises(ValueError, match='^{} rows of the policies given to evaluate_population'.format(n_bad)):
        f.evaluate_population(policies, gammas_d, n, values=values_d, reward=reward_d, want_q=True, out=out,
                              path=path)
      for k in ('values', 'q', 'residual'):
        assert same(out[k].cpu().numpy(), want[k]), (leg, n, path, k)
    pool = np.concatenate([want['values'].ravel(), want['q'].ravel(), want['residual'].ravel()])
    met['nan'] |= bool(np.isnan(pool).any())
    met['inf'] |= bool(np.isinf(pool).any())
    met['sub'] |= bool(fe.subnormal(pool).any())
  # the results reach the edges too: what is compared above is not all ordinary numbers
  assert met['sub'] if leg == 'underflow' else (met['nan'] and met['inf']), met
  assert same(values_d.cpu().numpy(), values)           # the values given are left as they are
  f.check_actions()
