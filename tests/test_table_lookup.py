"""`campx_amd.returns.table_lookup()` on the GPU (csrc/k_sums.hip, `campx::table_lookup`): the
forward bit for bit `table[states.long(), actions.long()]` (uint32 views), 0.0 at a bad index; the
backward bit for bit tests/state_sums_reference.py applied to the incoming gradient, and within
the fixed-point rule's derived bound of torch's own float64 gradient of the same loss.  Same
shapes and layouts as tests/test_state_sums.py; tables on both sides of the LDS staging."""

import functools

import numpy as np
import pytest
import torch

import state_sums_reference as ref

pytestmark = pytest.mark.gpu

CASES = [(T, 257) for T in (1, 7, 8, 9, 100)] + [(9, B) for B in (1, 63, 64, 65, 4099)]
TABLES = (1, 8, 1940, 70000)
F = 24


@functools.lru_cache(maxsize=None)
def _inputs(T, B, S, A, dirty):
  return ref.inputs(T, B, S, A, 1, dirty=dirty)


@functools.lru_cache(maxsize=None)
def _table(S, A):
  return np.random.RandomState(S + A).uniform(-2, 2, size=(S, A)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _game(B):
  from campx_amd.games import boat_race
  game = boat_race.build(B, 'cuda')
  game.use_state_table()
  game.its_showtime()
  return game


def _device(x, layout):
  T, B = x['states'].shape
  if layout == 'dense':
    return torch.from_numpy(x['states']).cuda(), torch.from_numpy(x['actions']).cuda()
  bufs = _game(B).rollout_policy_buffers(T)        # rows padded to a multiple of 16
  bufs['states'].copy_(torch.from_numpy(x['states']))
  bufs['actions'].copy_(torch.from_numpy(x['actions']))
  return bufs['states'], bufs['actions']


def _same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(
      a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('layout', ['dense', 'padded'])
@pytest.mark.parametrize('T,B', CASES, ids=['T{}-B{}'.format(T, B) for T, B in CASES])
def test_forward_bit_for_bit(T, B, layout):
  from campx_amd.returns import table_lookup
  for S in TABLES:
    for A in (1, 5):
      table = torch.from_numpy(_table(S, A)).cuda()
      if A == 1:
        table = table[:, 0].contiguous()
      # in range: the advanced index itself
      x = _inputs(T, B, S, A, False)
      states, actions = _device(x, layout)
      got = table_lookup(table, states, actions if A > 1 else None)
      want = table[states.long(), actions.long()] if A > 1 else table[states.long()]
      assert _same_bits(got, want), (S, A)
      # with bad indices: 0.0 there, counted
      x = _inputs(T, B, S, A, True)
      states, actions = _device(x, layout)
      bad = torch.full((1,), 5, dtype=torch.int64, device='cuda')
      got = table_lookup(table, states, actions if A > 1 else None, bad_count=bad)
      want, n_bad = ref.lookup(_table(S, A) if A > 1 else _table(S, A)[:, 0], x['states'],
                               x['actions'] if A > 1 else None)
      assert _same_bits(got, torch.from_numpy(want).cuda()), (S, A, 'dirty')
      assert int(bad) == 5 + n_bad and (n_bad > 0 or T * B < 257)
      if n_bad:
        s = x['states'].astype(np.int64)
        assert bool((got[torch.from_numpy((s < 0) | (s >= S)).cuda()] == 0).all())


@pytest.mark.parametrize('T,B', [(9, 257), (100, 257), (9, 4099)])
def test_backward_is_the_fixed_point_sum_of_the_gradient(T, B):
  from campx_amd.returns import table_lookup
  for S in (8, 1940):
    for A in (1, 5):
      x = _inputs(T, B, S, A, True)
      states, actions = _device(x, 'dense')
      acts = actions if A > 1 else None
      host = _table(S, A) if A > 1 else _table(S, A)[:, 0]
      table = torch.from_numpy(host).cuda().requires_grad_()
      w_host = np.random.RandomState(T + B).uniform(-2, 2, size=(T, B)).astype(np.float32)
      w = torch.from_numpy(w_host).cuda()
      (table_lookup(table, states, acts) * w).sum().backward()       # grad_out is w, exactly
      sums = ref.state_sums(x['states'], x['actions'] if A > 1 else None, [w_host], S, A, frac_bits=F)
      assert sums['skipped'] > 0 and sums['clamped'] == 0
      want = (sums['raw'][1].astype(np.float64) * 2.0 ** -F).astype(np.float32).reshape(host.shape)
      assert table.grad.shape == table.shape
      assert _same_bits(table.grad, torch.from_numpy(want).cuda()), (S, A)
      # and against torch's own gradient, in float64, of the same loss (a bad index: 0.0, no gradient)
      s = torch.from_numpy(x['states']).cuda().long()
      a = torch.from_numpy(x['actions']).cuda().long()
      good = (s >= 0) & (s < S)
      if A > 1:
        good = good & (a >= 0) & (a < A)
      t64 = torch.from_numpy(host).cuda().double().requires_grad_()
      picked = t64[s.clamp(0, S - 1), a.clamp(0, A - 1)] if A > 1 else t64[s.clamp(0, S - 1)]
      (picked * w.double() * good).sum().backward()
      count = torch.from_numpy(sums['raw'][0].reshape(host.shape)).cuda().double()
      # per bin: n_bin half-quanta of the fixed point, then one float32 rounding of that sum
      half = count * 2.0 ** -(F + 1)
      bound = half + (t64.grad.abs() + half) * 2.0 ** -24
      assert bool(((table.grad.double() - t64.grad).abs() <= bound).all()), (S, A)
      assert float(t64.grad.abs().max()) > 0.1


def test_a_broadcast_gradient_and_no_gradient():
  from campx_amd.returns import table_lookup
  T, B, S, A = 9, 257, 8, 5
  x = _inputs(T, B, S, A, False)
  states, actions = _device(x, 'padded')
  table = torch.from_numpy(_table(S, A)).cuda().requires_grad_()
  table_lookup(table, states, actions).sum().backward()         # grad_out is an expanded scalar
  count = ref.state_sums(x['states'], x['actions'], (), S, A)['raw'][0].reshape(S, A)
  assert torch.equal(table.grad, torch.from_numpy(count.astype(np.float32)).cuda())
  assert not table_lookup(table.detach(), states, actions).requires_grad


def test_argument_errors_raise_before_any_launch():
  from campx_amd.returns import table_lookup
  T, B, S, A = 9, 65, 8, 5
  x = _inputs(T, B, S, A, False)
  states, actions = _device(x, 'dense')
  table = torch.from_numpy(_table(S, A)).cuda()
  bad_count = torch.full((1,), 123, dtype=torch.int64, device='cuda')
  good = dict(table=table, states=states, actions=actions, bad_count=bad_count)
  sideways = lambda dtype: torch.zeros((B, T), dtype=dtype, device='cuda').t()
  narrow = lambda t: torch.as_strided(t, (T, B), (B - 1, 1))
  bad = {
      'table dtype': dict(table=table.double()),
      'table rank': dict(table=table[:, 0].contiguous()),
      'table rank without actions': dict(actions=None),
      'table on the CPU': dict(table=table.cpu()),
      'table not contiguous': dict(table=table.t().contiguous().t()),
      'table too wide': dict(table=torch.zeros((S, 129), device='cuda')),
      'table not a tensor': dict(table=_table(S, A)),
      'states dtype': dict(states=states.long()),
      'states on the CPU': dict(states=states.cpu()),
      'states stride(1)': dict(states=sideways(torch.int32)),
      'states pitch': dict(states=narrow(states)),
      'actions dtype': dict(actions=actions.long()),
      'actions shape': dict(actions=actions[:T - 1]),
      'actions on the CPU': dict(actions=actions.cpu()),
      'actions stride(1)': dict(actions=sideways(torch.int8)),
      'actions pitch': dict(actions=narrow(actions)),
      'bad_count dtype': dict(bad_count=bad_count.int()),
      'bad_count on the CPU': dict(bad_count=bad_count.cpu()),
      'bad_count size': dict(bad_count=torch.zeros((2,), dtype=torch.int64, device='cuda')),
  }
  for what, change in bad.items():
    with pytest.raises(ValueError):
      table_lookup(**dict(good, **change))
      pytest.fail('no ValueError for: ' + what)
  torch.cuda.synchronize()
  assert int(bad_count) == 123
  got = table_lookup(**good)
  assert _same_bits(got, table[states.long(), actions.long()]) and int(bad_count) == 123


def test_opcheck():
  T, B, S, A = 9, 65, 8, 5
  x = _inputs(T, B, S, A, True)
  states, actions = _device(x, 'dense')
  table = torch.from_numpy(_table(S, A)).cuda()
  out = torch.zeros((T, B), dtype=torch.float32, device='cuda')
  bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
  torch.library.opcheck(torch.ops.campx.table_lookup.default, (table, states, actions, out, bad))
