"""`campx_amd.returns.discounted_returns()` on the GPU (csrc/k_returns.hip, `campx::returns`)
against tests/returns_reference.py, the rule restated in numpy float32: every comparison is of
bits.  Shapes: every T of {1, 7, 8, 9, 100} - both sides of the kernel's 8-frame chunk, one frame,
many chunks - at B = 257, and every B of {1, 63, 64, 65, 257, 4 099} - both sides of a wave, more
than one 256-lane block, sixteen blocks and a tail - at T = 9.  Inputs dense and as padded views
(the streams of `rollout_trace_buffers()`, every other tensor with a pitch of its own); every
combination of discount / values / bootstrap present or None; lam 1.0, 0.95 and 0.0.  The inputs
are ordinary numbers; tests/test_float_edges.py has the subnormals, signed zeros, overflow and NaN."""

import functools
import itertools

import numpy as np
import pytest
import torch

import returns_reference as ref

pytestmark = pytest.mark.gpu

GAMMA = 0.99
LAMS = (1.0, 0.95, 0.0)
CASES = [(T, 257) for T in (1, 7, 8, 9, 100)] + [(9, B) for B in (1, 63, 64, 65, 4099)]
COMBOS = list(itertools.product((True, False), repeat=3))     # discount, values, bootstrap


@functools.lru_cache(maxsize=None)
def _inputs(T, B):
  return ref.inputs(T, B)


@functools.lru_cache(maxsize=None)
def _want(T, B, with_discount, with_values, with_bootstrap, lam):
  x = _inputs(T, B)
  return ref.returns(x['reward'], x['done'], GAMMA, x['discount'] if with_discount else None,
                     x['values'] if with_values else None,
                     x['bootstrap'] if with_bootstrap else None, lam)


@functools.lru_cache(maxsize=None)
def _game(B):
  from campx_amd.games import boat_race
  game = boat_race.build(B, 'cuda')
  game.use_state_table()
  game.its_showtime()
  return game


def _padded(x, pitch):
  """A [T, B] view with rows `pitch` apart, filled from the numpy array `x`."""
  T, B = x.shape
  src = torch.from_numpy(x)
  view = torch.full((T, pitch), 7, dtype=src.dtype, device='cuda')[:, :B]
  view.copy_(src)
  return view


def _device_inputs(T, B, layout):
  x = _inputs(T, B)
  if layout == 'dense':
    return {k: torch.from_numpy(x[k]).cuda() for k in ('reward', 'done', 'discount', 'values', 'bootstrap')}
  bufs = _game(B).rollout_trace_buffers(T)         # reward / discount / done: rows padded to 16
  up = (B + 15) // 16 * 16
  assert bufs['reward'] is not None and (T == 1 or bufs['reward'].stride(0) == up)
  d = {}
  for k in ('reward', 'done', 'discount'):
    bufs[k].copy_(torch.from_numpy(x[k]))
    d[k] = bufs[k]
  d['values'] = _padded(x['values'], B + 7)
  d['bootstrap'] = torch.from_numpy(x['bootstrap']).cuda()
  return d


def _outputs(T, B, layout):
  if layout == 'dense':
    return None
  return {'returns': torch.zeros((T, B + 3), dtype=torch.float32, device='cuda')[:, :B],
          'advantages': torch.zeros((T, up16(B) + 16), dtype=torch.float32, device='cuda')[:, :B]}


def up16(B):
  return (B + 15) // 16 * 16


@pytest.mark.parametrize('layout', ['dense', 'padded'])
@pytest.mark.parametrize('T,B', CASES, ids=['T{}-B{}'.format(T, B) for T, B in CASES])
def test_returns_and_advantages_bit_for_bit(T, B, layout):
  from campx_amd.returns import discounted_returns
  d = _device_inputs(T, B, layout)
  if layout == 'padded' and T > 1:
    pitches = {d['reward'].stride(0), d['values'].stride(0), B + 3, up16(B) + 16}
    assert len(pitches) == 4 and d['done'].stride(0) == d['reward'].stride(0)
  n = 0
  for with_discount, with_values, with_bootstrap in COMBOS:
    for lam in (LAMS if with_values else (1.0,)):
      out = _outputs(T, B, layout)
      if out is not None and not with_values:
        del out['advantages']
      got = discounted_returns(d['reward'], d['done'], GAMMA,
                               discount=d['discount'] if with_discount else None,
                               values=d['values'] if with_values else None,
                               bootstrap=d['bootstrap'] if with_bootstrap else None, lam=lam, out=out)
      G, A = _want(T, B, with_discount, with_values, with_bootstrap, lam)
      what = (with_discount, with_values, with_bootstrap, lam)
      assert set(got) == ({'returns', 'advantages'} if with_values else {'returns'}), what
      assert got['returns'].shape == (T, B) and got['returns'].dtype == torch.float32
      if out is not None:
        assert got['returns'].data_ptr() == out['returns'].data_ptr()
      g = got['returns'].cpu().numpy()
      assert not np.isnan(g).any(), what            # NaN rewards never reach the outputs
      assert ref.same_bits(g, G), what
      if with_values:
        a = got['advantages'].cpu().numpy()
        assert not np.isnan(a).any(), what
        assert ref.same_bits(a, A), what
      n += 1
  assert n == 4 * 3 + 4


def test_the_inputs_hold_what_the_docstring_says():
  """NaN rewards and every forced column are there (so the comparisons above meet them); and the
  reference itself stops at a `done`: the all-done column's return is its reward."""
  x = _inputs(100, 257)
  assert np.isnan(x['reward']).any() and set(np.unique(x['discount'])) == {0.0, 0.5, 1.0}
  f = x['forced']
  assert x['done'][:, f['all']].all() and not x['done'][:, f['never']].any()
  assert x['done'][:, f['first']].sum() == 1 and x['done'][0, f['first']] == 1
  assert x['done'][:, f['last']].sum() == 1 and x['done'][99, f['last']] == 1
  G, A = _want(100, 257, True, True, True, 0.95)
  r = np.where(np.isnan(x['reward']), np.float32(0), x['reward'])
  assert ref.same_bits(G[:, f['all']], r[:, f['all']])
  assert ref.same_bits(A[:, f['all']], r[:, f['all']] - x['values'][:, f['all']])
  # the bootstrap reaches frame 0 of the never-done column and no frame of the last-done one
  G0, _ = _want(100, 257, True, True, False, 0.95)
  assert ref.same_bits(G[:, f['last']], G0[:, f['last']])
  if x['discount'][99, f['never']] != 0:
    assert not ref.same_bits(G[-1:, f['never']], G0[-1:, f['never']])


def test_out_and_graph_capture():
  from campx_amd.returns import discounted_returns
  T, B = 9, 257
  d = _device_inputs(T, B, 'dense')
  out = {'returns': torch.empty((T, B), dtype=torch.float32, device='cuda'),
         'advantages': torch.empty((T, B), dtype=torch.float32, device='cuda')}
  call = lambda: discounted_returns(d['reward'], d['done'], GAMMA, discount=d['discount'],
                                    values=d['values'], bootstrap=d['bootstrap'], lam=0.95, out=out)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    call()                                    # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    call()
  for seed in (1, 2):
    x = ref.inputs(T, B, seed=seed)
    for k in ('reward', 'done', 'discount', 'values', 'bootstrap'):
      d[k].copy_(torch.from_numpy(x[k]))
    out['returns'].zero_()
    out['advantages'].zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = discounted_returns(d['reward'], d['done'], GAMMA, discount=d['discount'],
                               values=d['values'], bootstrap=d['bootstrap'], lam=0.95)
    G, A = ref.returns(x['reward'], x['done'], GAMMA, x['discount'], x['values'], x['bootstrap'], 0.95)
    for k, want in (('returns', G), ('advantages', A)):
      assert ref.same_bits(out[k].cpu().numpy(), want), (seed, k)
      assert ref.same_bits(eager[k].cpu().numpy(), want), (seed, k)


def test_undiscounted_returns_are_the_engines_own_episode_return():
  """gamma = 1 and no discount: for an environment whose rollout holds no `done`, returns[0] is
  the sum of its rewards - what wide_policy_update_kernel accumulates, forwards, into `ret`.  The
  boat race's rewards are small integers, so both summation orders are exact."""
  from campx_amd.returns import discounted_returns
  T, B = 100, 4099
  game = _game(B)
  f = game.fused
  policy = torch.ones((f.n_states, 5), dtype=torch.float32, device='cuda')
  out = game.rollout_policy(policy, T, seed=5, reset_first=True)
  reward = out['reward']
  assert not torch.isnan(reward).any() and torch.equal(reward, reward.round())
  assert float(reward.abs().max()) * T < 2 ** 24
  got = discounted_returns(reward, out['done'], 1.0)
  quiet = ~out['done'].bool().any(dim=0)
  assert int(quiet.sum()) > B // 2
  assert torch.equal(got['returns'][0][quiet].view(torch.int32), f.ret[quiet].view(torch.int32))
  assert len(set(f.ret[quiet].tolist())) > 3        # (and the returns are not all alike)
  f.check_actions()


def test_argument_errors_raise_before_any_launch():
  from campx_amd.returns import discounted_returns
  T, B = 9, 65
  d = _device_inputs(T, B, 'dense')
  out = {'returns': torch.full((T, B), 123.0, device='cuda'),
         'advantages': torch.full((T, B), 123.0, device='cuda')}
  good = dict(reward=d['reward'], done=d['done'], gamma=GAMMA, discount=d['discount'],
              values=d['values'], bootstrap=d['bootstrap'], lam=0.95, out=out)
  sideways = torch.zeros((B, T), dtype=torch.float32, device='cuda').t()      # [T, B], stride(1) = T
  assert sideways.shape == (T, B) and sideways.stride(1) != 1
  bad = {
      'reward dtype': dict(reward=d['reward'].double()),
      'reward not a tensor': dict(reward=d['reward'].cpu().numpy()),
      'reward rank': dict(reward=d['reward'][0]),
      'reward device': dict(reward=d['reward'].cpu()),
      'reward stride(1)': dict(reward=sideways),
      'done dtype': dict(done=d['done'].bool()),
      'done shape': dict(done=d['done'][:, :B - 1]),
      'done device': dict(done=d['done'].cpu()),
      'discount dtype': dict(discount=d['discount'].half()),
      'discount shape': dict(discount=d['discount'][:T - 1]),
      'discount stride(1)': dict(discount=sideways),
      'values shape': dict(values=d['values'][:, :B - 1]),
      'values dtype': dict(values=d['values'].double()),
      'values device': dict(values=d['values'].cpu()),
      'bootstrap shape': dict(bootstrap=d['bootstrap'][:B - 1]),
      'bootstrap dtype': dict(bootstrap=d['bootstrap'].double()),
      'gamma nan': dict(gamma=float('nan')),
      'gamma inf': dict(gamma=float('inf')),
      'gamma type': dict(gamma='0.99'),
      'lam inf': dict(lam=float('-inf')),
      'lam nan': dict(lam=float('nan')),
      'out not a dict': dict(out=out['returns']),
      'out without advantages': dict(out={'returns': out['returns']}),
      'out shape': dict(out={'returns': out['returns'][:T - 1], 'advantages': out['advantages']}),
      'out dtype': dict(out={'returns': out['returns'].double(), 'advantages': out['advantages']}),
  }
  for what, change in bad.items():
    with pytest.raises(ValueError):
      discounted_returns(**dict(good, **change))
      pytest.fail('no ValueError for: ' + what)
  torch.cuda.synchronize()
  assert bool((out['returns'] == 123.0).all()) and bool((out['advantages'] == 123.0).all())
  got = discounted_returns(**good)                   # and the good call goes through
  G, A = ref.returns(*(_inputs(T, B)[k] for k in ('reward', 'done')), GAMMA, _inputs(T, B)['discount'],
                     _inputs(T, B)['values'], _inputs(T, B)['bootstrap'], 0.95)
  assert ref.same_bits(got['returns'].cpu().numpy(), G) and ref.same_bits(got['advantages'].cpu().numpy(), A)
