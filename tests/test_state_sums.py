"""`campx_amd.returns.sum_by_state()` on the GPU (csrc/k_sums.hip, `campx::state_sums`) against
tests/state_sums_reference.py, the rule restated in numpy: every comparison is `array_equal` on the
int64 accumulators and the two counters.  Shapes: every T of {1, 7, 8, 9, 100} - both sides of the
kernel's 8-frame chunk, one frame, several slices of T - at B = 257, and every B of {1, 63, 64,
65, 257, 4 099} - both sides of a wave, more than one 256-lane block, sixteen blocks and a tail -
at T = 9; dense, and as padded views (the states and actions of a boat race's
`rollout_policy_buffers()`, every value stream with a pitch of its own).  Tables S of {1, 8,
1 940, 70 000} x A of {1 (no action stream), 5} x K of {0, 1, 4}; each with the LDS path forced
where the accumulators fit, the global path forced, and the library's choice."""

import functools

import numpy as np
import pytest
import torch

import state_sums_reference as ref
from campx_amd import _hip

pytestmark = pytest.mark.gpu

CASES = [(T, 257) for T in (1, 7, 8, 9, 100)] + [(9, B) for B in (1, 63, 64, 65, 4099)]
TABLES = (1, 8, 1940, 70000)
F = 24


@functools.lru_cache(maxsize=None)
def _inputs(T, B, S, A, dirty):
  return ref.inputs(T, B, S, A, 4, dirty=dirty)


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


def _device(x, layout):
  """The streams of `ref.inputs()` on the device: (states, actions, [values])."""
  T, B = x['states'].shape
  if layout == 'dense':
    return (torch.from_numpy(x['states']).cuda(), torch.from_numpy(x['actions']).cuda(),
            [torch.from_numpy(v).cuda() for v in x['values']])
  bufs = _game(B).rollout_policy_buffers(T)        # rows padded to a multiple of 16
  up = (B + 15) // 16 * 16
  assert T == 1 or (bufs['states'].stride(0) == up and bufs['actions'].stride(0) == up)
  bufs['states'].copy_(torch.from_numpy(x['states']))
  bufs['actions'].copy_(torch.from_numpy(x['actions']))
  values = [_padded(v, up + 16 + 3 * k) for k, v in enumerate(x['values'])]
  assert T == 1 or len({v.stride(0) for v in values} | {up}) == len(values) + 1
  return bufs['states'], bufs['actions'], values


def _fits_lds(S, A, K):
  return S * A * (K + 1) * 8 <= _hip.SUMS_LDS_BUDGET


def _check(got, want, shape, what):
  raw = torch.from_numpy(want['raw'].reshape(shape)).cuda()
  assert got['raw'].shape == shape and got['raw'].dtype == torch.int64, what
  assert torch.equal(got['raw'], raw), what
  assert torch.equal(got['count'], raw[0]), what
  assert (int(got['skipped']), int(got['clamped'])) == (want['skipped'], want['clamped']), what
  assert got['skipped'].dim() == 0 and got['skipped'].dtype == torch.int64 and got['skipped'].is_cuda
  assert got['sums'].dtype == torch.float64 and got['sums'].shape == (shape[0] - 1,) + shape[1:]
  assert torch.equal(got['sums'], raw[1:].double() * 2.0 ** -F), what


@pytest.mark.parametrize('dirty', [False, True], ids=['clean', 'dirty'])
@pytest.mark.parametrize('layout', ['dense', 'padded'])
@pytest.mark.parametrize('T,B', CASES, ids=['T{}-B{}'.format(T, B) for T, B in CASES])
def test_sums_bit_for_bit_on_every_path(T, B, layout, dirty):
  from campx_amd.returns import sum_by_state
  n = 0
  for S in TABLES:
    for A in (1, 5):
      x = _inputs(T, B, S, A, dirty)
      states, actions, values = _device(x, layout)
      for K in (0, 1, 4):
        want = ref.state_sums(x['states'], x['actions'] if A > 1 else None, x['values'][:K], S, A,
                              frac_bits=F)
        if dirty and T * B >= 257:
          assert want['skipped'] > 0 and (K == 0 or want['clamped'] > 0)
        else:
          assert dirty or (want['skipped'] == 0 and want['clamped'] == 0)
        shape = (K + 1, S) + ((A,) if A > 1 else ())
        for path in (1, 2, 0):
          if path == 1 and not _fits_lds(S, A, K):
            continue
          got = sum_by_state(states, actions if A > 1 else None, tuple(values[:K]), n_states=S,
                             n_actions=A, frac_bits=F, path=path)
          _check(got, want, shape, (S, A, K, path))
          n += 1
  assert n == 4 * 2 * 3 * 2 + sum(_fits_lds(S, A, K) for S in TABLES for A in (1, 5) for K in (0, 1, 4))


def test_the_inputs_hold_what_the_docstring_says():
  x = _inputs(100, 257, 8, 5, True)
  v = x['values'][1]
  assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
  assert (np.abs(v[np.isfinite(v)]) > 1e30).any()
  assert (x['states'] < 0).any() and (x['states'] >= 8).any()
  assert (x['actions'] == 5).any() and (x['actions'] == -1).any()
  c = _inputs(100, 257, 8, 5, False)
  assert set(np.unique(c['values'][0])) == {-1.0, -0.25, 0.0, 0.5, 1.0, 3.0}
  assert np.abs(c['values'][1]).max() <= 2 and len(np.unique(c['values'][1])) > 1000
  # the three paths are really three: the plan takes LDS for the small tables, global for the large
  out = (__import__('ctypes').c_int64 * 8)()
  assert _hip.lib.campx_state_sums_plan(8, 5, 1, 257, 100, F, 0, out) == 0 and out[0] == 1 and out[1] > 1
  assert _hip.lib.campx_state_sums_plan(70000, 5, 1, 257, 100, F, 0, out) == 0 and out[0] == 2


def test_worst_contention_every_frame_in_one_bin():
  from campx_amd.returns import sum_by_state
  T, B = 100, 4099
  x = _inputs(T, B, 8, 5, False)
  states = torch.zeros((T, B), dtype=torch.int32, device='cuda')
  actions = torch.zeros((T, B), dtype=torch.int8, device='cuda')
  values = [torch.from_numpy(x['values'][0]).cuda(), torch.from_numpy(x['values'][1]).cuda()]
  zeros = np.zeros((T, B), dtype=np.int32)
  want = ref.state_sums(zeros, zeros.astype(np.int8), x['values'][:2], 8, 5, frac_bits=F)
  assert want['raw'][0][0] == 409900 and want['raw'][0][1:].sum() == 0
  # stream 0 holds multiples of 0.25: its sum is exact, and so is the fixed-point one
  assert want['raw'][1][0] == int(round(float(x['values'][0].astype(np.float64).sum()) * 2 ** F))
  for path in (1, 2, 0):
    got = sum_by_state(states, actions, tuple(values), n_states=8, n_actions=5, frac_bits=F, path=path)
    _check(got, want, (3, 8, 5), path)
    assert int(got['count'][0, 0]) == 409900
    assert float(got['sums'][0, 0, 0]) == float(x['values'][0].astype(np.float64).sum())


def test_accumulate_adds_and_plain_calls_overwrite():
  from campx_amd.returns import sum_by_state
  T, B, S, A, K = 9, 257, 8, 5, 4
  halves = [ref.inputs(T, B, S, A, K, dirty=True, seed=s) for s in (1, 2)]
  both = {'states': np.concatenate([h['states'] for h in halves]),
          'actions': np.concatenate([h['actions'] for h in halves]),
          'values': [np.concatenate([h['values'][k] for h in halves]) for k in range(K)]}
  # one call over the concatenated streams, the limit taken from a call's own frame count
  want = ref.state_sums(both['states'], both['actions'], both['values'], S, A, frac_bits=F, N=T * B)
  for path in (1, 2, 0):
    out = {'raw': torch.full((K + 1, S, A), -12345, dtype=torch.int64, device='cuda'),
           'skipped': torch.full((1,), 77, dtype=torch.int64, device='cuda'),
           'clamped': torch.full((), 99, dtype=torch.int64, device='cuda')}
    for i, h in enumerate(halves):
      states, actions, values = _device(h, 'dense')
      got = sum_by_state(states, actions, tuple(values), n_states=S, n_actions=A, frac_bits=F,
                         accumulate=(i > 0), out=out, path=path)     # the first call overwrites the garbage
      assert got['raw'].data_ptr() == out['raw'].data_ptr()
      if i == 0:
        _check(got, ref.state_sums(h['states'], h['actions'], h['values'], S, A, frac_bits=F),
               (K + 1, S, A), path)
    _check(got, want, (K + 1, S, A), path)


def test_out_and_graph_capture():
  from campx_amd.returns import sum_by_state
  T, B, S, A, K = 9, 257, 8, 5, 1
  x = ref.inputs(T, B, S, A, K, dirty=True)
  states, actions, values = _device(x, 'dense')
  out = {'raw': torch.empty((K + 1, S, A), dtype=torch.int64, device='cuda'),
         'skipped': torch.empty((1,), dtype=torch.int64, device='cuda'),
         'clamped': torch.empty((1,), dtype=torch.int64, device='cuda')}
  call = lambda: sum_by_state(states, actions, tuple(values), n_states=S, n_actions=A, frac_bits=F,
                              out=out)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    call()                                    # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):               # one stream, no parallel branches
    call()
  for seed in (1, 2):
    y = ref.inputs(T, B, S, A, K, dirty=True, seed=seed)
    states.copy_(torch.from_numpy(y['states']))
    actions.copy_(torch.from_numpy(y['actions']))
    values[0].copy_(torch.from_numpy(y['values'][0]))
    out['raw'].fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    want = ref.state_sums(y['states'], y['actions'], y['values'], S, A, frac_bits=F)
    assert np.array_equal(out['raw'].cpu().numpy().reshape(K + 1, -1), want['raw']), seed
    assert (int(out['skipped']), int(out['clamped'])) == (want['skipped'], want['clamped']), seed


def test_the_streams_of_a_real_rollout():
  from campx_amd.returns import sum_by_state
  T, B = 100, 4099
  game = _game(B)
  f = game.fused
  policy = torch.ones((f.n_states, 5), dtype=torch.float32, device='cuda')
  out = game.rollout_policy(policy, T, seed=5, reset_first=True)
  reward = torch.nan_to_num(out['reward'])
  S = f.n_states
  got = sum_by_state(out['states'], out['actions'], (reward,), n_states=S)
  assert got['count'].shape == (S, 5) and int(got['count'].sum()) == T * B
  assert int(got['skipped']) == 0 and int(got['clamped']) == 0
  s, a = out['states'].cpu().numpy().astype(np.int64), out['actions'].cpu().numpy().astype(np.int64)
  assert np.array_equal(got['count'].cpu().numpy().reshape(-1), np.bincount((s * 5 + a).reshape(-1), minlength=S * 5))
  want = ref.state_sums(s.astype(np.int32), a.astype(np.int8), [reward.cpu().numpy()], S, 5, frac_bits=F)
  assert np.array_equal(got['raw'].cpu().numpy().reshape(2, -1), want['raw'])
  assert len(np.unique(got['count'].cpu().numpy())) > 5        # (and the bins are not all alike)
  f.check_actions()


def test_argument_errors_raise_before_any_launch():
  from campx_amd.returns import sum_by_state
  T, B, S, A, K = 9, 65, 8, 5, 1
  x = ref.inputs(T, B, S, A, 4)
  states, actions, values = _device(x, 'dense')
  out = {'raw': torch.full((K + 1, S, A), 123, dtype=torch.int64, device='cuda'),
         'skipped': torch.full((1,), 123, dtype=torch.int64, device='cuda'),
         'clamped': torch.full((1,), 123, dtype=torch.int64, device='cuda')}
  good = dict(states=states, actions=actions, values=(values[0],), n_states=S, n_actions=A,
              frac_bits=F, out=out)
  sideways = lambda dtype: torch.zeros((B, T), dtype=dtype, device='cuda').t()     # stride(1) = T
  narrow = lambda t: torch.as_strided(t, (T, B), (B - 1, 1))                       # pitch below B
  assert sideways(torch.int32).stride(1) != 1 and narrow(states).stride(0) < B
  bad = {
      'states dtype': dict(states=states.long()),
      'states not a tensor': dict(states=x['states']),
      'states on the CPU': dict(states=states.cpu()),
      'everything on the CPU': dict(states=states.cpu(), actions=actions.cpu(), values=(values[0].cpu(),)),
      'states stride(1)': dict(states=sideways(torch.int32)),
      'states pitch': dict(states=narrow(states)),
      'actions dtype': dict(actions=actions.int()),
      'actions shape': dict(actions=actions[:, :B - 1]),
      'actions on the CPU': dict(actions=actions.cpu()),
      'actions stride(1)': dict(actions=sideways(torch.int8)),
      'actions pitch': dict(actions=narrow(actions)),
      'values dtype': dict(values=(values[0].double(),)),
      'values shape': dict(values=(values[0][:T - 1],)),
      'values on the CPU': dict(values=(values[0].cpu(),)),
      'values stride(1)': dict(values=(sideways(torch.float32),)),
      'values pitch': dict(values=(narrow(values[0]),)),
      'values not a tuple': dict(values=values[0]),
      'K > 4': dict(values=tuple(values) + (values[0],),
                    out=dict(out, raw=torch.full((6, S, A), 123, dtype=torch.int64, device='cuda'))),
      'n_states 0': dict(n_states=0),
      'n_states missing': dict(n_states=None),
      'n_actions 0': dict(n_actions=0),
      'n_actions 129': dict(n_actions=129),
      'frac_bits negative': dict(frac_bits=-1),
      'frac_bits past what N allows': dict(frac_bits=62 - ref.limits(T * B)[0] + 1),
      'frac_bits type': dict(frac_bits=24.0),
      'path': dict(path=3),
      'path 1 for a table that does not fit': dict(path=1, n_states=70000,
                                                   out=dict(out, raw=torch.full((K + 1, 70000, A), 123, dtype=torch.int64, device='cuda'))),
      'out not a dict': dict(out=out['raw']),
      'out raw shape': dict(out=dict(out, raw=out['raw'][:, :S - 1].contiguous())),
      'out raw planes': dict(out=dict(out, raw=out['raw'][:1])),
      'out raw dtype': dict(out=dict(out, raw=out['raw'].int())),
      'out raw not contiguous': dict(out=dict(out, raw=torch.full((K + 1, S, 2 * A), 123, dtype=torch.int64, device='cuda')[..., :A])),
      'out without counters': dict(out={'raw': out['raw']}),
      'out counter dtype': dict(out=dict(out, skipped=out['skipped'].int())),
      'accumulate without out': dict(accumulate=True, out=None),
  }
  for what, change in bad.items():
    with pytest.raises(ValueError):
      sum_by_state(**dict(good, **change))
      pytest.fail('no ValueError for: ' + what)
  torch.cuda.synchronize()
  for k in ('raw', 'skipped', 'clamped'):
    assert bool((out[k] == 123).all()), k
  assert sum_by_state(**dict(good, frac_bits=62 - ref.limits(T * B)[0]))['raw'] is out['raw']
  got = sum_by_state(**good)                         # and the good call goes through
  _check(got, ref.state_sums(x['states'], x['actions'], x['values'][:1], S, A, frac_bits=F), (K + 1, S, A), 'good')


def test_opcheck():
  T, B, S, A = 9, 65, 8, 5
  x = ref.inputs(T, B, S, A, 1, dirty=True)
  states, actions, values = _device(x, 'dense')
  raw = torch.zeros((2, S, A), dtype=torch.int64, device='cuda')
  skipped = torch.zeros((1,), dtype=torch.int64, device='cuda')
  clamped = torch.zeros((1,), dtype=torch.int64, device='cuda')
  torch.library.opcheck(torch.ops.campx.state_sums.default,
                        (states, actions, values, S, A, F, False, 0, raw, skipped, clamped))
