"""`campx_amd.returns.vtrace_returns()` on the GPU (csrc/k_vtrace.hip, `campx::vtrace`) against
tests/vtrace_reference.py, the rule restated in numpy float32: every comparison is of bits.
Shapes as in tests/test_returns.py: every T of {1, 7, 8, 9, 100} - both sides of the kernel's
8-frame chunk - at B = 257, every B of {1, 63, 64, 65, 4 099} - both sides of a wave and of a
256-lane block - at T = 9.  Ratio mode dense and as padded views with a pitch per stream; table
mode on every path against ratio mode fed the quotient computed on the host; bad ids at known
frames; the boat race's population rollout end to end, eagerly and from a captured graph."""

import functools

import numpy as np
import pytest
import torch

import vtrace_reference as ref
from test_returns import _game, _padded, up16

pytestmark = pytest.mark.gpu

GAMMA = 0.99
LAMS = (1.0, 0.95, 0.0)
BARS = ((1.0, 1.0, None), (2.0, 0.5, 3.0), (1.0, 0.0, 1.0))          # rho_bar, c_bar, pg_rho_bar
CASES = [(T, 257) for T in (1, 7, 8, 9, 100)] + [(9, B) for B in (1, 63, 64, 65, 4099)]
STREAMS = ('reward', 'done', 'discount', 'values', 'bootstrap')


@functools.lru_cache(maxsize=None)
def _inputs(T, B):
  return dict(ref.inputs(T, B), ratio=ref.ratios(T, B))


@functools.lru_cache(maxsize=None)
def _want(T, B, with_discount, with_bootstrap, lam, bars):
  x = _inputs(T, B)
  return ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], x['ratio'],
                    discount=x['discount'] if with_discount else None,
                    bootstrap=x['bootstrap'] if with_bootstrap else None, lam=lam, rho_bar=bars[0],
                    c_bar=bars[1], pg_rho_bar=bars[2])


def _device_inputs(T, B, layout):
  x = _inputs(T, B)
  if layout == 'dense':
    return {k: torch.from_numpy(x[k]).cuda() for k in STREAMS + ('ratio',)}
  bufs = _game(B).rollout_trace_buffers(T)         # reward / discount / done: rows padded to 16
  d = {}
  for k in ('reward', 'done', 'discount'):
    bufs[k].copy_(torch.from_numpy(x[k]))
    d[k] = bufs[k]
  d['values'] = _padded(x['values'], B + 7)
  d['ratio'] = _padded(x['ratio'], B + 5)
  d['bootstrap'] = torch.from_numpy(x['bootstrap']).cuda()
  return d


def _outputs(T, B, layout):
  if layout == 'dense':
    return None
  return {'vs': torch.zeros((T, B + 3), dtype=torch.float32, device='cuda')[:, :B],
          'advantages': torch.zeros((T, up16(B) + 16), dtype=torch.float32, device='cuda')[:, :B]}


def _same(got, want, what):
  for k in ('vs', 'advantages'):
    g = got[k].cpu().numpy()
    assert g.shape == want[k].shape and got[k].dtype == torch.float32, (what, k)
    assert ref.same_bits(g, want[k]), (what, k)


@pytest.mark.parametrize('layout', ['dense', 'padded'])
@pytest.mark.parametrize('T,B', CASES, ids=['T{}-B{}'.format(T, B) for T, B in CASES])
def test_ratio_mode_bit_for_bit(T, B, layout):
  from campx_amd.returns import vtrace_returns
  d = _device_inputs(T, B, layout)
  if layout == 'padded' and T > 1:
    pitches = {d['reward'].stride(0), d['values'].stride(0), d['ratio'].stride(0), B + 3, up16(B) + 16}
    assert len(pitches) == 5
  n = 0
  for with_discount in (True, False):
    for with_bootstrap in (True, False):
      for lam in LAMS:
        for bars in BARS:
          out = _outputs(T, B, layout)
          got = vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], ratio=d['ratio'],
                               discount=d['discount'] if with_discount else None,
                               bootstrap=d['bootstrap'] if with_bootstrap else None, lam=lam,
                               rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2], out=out)
          what = (with_discount, with_bootstrap, lam, bars)
          assert set(got) == {'vs', 'advantages'}, what
          if out is not None:
            assert got['vs'].data_ptr() == out['vs'].data_ptr()
          for k in got:                               # no ratio, no NaN reward reaches the outputs
            assert not bool(torch.isnan(got[k]).any()), (what, k)
          _same(got, _want(T, B, with_discount, with_bootstrap, lam, bars), what)
          n += 1
  assert n == 36


def test_the_inputs_hold_what_the_docstring_says():
  x = _inputs(100, 257)
  w = x['ratio']
  assert np.isnan(w).mean() > 0.01 and (w == -1).mean() > 0.01 and np.isinf(w).mean() > 0.01
  assert set(np.unique(w[np.isfinite(w)])) == {-1.0, 0.0, 0.25, 0.5, 1.0, 1.5, 4.0}
  assert np.isnan(x['reward']).any() and x['done'][:, x['forced']['all']].all()


@pytest.mark.parametrize('lam', LAMS)
def test_on_policy_identity_on_the_device(lam):
  """A ratio of ones and bars of 1: vs is values + discounted_returns()'s advantages, bit for bit."""
  from campx_amd.returns import discounted_returns, vtrace_returns
  T, B = 100, 257
  d = _device_inputs(T, B, 'dense')
  ones = torch.ones((T, B), dtype=torch.float32, device='cuda')
  got = vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], ratio=ones, discount=d['discount'],
                       bootstrap=d['bootstrap'], lam=lam)
  gae = discounted_returns(d['reward'], d['done'], GAMMA, discount=d['discount'], values=d['values'],
                           bootstrap=d['bootstrap'], lam=lam)
  assert torch.equal(got['vs'].view(torch.int32), (d['values'] + gae['advantages']).view(torch.int32))


# ------------------------------------------------------------------ table mode

TABLE_T, TABLE_B = 20, 257
TABLE_SIZES = ((8, 8), (8, 24), (1, 1), (1, 6), (2500, 2500))        # Nt, Nb


@functools.lru_cache(maxsize=None)
def _table_inputs(Nt, Nb):
  T, B = TABLE_T, TABLE_B
  target, behaviour = ref.tables(Nt, Nb)
  states, actions = ref.ids(T, B, Nb)
  w0, bad = ref.table_ratio(target, behaviour, states, actions)
  assert bad == 0 and (w0 > 2.0).any() and (w0 < 0.5).any()
  return dict(ref.inputs(T, B), target=target, behaviour=behaviour, states=states, actions=actions, ratio=w0)


def _fits(Nt, Nb, A=5):
  from campx_amd import _hip
  return (Nt + Nb) * A * 4 <= _hip.SUMS_LDS_BUDGET


@pytest.mark.parametrize('Nt,Nb', TABLE_SIZES, ids=['Nt{}-Nb{}'.format(*s) for s in TABLE_SIZES])
def test_table_mode_is_ratio_mode_fed_the_quotient_on_every_path(Nt, Nb):
  from campx_amd.returns import vtrace_returns
  T, B = TABLE_T, TABLE_B
  x = _table_inputs(Nt, Nb)
  d = {k: torch.from_numpy(x[k]).cuda() for k in STREAMS + ('target', 'behaviour', 'ratio')}
  states, actions = _padded(x['states'], B + 9), _padded(x['actions'], up16(B) + 32)
  kw = dict(discount=d['discount'], bootstrap=d['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.5, pg_rho_bar=3.0)
  want = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], x['ratio'], discount=x['discount'],
                    bootstrap=x['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.5, pg_rho_bar=3.0)
  by_ratio = vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], ratio=d['ratio'], **kw)
  _same(by_ratio, want, 'ratio')
  assert _fits(Nt, Nb) == (Nt != 2500)
  bad = torch.full((1,), 5, dtype=torch.int64, device='cuda')
  for path in (0, 1, 2):
    if path == 1 and not _fits(Nt, Nb):
      with pytest.raises(ValueError, match='do not fit the LDS budget'):
        vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], target=d['target'], behaviour=d['behaviour'],
                       states=states, actions=actions, path=1, **kw)
      continue
    for with_discount in (True, False):
      got = vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], target=d['target'],
                           behaviour=d['behaviour'], states=states, actions=actions, bad_count=bad, path=path,
                           **dict(kw, discount=d['discount'] if with_discount else None))
      if with_discount:
        _same(got, want, ('path', path))
      else:
        plain = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], x['ratio'], bootstrap=x['bootstrap'],
                           lam=0.95, rho_bar=2.0, c_bar=0.5, pg_rho_bar=3.0)
        _same(got, plain, ('path', path, 'no discount'))
  assert int(bad) == 5                                # every id is in range


BAD_T, BAD_B = 21, 257                                # two chunks of eight frames and a partial one of five


@functools.lru_cache(maxsize=None)
def _bad_inputs(Nt, Nb):
  """Bad states {-1, Nb, 2^31 - 1} and bad actions {-1, 5, 127} at known frames: the last frame
  (the first the kernel's first chunk takes) and frame 13 (its last), frames 12 and 5 (the same of
  the second chunk), frames 4, 1 and 0 (the partial chunk), in columns of two waves and of the
  second block."""
  T, B = BAD_T, BAD_B
  x = dict(_table_inputs_at(T, B, Nt, Nb))
  states, actions = x['states'].copy(), x['actions'].copy()
  frames = (T - 1, 13, 12, 5, 4, 1, 0)
  n = 0
  for i, t in enumerate(frames):
    for k, col in enumerate((0, 3, 64, 200, 256)):
      which = (i + k) % 6
      if which < 3:
        states[t, col] = (-1, Nb, 2 ** 31 - 1)[which]
      else:
        actions[t, col] = (-1, 5, 127)[which - 3]
      n += 1
  states[7, 100], actions[7, 100] = Nb, 5             # both bad: one frame, counted once
  n += 1
  w0, bad = ref.table_ratio(x['target'], x['behaviour'], states, actions)
  assert bad == n == 36
  return dict(x, states=states, actions=actions, ratio=w0, bad=bad)


@functools.lru_cache(maxsize=None)
def _table_inputs_at(T, B, Nt, Nb):
  target, behaviour = ref.tables(Nt, Nb)
  states, actions = ref.ids(T, B, Nb)
  return dict(ref.inputs(T, B), target=target, behaviour=behaviour, states=states, actions=actions)


@pytest.mark.parametrize('Nt,Nb', [(8, 24), (2500, 2500)], ids=['Nt8-Nb24', 'Nt2500-Nb2500'])
def test_bad_ids_count_as_a_ratio_of_zero_and_are_counted_exactly(Nt, Nb):
  from campx_amd.returns import vtrace_returns
  x = _bad_inputs(Nt, Nb)
  d = {k: torch.from_numpy(x[k]).cuda() for k in STREAMS + ('target', 'behaviour', 'states', 'actions')}
  want = ref.vtrace(x['reward'], x['done'], GAMMA, x['values'], x['ratio'], discount=x['discount'],
                    bootstrap=x['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.5, pg_rho_bar=3.0)
  start = 1 << 40
  for path in (0, 1, 2):
    if path == 1 and not _fits(Nt, Nb):
      continue
    bad = torch.full((1,), start, dtype=torch.int64, device='cuda')
    got = vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], target=d['target'],
                         behaviour=d['behaviour'], states=d['states'], actions=d['actions'],
                         discount=d['discount'], bootstrap=d['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.5,
                         pg_rho_bar=3.0, bad_count=bad, path=path)
    _same(got, want, ('path', path))
    assert int(bad) == start + x['bad'], path         # exactly, and onto what was there
    got = vtrace_returns(d['reward'], d['done'], GAMMA, d['values'], target=d['target'],
                         behaviour=d['behaviour'], states=d['states'], actions=d['actions'],
                         discount=d['discount'], bootstrap=d['bootstrap'], lam=0.95, rho_bar=2.0, c_bar=0.5,
                         pg_rho_bar=3.0, path=path)                                    # without a counter
    _same(got, want, ('path', path, 'no counter'))


# ------------------------------------------------------------------ end to end

def _population(game, P, T, seed):
  S = game.fused.n_states
  rng = np.random.RandomState(seed)
  probs = rng.uniform(0.05, 1.0, size=(P, S, 5)).astype(np.float32)
  probs /= probs.sum(axis=2, keepdims=True)
  learner = rng.uniform(0.05, 1.0, size=(S, 5)).astype(np.float32)
  learner /= learner.sum(axis=1, keepdims=True)
  return probs.astype(np.float32), learner.astype(np.float32)


def test_boat_race_population_end_to_end_and_from_a_graph():
  """`rollout_population()` with P = 4, B = 1 024, T = 20: its padded buffers straight in, table
  mode, against the reference; then the same call captured in a HIP graph with `out=`."""
  from campx_amd.returns import vtrace_returns
  P, B, T = 4, 1024, 20
  game = _game(B)
  S = game.fused.n_states
  probs, learner = _population(game, P, T, 3)
  policies = torch.from_numpy(probs).cuda()
  target = torch.from_numpy(learner).cuda()
  bufs = game.rollout_population_buffers(T)
  values_table = np.random.RandomState(4).uniform(-1, 1, size=(P * S,)).astype(np.float32)
  out = {'vs': torch.zeros((T, B + 3), dtype=torch.float32, device='cuda')[:, :B],
         'advantages': torch.zeros((T, up16(B) + 16), dtype=torch.float32, device='cuda')[:, :B]}
  values = torch.empty((T, B), dtype=torch.float32, device='cuda')
  bootstrap = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, size=(B,)).astype(np.float32)).cuda()
  bad = torch.zeros((1,), dtype=torch.int64, device='cuda')

  def roll(seed):
    res = game.rollout_population(policies, T, seed=seed, reset_first=True, out=bufs)
    values.copy_(torch.from_numpy(values_table).cuda()[res['states'].long()])
    return res

  def call(res):
    return vtrace_returns(res['reward'], res['done'], GAMMA, values, target=target,
                          behaviour=policies.view(-1, 5), states=res['states'], actions=res['actions'],
                          discount=res['discount'], bootstrap=bootstrap, lam=0.95, rho_bar=1.0, c_bar=1.0,
                          bad_count=bad, out=out)

  def check(res, what):
    states, actions = res['states'].cpu().numpy(), res['actions'].cpu().numpy()
    assert states.max() >= S and states.min() >= 0     # flat ids: member * S + state
    w0, n_bad = ref.table_ratio(learner, probs.reshape(-1, 5), states, actions)
    assert n_bad == 0
    want = ref.vtrace(res['reward'].cpu().numpy(), res['done'].cpu().numpy(), GAMMA, values.cpu().numpy(), w0,
                      discount=res['discount'].cpu().numpy(), bootstrap=bootstrap.cpu().numpy(), lam=0.95)
    _same(out, want, what)

  res = roll(11)
  assert T == 1 or res['reward'].stride(0) >= B
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    got = call(res)                                   # (also the warm-up outside the capture)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  assert got['vs'].data_ptr() == out['vs'].data_ptr()
  check(res, 'eager')
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    call(res)
  for seed in (12, 13):
    res = roll(seed)
    out['vs'].zero_()
    out['advantages'].zero_()
    graph.replay()
    torch.cuda.synchronize()
    check(res, ('graph', seed))
  assert int(bad) == 0
  game.fused.check_actions()


def test_argument_errors_raise_before_any_launch():
  from campx_amd.returns import vtrace_returns
  T, B = 9, 65
  d = _device_inputs(T, B, 'dense')
  x = _table_inputs_at(T, B, 8, 24)
  tb = {k: torch.from_numpy(x[k]).cuda() for k in ('target', 'behaviour', 'states', 'actions')}
  out = {'vs': torch.full((T, B), 123.0, device='cuda'), 'advantages': torch.full((T, B), 123.0, device='cuda')}
  good = dict(reward=d['reward'], done=d['done'], gamma=GAMMA, values=d['values'], ratio=d['ratio'],
              discount=d['discount'], bootstrap=d['bootstrap'], lam=0.95, out=out)
  tabled = dict(good, ratio=None, **tb)
  sideways = torch.zeros((B, T), dtype=torch.float32, device='cuda').t()
  bad = {
      'reward device': dict(good, reward=d['reward'].cpu()),
      'reward stride(1)': dict(good, reward=sideways),
      'done dtype': dict(good, done=d['done'].bool()),
      'done shape': dict(good, done=d['done'][:, :B - 1]),
      'values None': dict(good, values=None),
      'values dtype': dict(good, values=d['values'].double()),
      'values shape': dict(good, values=d['values'][:T - 1]),
      'ratio dtype': dict(good, ratio=d['ratio'].half()),
      'ratio shape': dict(good, ratio=d['ratio'][:, :B - 1]),
      'ratio device': dict(good, ratio=d['ratio'].cpu()),
      'discount stride(1)': dict(good, discount=sideways),
      'bootstrap shape': dict(good, bootstrap=d['bootstrap'][:B - 1]),
      'bad_count dtype': dict(good, bad_count=torch.zeros((1,), dtype=torch.int32, device='cuda')),
      'bad_count size': dict(good, bad_count=torch.zeros((2,), dtype=torch.int64, device='cuda')),
      'out not a dict': dict(good, out=out['vs']),
      'out without advantages': dict(good, out={'vs': out['vs']}),
      'out shape': dict(good, out={'vs': out['vs'][:T - 1], 'advantages': out['advantages']}),
      'out dtype': dict(good, out={'vs': out['vs'].double(), 'advantages': out['advantages']}),
      'both modes': dict(tabled, ratio=d['ratio']),
      'no mode': dict(good, ratio=None),
      'target rank': dict(tabled, target=tb['target'][0]),
      'target dtype': dict(tabled, target=tb['target'].double()),
      'target device': dict(tabled, target=tb['target'].cpu()),
      'behaviour actions': dict(tabled, behaviour=tb['behaviour'][:, :4].contiguous()),
      'behaviour rows': dict(tabled, behaviour=tb['behaviour'][:23]),
      'behaviour not contiguous': dict(tabled, behaviour=tb['behaviour'][::2][:8]),
      'too many actions': dict(tabled, target=torch.ones((8, 129), device='cuda'),
                               behaviour=torch.ones((8, 129), device='cuda')),
      'states dtype': dict(tabled, states=tb['states'].long()),
      'states shape': dict(tabled, states=tb['states'][:, :B - 1]),
      'actions dtype': dict(tabled, actions=tb['actions'].int()),
      'path 1 too large': dict(tabled, target=torch.ones((2500, 5), device='cuda'),
                               behaviour=torch.ones((2500, 5), device='cuda'), path=1),
  }
  for what, kwargs in bad.items():
    with pytest.raises(ValueError):
      vtrace_returns(**kwargs)
      pytest.fail('no ValueError for: ' + what)
  torch.cuda.synchronize()
  assert bool((out['vs'] == 123.0).all()) and bool((out['advantages'] == 123.0).all())
  got = vtrace_returns(**good)                        # and the good calls go through
  _same(got, _want(T, B, True, True, 0.95, (1.0, 1.0, None)), 'good')
  got = vtrace_returns(**tabled)
  assert not bool(torch.isnan(got['vs']).any())
