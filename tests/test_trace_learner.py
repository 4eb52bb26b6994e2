"""Online learners with eligibility traces on the GPU: `WideGame.learn_traces()` (csrc/k_learn.hip,
`campx::wide_learn_traces`) against tests/trace_learner_reference.py - a numpy walk of the game's
state table under the frame of include/campx_hip.h - bit for bit: q, traces, the three window
tensors, state, done, ret.

The games are test_learner.py's: boat_race (8 states, hidden performance: one lane per learner, q
and traces lane-innermost in LDS), maze (159 states: teams of 16 lanes, entry-innermost), pickups
(470 states, episodes that end: teams of 64).  Hyper-parameters and tables are ordinary numbers;
tests/test_trace_learner_edges.py has the subnormals, signed zeros, infinities and NaN.
"""

import ctypes
import gc
import re

import numpy as np
import pytest
import torch

import trace_learner_reference as trace_ref
from test_learner import CALLS, FAR, GAMES, SEED, _hyper, _random_q
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

LAMS = np.array([0.0, 1.0, 0.5, 0.9], np.float32)


def _lam(B):
  return LAMS[np.arange(B) % 4]


def _cuda(*arrays):
  return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _plan(f, path=0, team=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_traces_plan(f.n_states, int(f.has_perf), f.batch,
                                         _hip.config_get('wide_lds_max'), path, team, plan)
  return code, list(plan)


def _check(f, res, want, L, q, z):
  assert res['q'] is q and res['traces'] is z
  assert _same(q.cpu().numpy(), L.q), 'q'
  assert _same(z.cpu().numpy(), L.z), 'traces'
  assert res['reward_sum'].dtype == torch.float32 and res['episodes'].dtype == torch.int32
  assert _same(res['reward_sum'].cpu().numpy(), want['reward_sum']), 'reward_sum'
  assert np.array_equal(res['episodes'].cpu().numpy(), want['episodes']), 'episodes'
  if f.has_perf:
    assert res['perf_sum'].dtype == torch.int32
    assert np.array_equal(res['perf_sum'].cpu().numpy(), want['perf_sum']), 'perf_sum'
  else:
    assert 'perf_sum' not in res
  assert np.array_equal(f.state.cpu().numpy(), L.state)
  assert np.array_equal(f.done.cpu().numpy(), L.over.astype(np.uint8))
  assert _same(f.ret.cpu().numpy(), L.ret)


def test_names_the_teams_the_games_take():
  plans = {name: _plan(_game(name, 1).fused) for name in GAMES}
  assert plans['boat_race'] == (0, [1, 1, 320 + 48 + 81920, 256, 1])
  assert plans['maze'] == (0, [1, 16, 6368 + 16 * 159 * 40, 256, 1])
  assert plans['pickups'] == (0, [1, 64, 18800 + 4 * 470 * 40, 256, 1])


@pytest.mark.parametrize('kind', trace_ref.KINDS)
@pytest.mark.parametrize('rule', trace_ref.RULES)
@pytest.mark.parametrize('B', [1, 63, 65, 257])
@pytest.mark.parametrize('name', GAMES)
def test_learners_against_the_reference_walk(name, B, rule, kind):
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon = _hyper(B)
  lam = _lam(B)
  hyper = dict(zip(('alpha', 'gamma', 'epsilon', 'lam'), _cuda(alpha, gamma, epsilon, lam)))
  q0 = _random_q(B, S)
  q, z = _cuda(q0, np.zeros_like(q0))
  L = trace_ref.TraceLearners(f.traced, B, q0)
  kw = dict(rule=rule, seed=SEED)
  frame = 0
  for T, window, reset in CALLS:
    res = game.learn_traces(T, q, z, trace=kind, reset_first=reset, window=window, **kw, **hyper)
    want = L.learn_traces(T, lam, kind, alpha, gamma, epsilon, reset_first=reset, window=window, **kw)
    W = 1 if window is None else (T + window - 1) // window
    assert res['reward_sum'].shape == (W, B) and res['episodes'].shape == (W, B)
    _check(f, res, want, L, q, z)
    frame += T
    assert f._policy_frame == frame == L.frame and f.frame == frame
  assert want['bad'] == 0 and (B == 1 or (not _same(L.q, q0) and L.z.any()))
  # an explicit first_frame: inside a pair, the high counter word in use; into buffers made once
  bufs = game.learner_buffers(5, window=2)
  res = game.learn_traces(5, q, z, trace=kind, first_frame=FAR, window=2, out=bufs, **kw, **hyper)
  want = L.learn_traces(5, lam, kind, alpha, gamma, epsilon, first_frame=FAR, window=2, **kw)
  assert res['reward_sum'] is bufs['reward_sum'] and res['episodes'] is bufs['episodes']
  _check(f, res, want, L, q, z)
  assert f._policy_frame == FAR + 5
  game.fused.check_actions()


@pytest.mark.parametrize('rule', trace_ref.RULES)
@pytest.mark.parametrize('S', [14, 15, 28, 29])
def test_synthetic_tables_on_both_sides_of_a_team_boundary(S, rule):
  """Tables of tests/wide_table_reference.py with discount codes, hidden performance and episodes
  that end: 14 states is the largest table with one lane per learner, 28 with two."""
  import types
  import wide_table_reference as table_ref
  from campx_amd import wide
  B = 65
  g = table_ref.make_table(S * 100 + B, 4, 5, 4, 2, S, dcodes=True, perf=True)
  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', g)
  f.showtime()
  assert _plan(f)[1][:2] == [1, {14: 1, 15: 2, 28: 2, 29: 4}[S]]
  assert (g.st_dcode != 0).any() and g.st_done.any()
  alpha, gamma, epsilon = _hyper(B)
  lam = _lam(B)
  hyper = _cuda(alpha, gamma, epsilon)
  q0 = _random_q(B, S)
  q, z = _cuda(q0, np.zeros_like(q0))
  L = trace_ref.TraceLearners(g, B, q0)
  for kind, T, first in (('accumulating', 11, 1), ('replacing', 6, None)):
    res = f.learn_traces(T, q, z, _cuda(lam)[0], kind, *hyper, rule, SEED, first, window=4)
    want = L.learn_traces(T, lam, kind, alpha, gamma, epsilon, rule, SEED, first, window=4)
    _check(f, res, want, L, q, z)
  assert np.abs(want['perf_sum']).max() > 0
  f.check_actions()


def _run(game, B, S, T, path, team, rule, kind, lds_max=None):
  from campx_amd import _hip
  alpha, gamma, epsilon = _hyper(B)
  hyper = dict(zip(('alpha', 'gamma', 'epsilon', 'lam'), _cuda(alpha, gamma, epsilon, _lam(B))))
  q0 = _random_q(B, S)
  q, z = _cuda(q0, np.zeros_like(q0))
  with _hip.config(**({} if lds_max is None else {'wide_lds_max': lds_max})):
    for first in (3, None):                     # (two calls: the traces are carried)
      res = game.learn_traces(T, q, z, trace=kind, rule=rule, seed=SEED, first_frame=first, window=4,
                              path=path, team=team, reset_first=first == 3, **hyper)
    torch.cuda.synchronize()
  return ({k: v.cpu().numpy() for k, v in res.items()}
          | {'state': game.fused.state.cpu().numpy(), 'ret': game.fused.ret.cpu().numpy()})


@pytest.mark.parametrize('rule,kind', [('q', 'accumulating'), ('expected_sarsa', 'replacing')])
def test_every_team_on_each_path_gives_the_same_bits(rule, kind):
  """The boat race at B = 65: a partial last workgroup for every team up to 64 and, at 256 lanes a
  learner, one learner per workgroup; the last run has even the entries read through L1 / L2."""
  B, T = 65, 13
  game = _game('boat_race', B)
  f = game.fused
  L = trace_ref.TraceLearners(f.traced, B, _random_q(B, 8))
  alpha, gamma, epsilon = _hyper(B)
  for first in (3, None):
    want = L.learn_traces(T, _lam(B), kind, alpha, gamma, epsilon, rule, SEED, first, first == 3, 4)
  runs = [(path, team, None) for path in (1, 2) for team in (1, 2, 8, 64, 256)] + [(0, 0, None), (2, 8, 0)]
  for path, team, lds_max in runs:
    assert _plan(f, path, team)[1][:2] == [path or 1, team or 1]
    got = _run(game, B, 8, T, path, team, rule, kind, lds_max)
    assert _same(got['q'], L.q) and _same(got['traces'], L.z), (path, team)
    assert _same(got['reward_sum'], want['reward_sum']), (path, team)
    assert np.array_equal(got['perf_sum'], want['perf_sum']), (path, team)
    assert np.array_equal(got['episodes'], want['episodes']), (path, team)
    assert np.array_equal(got['state'], L.state) and _same(got['ret'], L.ret), (path, team)


def test_forced_teams_on_the_maze_with_an_absent_team_in_the_last_workgroup():
  """The maze forced to 2 learners per workgroup (team 128) at B = 65: the last workgroup holds one
  learner and an absent team; against the planned team of 16."""
  B, T = 65, 9
  game = _game('maze', B)
  planned = _run(game, B, 159, T, 0, 0, 'q', 'accumulating')
  for path, team in ((1, 128), (2, 128), (2, 256), (2, 1)):
    got = _run(game, B, 159, T, path, team, 'q', 'accumulating')
    for k in planned:
      assert _same(planned[k], got[k]), (k, path, team)


@pytest.mark.parametrize('kind', trace_ref.KINDS)
@pytest.mark.parametrize('rule', trace_ref.RULES)
@pytest.mark.parametrize('name', ['boat_race', 'maze'])
def test_lam_zero_is_learn_tabular_bit_for_bit(name, rule, kind):
  B = 65
  alpha, gamma, epsilon = _hyper(B)
  hyper = dict(zip(('alpha', 'gamma', 'epsilon'), _cuda(alpha, gamma, epsilon)))
  got = []
  for traces in (False, True):
    game = _game(name, B)
    f = game.fused
    q = _cuda(_random_q(B, f.n_states))[0]
    for T, window, reset in CALLS:
      kw = dict(rule=rule, seed=SEED, reset_first=reset, window=window, **hyper)
      res = (game.learn_traces(T, q, None, lam=0.0, trace=kind, **kw) if traces
             else game.learn_tabular(T, q, **kw))
    got.append({k: res[k].cpu().numpy() for k in res if k != 'traces'}
               | {'state': f.state.cpu().numpy(), 'done': f.done.cpu().numpy(), 'ret': f.ret.cpu().numpy()})
  for k in got[0]:
    assert _same(got[0][k], got[1][k]), k
  assert not res['traces'].any()


@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_calls_of_5_and_6_frames_are_one_call_of_11(name):
  B = 65
  hyper = dict(alpha=0.3, gamma=0.9, epsilon=0.25, lam=0.8, seed=SEED)
  ends = []
  for split in ((11,), (5, 6)):
    game = _game(name, B)
    f = game.fused
    q, z = _cuda(_random_q(B, f.n_states), np.zeros((B, f.n_states, 5), np.float32))
    for i, T in enumerate(split):
      game.learn_traces(T, q, z, reset_first=i == 0, **hyper)
    ends.append((q.cpu().numpy(), z.cpu().numpy(), f.state.cpu().numpy(), f.ret.cpu().numpy()))
    assert f._policy_frame == 11
  for one, two in zip(*ends):
    assert _same(one, two)
  assert ends[0][1].any()


def test_reset_first_zeroes_the_traces():
  B = 65
  game = _game('boat_race', B)
  f = game.fused
  q0 = _random_q(B, 8)
  z0 = np.abs(_random_q(B, 8, seed=1))
  hyper = dict(alpha=0.3, gamma=0.9, epsilon=0.25, lam=0.8, seed=SEED, rule='expected_sarsa')
  q, z = _cuda(q0, z0)
  game.learn_traces(3, q, z, reset_first=True, **hyper)
  L = trace_ref.TraceLearners(f.traced, B, q0, z0)
  L.learn_traces(3, reset_first=True, **hyper)
  assert _same(q.cpu().numpy(), L.q) and _same(z.cpu().numpy(), L.z)
  # as if the traces had been zeros: at most three entries of a learner have one
  assert (np.count_nonzero(L.z.reshape(B, -1), axis=1) <= 3).all()
  fresh = trace_ref.TraceLearners(f.traced, B, q0)
  fresh.learn_traces(3, reset_first=True, **hyper)
  assert _same(fresh.q, L.q) and _same(fresh.z, L.z)


def test_zeros_for_q_and_traces_and_numbers_for_hyper_parameters():
  B = 65
  game = _game('boat_race', B)
  f = game.fused
  res = game.learn_traces(12, lam=0.75, trace='replacing', alpha=0.25, gamma=0.5, epsilon=0.5, seed=3,
                          window=5, reset_first=True)
  L = trace_ref.TraceLearners(f.traced, B)
  want = L.learn_traces(12, 0.75, 'replacing', 0.25, 0.5, 0.5, seed=3, window=5, reset_first=True)
  assert res['q'].shape == res['traces'].shape == (B, 8, 5) and res['traces'].dtype == torch.float32
  _check(f, res, want, L, res['q'], res['traces'])
  assert np.abs(L.q).max() > 0
  # the defaults: lam 0.9, accumulating, alpha 0.1, gamma 0.99, epsilon 0.1, rule 'q', seed 0
  res = game.learn_traces(4, res['q'], res['traces'])
  want = L.learn_traces(4)
  _check(f, res, want, L, res['q'], res['traces'])
  # a captured learn_tabular() never sees lam: the numbers live in tensors of their own
  assert ('learn_traces', B) in f._hyper_floats and ('learn_tabular', B) not in f._hyper_floats


@pytest.mark.parametrize('name,B', [('boat_race', 257), ('maze', 65)])
def test_bad_learners_keep_table_and_traces_and_their_neighbours_learn(name, B):
  T = 10
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon = _hyper(B)
  lam = _lam(B)
  lam[3], lam[40], alpha[64] = np.nan, 1.5, np.inf
  q0, z0 = _random_q(B, S), np.abs(_random_q(B, S, seed=1))
  q, z = _cuda(q0, z0)
  bufs = game.learner_buffers(T, window=4)
  with pytest.raises(ValueError) as caught:
    game.learn_traces(T, q, z, *_cuda(lam), 'accumulating', *_cuda(alpha, gamma, epsilon), seed=SEED,
                      window=4, out=bufs, reset_first=True)
    f.check_actions()
  assert re.match(r'^3 learners of learn_traces\(\) have bad hyper-parameters', str(caught.value))
  assert 'they took action 4 at every frame' in str(caught.value)
  torch.cuda.synchronize()
  L = trace_ref.TraceLearners(f.traced, B, q0, z0)
  want = L.learn_traces(T, lam, 'accumulating', alpha, gamma, epsilon, seed=SEED, window=4,
                        reset_first=True)
  assert want['bad'] == 3
  got_q, got_z = q.cpu().numpy(), z.cpu().numpy()
  bad = [3, 40, 64]
  assert _same(got_q[bad], q0[bad]) and _same(got_z[bad], z0[bad])
  assert not _same(got_q[2], q0[2]) and not _same(got_q[41], q0[41])
  _check(f, dict(bufs, q=q, traces=z), want, L, q, z)
  f.check_actions()                                  # the counters were cleared
  assert int(f._bad_trace_learners.item()) == 0


def test_argument_errors_raise_before_anything_is_launched():
  B = 64
  game = _game('boat_race', B)
  f = game.fused
  q = torch.zeros((B, 8, 5), device='cuda')
  z = torch.zeros((B, 8, 5), device='cuda')
  for kw in (dict(lam=float('nan')), dict(lam=1.5), dict(lam=-0.1), dict(lam='0.9'),
             dict(lam=torch.zeros((B,))), dict(lam=torch.zeros((B + 1,), device='cuda')),
             dict(trace='dutch'), dict(trace=0), dict(alpha=float('nan')), dict(epsilon=1.5),
             dict(rule='sarsa'), dict(window=0), dict(first_frame=-1), dict(path=3), dict(team=3),
             dict(team=512), dict(team=-2), dict(team=2.0), dict(out={}),
             dict(out=game.learner_buffers(4, window=3))):
    with pytest.raises(ValueError):
      game.learn_traces(4, q, z, **kw)
  for name in ('q', 'traces'):
    for bad in (torch.zeros((B, 8, 4), device='cuda'), torch.zeros((B, 8, 5)), q.double(),
                torch.zeros((B * 40 + 1,), device='cuda')[1:].view(B, 8, 5), 'q'):
      with pytest.raises(ValueError, match=name + ' must be a contiguous, 16-byte aligned'):
        game.learn_traces(4, **{'q': q, 'traces': z, name: bad})
  with pytest.raises(ValueError):
    game.learn_traces(0, q, z)
  assert f._policy_frame == 0 and f.frame == 0 and not bool(q.any()) and not bool(z.any())
  # a forced shape that does not fit names the setting
  maze = _game('maze', 64)
  with pytest.raises(ValueError, match=r'path=1, team=8: a table of 159 states .* wide_lds_max'):
    maze.learn_traces(4, path=1, team=8)
  assert maze.fused._policy_frame == 0


def test_a_captured_call_allocates_nothing_and_replays_to_the_same_bits():
  B, T = 257, 9
  game = _game('maze', B)                      # teams of 16: barriers inside the captured kernel
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon, lam = _cuda(*_hyper(B), _lam(B))
  q0 = _cuda(_random_q(B, S))[0]
  kw = dict(alpha=alpha, gamma=gamma, epsilon=epsilon, lam=lam, rule='expected_sarsa',
            trace='replacing', seed=SEED, first_frame=5, window=4)

  def start(q, z):
    q.copy_(q0)
    z.zero_()
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()

  q_eager, z_eager, q_graph, z_graph = (torch.empty_like(q0) for _ in range(4))
  start(q_eager, z_eager)
  eager = game.learn_traces(T, q_eager, z_eager, **kw)
  eager = {k: v.clone() for k, v in eager.items()}
  end = f.state.clone(), f.done.clone(), f.ret.clone()
  bufs = game.learner_buffers(T, window=4)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    game.learn_traces(T, q_graph, z_graph, out=bufs, **kw)       # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  gc.collect()                                 # (no dead cycle of an earlier test is left to be
  gc.disable()                                 #  collected - and to free device memory - mid-capture)
  try:
    with torch.cuda.graph(graph):              # one stream, no parallel branches
      before = torch.cuda.memory_allocated()   # (the capture itself has made its generator state)
      game.learn_traces(T, q_graph, z_graph, out=bufs, **kw)
      allocated = torch.cuda.memory_allocated() - before
  finally:
    gc.enable()
  assert allocated == 0
  start(q_graph, z_graph)
  for t in bufs.values():
    t.fill_(-1)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(q_graph.view(torch.int32), eager['q'].view(torch.int32))
  assert torch.equal(z_graph.view(torch.int32), eager['traces'].view(torch.int32))
  for k in ('reward_sum', 'episodes'):
    assert torch.equal(bufs[k], eager[k]), k
  assert torch.equal(f.state, end[0]) and torch.equal(f.done, end[1]) and torch.equal(f.ret, end[2])
  assert bool(z_graph.any())
  game.fused.check_actions()
