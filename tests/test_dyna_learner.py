"""Dyna-Q online learners on the GPU: `WideGame.learn_dyna()` (csrc/k_learn.hip,
`campx::wide_learn_dyna`) against tests/dyna_learner_reference.py - a numpy walk of the game's state
table under the frame of include/campx_hip.h - bit for bit: q, the model (seen up to n_seen, n_seen),
the three window tensors, state, done, ret.

The games are test_learner.py's: boat_race (8 states, hidden performance: q, lists and bitmaps in
LDS), maze (159 states) and pickups (470 states, episodes that end), both through L1 / L2.
"""

import ctypes
import gc
import re

import numpy as np
import pytest
import torch

import dyna_learner_reference as dyna_ref
from test_learner import CALLS, FAR, GAMES, SEED, _hyper, _random_q
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

# a learner without planning, one update, a whole Philox block, one word into the next, two blocks
# and a word: in every wave the lanes leave the planning loop at different times
PLANNING = np.array([0, 1, 4, 5, 9], np.int32)


def _planning(B):
  return PLANNING[np.arange(B) % 5]


def _cuda(*arrays):
  return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _plan(f, path=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_dyna_plan(f.n_states, int(f.has_perf), f.batch,
                                       _hip.config_get('wide_lds_max'), path, plan)
  return code, list(plan)


def _model(B, S, fill=0):
  return {'seen': torch.full((B, S * 5), fill, dtype=torch.int32, device='cuda'),
          'n_seen': torch.zeros((B,), dtype=torch.int32, device='cuda')}


def _check_model(model, L):
  n = model['n_seen'].cpu().numpy()
  assert n.dtype == np.int32 and np.array_equal(n, L.n_seen), 'n_seen'
  listed = np.arange(L.seen.shape[1])[None, :] < n[:, None]
  got = model['seen'].cpu().numpy()
  assert np.array_equal(got[listed], L.seen[listed]), 'seen'


def _check(f, res, want, L, q, model):
  assert res['q'] is q and res['model'] is model
  assert _same(q.cpu().numpy(), L.q), 'q'
  _check_model(model, L)
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


def test_names_the_paths_the_games_take_and_dyna_buffers_follows_the_plan():
  for name, words in (('boat_race', [1, 320 + 48 + 63488, 256, 1, 2]), ('maze', [2, 6368, 256, 1, 25]),
                      ('pickups', [2, 18800, 256, 1, 74])):
    game = _game(name, 3)
    f = game.fused
    assert _plan(f) == (0, words)
    for path in (0, 2) + ((1,) if words[0] == 1 else ()):
      bufs = game.dyna_buffers(7, window=3, path=path)
      taken = _plan(f, path)[1][0]
      assert ('marks' in bufs) == (taken == 2), (name, path)
      assert set(bufs) - {'marks'} == set(game.learner_buffers(7, window=3))
      assert bufs['reward_sum'].shape == (3, 3)
      if taken == 2:
        assert bufs['marks'].dtype == torch.int32 and bufs['marks'].shape == (3, words[4])


@pytest.mark.parametrize('rule', dyna_ref.RULES)
@pytest.mark.parametrize('B', [1, 63, 65, 257])
@pytest.mark.parametrize('name', GAMES)
def test_learners_against_the_reference_walk(name, B, rule):
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon = _hyper(B)
  planning = _planning(B)
  hyper = dict(zip(('alpha', 'gamma', 'epsilon', 'planning'), _cuda(alpha, gamma, epsilon, planning)))
  q0 = _random_q(B, S)
  q = _cuda(q0)[0]
  model = _model(B, S)
  L = dyna_ref.DynaLearners(f.traced, B, q0)
  kw = dict(rule=rule, seed=SEED)
  frame = 0
  for T, window, reset in CALLS:
    res = game.learn_dyna(T, q, model, reset_first=reset, window=window, **kw, **hyper)
    want = L.learn_dyna(T, planning, alpha, gamma, epsilon, reset_first=reset, window=window, **kw)
    W = 1 if window is None else (T + window - 1) // window
    assert res['reward_sum'].shape == (W, B) and res['episodes'].shape == (W, B)
    _check(f, res, want, L, q, model)
    frame += T
    assert f._policy_frame == frame == L.frame and f.frame == frame
  assert want['bad'] == 0 and (B == 1 or not _same(L.q, q0)) and L.n_seen.min() >= 1
  # an explicit first_frame: the high counter word in use; into buffers made once
  bufs = game.dyna_buffers(5, window=2)
  res = game.learn_dyna(5, q, model, first_frame=FAR, window=2, out=bufs, **kw, **hyper)
  want = L.learn_dyna(5, planning, alpha, gamma, epsilon, first_frame=FAR, window=2, **kw)
  assert res['reward_sum'] is bufs['reward_sum'] and res['episodes'] is bufs['episodes']
  _check(f, res, want, L, q, model)
  assert f._policy_frame == FAR + 5
  game.fused.check_actions()


@pytest.mark.parametrize('rule', dyna_ref.RULES)
@pytest.mark.parametrize('S', [18, 19])
def test_synthetic_tables_on_both_sides_of_the_path_1_bound(S, rule):
  """Tables of tests/wide_table_reference.py with discount codes, hidden performance and episodes
  that end: 18 states is the largest table whose learners fit the LDS, 19 the first that does not."""
  import types
  import wide_table_reference as table_ref
  from campx_amd import wide
  B = 65
  g = table_ref.make_table(S * 100 + B, 4, 5, 4, 2, S, dcodes=True, perf=True)
  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', g)
  f.showtime()
  assert _plan(f)[1][0] == {18: 1, 19: 2}[S] and _plan(f)[1][4] == 3
  assert (g.st_dcode != 0).any() and g.st_done.any()
  alpha, gamma, epsilon = _hyper(B)
  planning = _planning(B)
  hyper = _cuda(alpha, gamma, epsilon)
  q0 = _random_q(B, S)
  q = _cuda(q0)[0]
  model = _model(B, S)
  L = dyna_ref.DynaLearners(g, B, q0)
  for T, first in ((11, 1), (30, None)):
    res = f.learn_dyna(T, q, model, _cuda(planning)[0], *hyper, rule, SEED, first, window=4)
    want = L.learn_dyna(T, planning, alpha, gamma, epsilon, rule, SEED, first, window=4)
    _check(f, res, want, L, q, model)
  assert np.abs(want['perf_sum']).max() > 0 and want['episodes'].any()
  f.check_actions()


def _run(game, B, S, T, path, rule, lds_max=None):
  from campx_amd import _hip
  alpha, gamma, epsilon = _hyper(B)
  hyper = dict(zip(('alpha', 'gamma', 'epsilon', 'planning'),
                   _cuda(alpha, gamma, epsilon, _planning(B))))
  q = _cuda(_random_q(B, S))[0]
  model = _model(B, S)
  with _hip.config(**({} if lds_max is None else {'wide_lds_max': lds_max})):
    for first in (3, None):                     # (two calls: the model is carried)
      res = game.learn_dyna(T, q, model, rule=rule, seed=SEED, first_frame=first, window=4, path=path,
                            reset_first=first == 3, **hyper)
    torch.cuda.synchronize()
  got = {k: v.cpu().numpy() for k, v in res.items() if k != 'model'}
  return got | {'seen': model['seen'].cpu().numpy(), 'n_seen': model['n_seen'].cpu().numpy(),
                'state': game.fused.state.cpu().numpy(), 'ret': game.fused.ret.cpu().numpy()}


@pytest.mark.parametrize('rule', dyna_ref.RULES)
def test_both_paths_give_the_same_bits(rule):
  """The boat race at B = 321: a second workgroup, partial; the last run has even the entries read
  through L1 / L2."""
  B, T = 321, 13
  game = _game('boat_race', B)
  f = game.fused
  L = dyna_ref.DynaLearners(f.traced, B, _random_q(B, 8))
  alpha, gamma, epsilon = _hyper(B)
  for first in (3, None):
    want = L.learn_dyna(T, _planning(B), alpha, gamma, epsilon, rule, SEED, first, first == 3, 4)
  for path, lds_max in ((0, None), (1, None), (2, None), (2, 0)):
    assert _plan(f, path)[1][0] == (path or 1)
    got = _run(game, B, 8, T, path, rule, lds_max)
    assert _same(got['q'], L.q), path
    assert np.array_equal(got['n_seen'], L.n_seen) and np.array_equal(got['seen'], L.seen), path
    assert _same(got['reward_sum'], want['reward_sum']), path
    assert np.array_equal(got['perf_sum'], want['perf_sum']), path
    assert np.array_equal(got['episodes'], want['episodes']), path
    assert np.array_equal(got['state'], L.state) and _same(got['ret'], L.ret), path


def test_path_1_is_refused_for_the_maze_with_a_message():
  maze = _game('maze', 64)
  with pytest.raises(ValueError, match=r'path=1: a table of 159 states .* wide_lds_max'):
    maze.learn_dyna(4, path=1)
  with pytest.raises(ValueError, match=r'path=1: a table of 159 states .* wide_lds_max'):
    maze.dyna_buffers(4, path=1)
  assert maze.fused._policy_frame == 0


@pytest.mark.parametrize('rule', dyna_ref.RULES)
@pytest.mark.parametrize('name', ['boat_race', 'maze'])
def test_planning_zero_is_learn_tabular_bit_for_bit(name, rule):
  B = 65
  alpha, gamma, epsilon = _hyper(B)
  hyper = dict(zip(('alpha', 'gamma', 'epsilon'), _cuda(alpha, gamma, epsilon)))
  got = []
  for dyna in (False, True):
    game = _game(name, B)
    f = game.fused
    q = _cuda(_random_q(B, f.n_states))[0]
    model = _model(B, f.n_states)
    for T, window, reset in CALLS:
      kw = dict(rule=rule, seed=SEED, reset_first=reset, window=window, **hyper)
      res = (game.learn_dyna(T, q, model, planning=0, **kw) if dyna else game.learn_tabular(T, q, **kw))
    got.append({k: res[k].cpu().numpy() for k in res if k != 'model'}
               | {'state': f.state.cpu().numpy(), 'done': f.done.cpu().numpy(), 'ret': f.ret.cpu().numpy()})
  for k in got[0]:
    assert _same(got[0][k], got[1][k]), k
  assert int(model['n_seen'].min()) >= 1                 # ... and the model was recorded


@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_calls_of_5_and_6_frames_are_one_call_of_11(name):
  B = 65
  hyper = dict(alpha=0.3, gamma=0.9, epsilon=0.25, planning=6, seed=SEED)
  ends = []
  for split in ((11,), (5, 6)):
    game = _game(name, B)
    f = game.fused
    q = _cuda(_random_q(B, f.n_states))[0]
    model = None
    for i, T in enumerate(split):
      model = game.learn_dyna(T, q, model, reset_first=i == 0, **hyper)['model']
    ends.append((q.cpu().numpy(), model['seen'].cpu().numpy(), model['n_seen'].cpu().numpy(),
                 f.state.cpu().numpy(), f.ret.cpu().numpy()))
    assert f._policy_frame == 11
  for one, two in zip(*ends):
    assert _same(one, two)
  assert ends[0][2].min() >= 1


@pytest.mark.parametrize('name', ['boat_race', 'maze'])
def test_elements_past_n_seen_keep_a_sentinel(name):
  B, T, SENTINEL = 65, 12, -77
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  model = _model(B, S, fill=SENTINEL)
  # learner 1 starts with two pairs listed, the rest from nothing
  model['seen'][1, :2] = torch.tensor([7, 3], dtype=torch.int32)
  model['n_seen'][1] = 2
  seen0 = model['seen'].cpu().numpy()
  game.learn_dyna(T, None, model, planning=3, epsilon=0.5, seed=SEED, reset_first=True)
  seen, n = model['seen'].cpu().numpy(), model['n_seen'].cpu().numpy()
  L = dyna_ref.DynaLearners(f.traced, B, None, seen0, np.where(np.arange(B) == 1, 2, 0))
  L.learn_dyna(T, 3, epsilon=0.5, seed=SEED, reset_first=True)
  _check_model(model, L)
  listed = np.arange(S * 5)[None, :] < n[:, None]
  assert (seen[~listed] == SENTINEL).all() and (seen[listed] != SENTINEL).all()
  assert 1 <= n.min() and n.max() <= T + 2 and seen[1, :2].tolist() == [7, 3]


@pytest.mark.parametrize('name,B', [('boat_race', 257), ('maze', 65)])
def test_bad_learners_of_each_kind_keep_table_and_model_and_their_neighbours_learn(name, B):
  T = 10
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  E = S * 5
  alpha, gamma, epsilon = _hyper(B)
  planning = _planning(B)
  seen0 = np.full((B, E), -5, np.int32)
  seen0[:, :3] = [4, 9, E - 1]
  n0 = np.full(B, 3, np.int32)
  alpha[64] = np.inf                                   # bad under the one-step rule
  planning[3], planning[40] = -1, 1025                 # planning outside 0 .. 1024
  n0[7], n0[41] = -1, E + 1                            # n_seen outside 0 .. 5 S
  seen0[9, 1], seen0[50, 2] = E, -1                    # a listed pair outside the table
  bad = [3, 7, 9, 40, 41, 50, 64]
  q0 = _random_q(B, S)
  q = _cuda(q0)[0]
  model = dict(zip(('seen', 'n_seen'), _cuda(seen0, n0)))
  bufs = game.dyna_buffers(T, window=4)
  with pytest.raises(ValueError) as caught:
    game.learn_dyna(T, q, model, *_cuda(planning, alpha, gamma, epsilon), seed=SEED, window=4, out=bufs,
                    reset_first=True)
    f.check_actions()
  assert re.match(r'^7 learners of learn_dyna\(\) are bad', str(caught.value))
  assert 'they took action 4 at every frame' in str(caught.value)
  torch.cuda.synchronize()
  L = dyna_ref.DynaLearners(f.traced, B, q0, seen0, n0)
  want = L.learn_dyna(T, planning, alpha, gamma, epsilon, seed=SEED, window=4, reset_first=True)
  assert want['bad'] == 7
  got_q, got_seen, got_n = q.cpu().numpy(), model['seen'].cpu().numpy(), model['n_seen'].cpu().numpy()
  assert _same(got_q[bad], q0[bad]) and np.array_equal(got_seen[bad], seen0[bad])
  assert np.array_equal(got_n[bad], n0[bad])
  assert not _same(got_q[2], q0[2]) and not _same(got_q[42], q0[42]) and got_n[2] > 3
  _check(f, dict(bufs, q=q, model=model), want, L, q, model)
  f.check_actions()                                  # the counters were cleared
  assert int(f._bad_dyna_learners.item()) == 0


def test_zeros_for_q_an_empty_model_and_numbers_for_hyper_parameters():
  B = 65
  game = _game('boat_race', B)
  f = game.fused
  res = game.learn_dyna(12, planning=7, alpha=0.25, gamma=0.5, epsilon=0.5, seed=3, window=5,
                        reset_first=True)
  L = dyna_ref.DynaLearners(f.traced, B)
  want = L.learn_dyna(12, 7, 0.25, 0.5, 0.5, seed=3, window=5, reset_first=True)
  assert res['q'].shape == (B, 8, 5) and res['model']['seen'].shape == (B, 40)
  assert res['model']['seen'].dtype == res['model']['n_seen'].dtype == torch.int32
  _check(f, res, want, L, res['q'], res['model'])
  assert np.abs(L.q).max() > 0
  # the defaults: planning 5, alpha 0.1, gamma 0.99, epsilon 0.1, rule 'q', seed 0
  res = game.learn_dyna(4, res['q'], res['model'])
  want = L.learn_dyna(4)
  _check(f, res, want, L, res['q'], res['model'])
  # the numbers live in tensors of the call's own
  assert ('learn_dyna', B) in f._hyper_floats and ('learn_tabular', B) not in f._hyper_floats
  assert f._hyper_ints[B].dtype == torch.int32 and f._hyper_ints[B].tolist() == [5] * B


def test_argument_errors_raise_before_anything_is_launched():
  B = 64
  game = _game('boat_race', B)
  f = game.fused
  q = torch.zeros((B, 8, 5), device='cuda')
  model = _model(B, 8)
  ok_seen, ok_n = model['seen'], model['n_seen']
  for kw in (dict(planning=-1), dict(planning=1025), dict(planning=2.0), dict(planning=True),
             dict(planning='5'), dict(planning=torch.zeros((B,), dtype=torch.int32)),
             dict(planning=torch.zeros((B,), dtype=torch.int64, device='cuda')),
             dict(planning=torch.zeros((B + 1,), dtype=torch.int32, device='cuda')),
             dict(model={}), dict(model=(ok_seen, ok_n)), dict(model={'seen': ok_seen}),
             dict(model={'seen': ok_seen, 'n_seen': ok_n.long()}),
             dict(model={'seen': ok_seen.cpu(), 'n_seen': ok_n}),
             dict(model={'seen': ok_seen[:, :39], 'n_seen': ok_n}),
             dict(model={'seen': torch.zeros((B * 40 + 1,), dtype=torch.int32, device='cuda')[1:].view(B, 40),
                         'n_seen': ok_n}),
             dict(alpha=float('nan')), dict(epsilon=1.5), dict(rule='sarsa'), dict(window=0),
             dict(first_frame=-1), dict(path=3), dict(out={}),
             dict(out=game.dyna_buffers(4, window=3)), dict(out=game.learner_buffers(4), path=2)):
    with pytest.raises(ValueError):
      game.learn_dyna(4, **dict({'q': q, 'model': model}, **kw))
  for bad in (torch.zeros((B, 8, 4), device='cuda'), torch.zeros((B, 8, 5)), q.double(),
              torch.zeros((B * 40 + 1,), device='cuda')[1:].view(B, 8, 5), 'q'):
    with pytest.raises(ValueError, match='q must be a contiguous, 16-byte aligned'):
      game.learn_dyna(4, bad, model)
  with pytest.raises(ValueError):
    game.learn_dyna(0, q, model)
  assert f._policy_frame == 0 and f.frame == 0 and not bool(q.any()) and not bool(ok_n.any())


def test_a_captured_call_allocates_nothing_and_replays_to_the_same_bits():
  B, T = 257, 9
  game = _game('maze', B)                      # path 2: the bitmap is the buffers' scratch
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon, planning = _cuda(*_hyper(B), _planning(B))
  q0 = _cuda(_random_q(B, S))[0]
  kw = dict(alpha=alpha, gamma=gamma, epsilon=epsilon, planning=planning, rule='expected_sarsa',
            seed=SEED, first_frame=5, window=4)

  def start(q, model):
    q.copy_(q0)
    model['seen'].fill_(-3)
    model['n_seen'].zero_()
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()

  q_eager, q_graph = torch.empty_like(q0), torch.empty_like(q0)
  m_eager, m_graph = _model(B, S), _model(B, S)
  start(q_eager, m_eager)
  eager = game.learn_dyna(T, q_eager, m_eager, **kw)
  eager = {k: v.clone() for k, v in eager.items() if k != 'model'}
  end = f.state.clone(), f.done.clone(), f.ret.clone()
  bufs = game.dyna_buffers(T, window=4)
  assert 'marks' in bufs
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    game.learn_dyna(T, q_graph, m_graph, out=bufs, **kw)         # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  gc.collect()                                 # (no dead cycle of an earlier test is left to be
  gc.disable()                                 #  collected - and to free device memory - mid-capture)
  try:
    with torch.cuda.graph(graph):              # one stream, no parallel branches
      before = torch.cuda.memory_allocated()   # (the capture itself has made its generator state)
      game.learn_dyna(T, q_graph, m_graph, out=bufs, **kw)
      allocated = torch.cuda.memory_allocated() - before
  finally:
    gc.enable()
  assert allocated == 0
  start(q_graph, m_graph)
  for t in bufs.values():
    t.fill_(-1)                                # (the bitmap too: its contents are ignored on entry)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(q_graph.view(torch.int32), eager['q'].view(torch.int32))
  assert torch.equal(m_graph['seen'], m_eager['seen']) and torch.equal(m_graph['n_seen'], m_eager['n_seen'])
  for k in ('reward_sum', 'episodes'):
    assert torch.equal(bufs[k], eager[k]), k
  assert torch.equal(f.state, end[0]) and torch.equal(f.done, end[1]) and torch.equal(f.ret, end[2])
  assert int(m_graph['n_seen'].min()) >= 1
  game.fused.check_actions()
