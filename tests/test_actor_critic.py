"""Actor-critic online learners on the GPU: `WideGame.learn_actor_critic()` (csrc/k_learn.hip,
`campx::wide_learn_actor`) against tests/actor_critic_reference.py - a numpy walk of the game's state
table under the rule and the frame of include/campx_hip.h - bit for bit: prefs, values, the three
window tensors, state, done, ret; and against `rollout_population()` on `softmax_weights(prefs)`
for learners that do not learn.

The games are test_learner.py's: boat_race (8 states, hidden performance: both tables in LDS), maze
(159 states) and pickups (470 states, episodes that end), both through L1 / L2.
"""

import ctypes
import gc
import re

import numpy as np
import pytest
import torch

import actor_critic_reference as ac_ref
from test_learner import FAR, GAMES, SEED
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

T = 11


def _cuda(*arrays):
  return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _plan(f, path=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_actor_plan(f.n_states, int(f.has_perf), f.batch,
                                        _hip.config_get('wide_lds_max'), path, plan)
  return code, list(plan)


def _hyper(B):
  """Per-learner alpha_actor, alpha_critic, gamma: step sizes 0 and 1 among them, in every
  combination (the periods 4, 5 and 3 are coprime)."""
  e = np.arange(B)
  alpha_actor = np.array([0.5, 0.0, 1.0, 0.1], np.float32)[e % 4]
  alpha_critic = np.array([0.3, 1.0, 0.0, 0.1, 0.75], np.float32)[e % 5]
  gamma = np.array([0.9, 0.99, 0.5], np.float32)[e % 3]
  return alpha_actor, alpha_critic, gamma


def _random_tables(B, S, seed=0):
  """Preferences within +-3 - every fifth learner's within +-60, so that weights reach the cut and
  some are exactly 0 - and values within +-1."""
  rs = np.random.RandomState(seed + B + S)
  prefs = rs.uniform(-3, 3, size=(B, S, 5)).astype(np.float32)
  prefs[::5] *= np.float32(20)
  return prefs, rs.uniform(-1, 1, size=(B, S)).astype(np.float32)


def _check(f, res, want, L, prefs, values):
  assert res['prefs'] is prefs and res['values'] is values and 'q' not in res
  assert _same(prefs.cpu().numpy(), L.prefs), 'prefs'
  assert _same(values.cpu().numpy(), L.values), 'values'
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


def test_names_the_paths_the_games_take():
  paths = {name: _plan(_game(name, 1).fused) for name in GAMES}
  assert paths['boat_race'] == (0, [1, 320 + 48 + 49152, 256, 1])
  assert paths['maze'] == (0, [2, 6368, 256, 1]) and paths['pickups'] == (0, [2, 18800, 256, 1])


def test_softmax_weights_gives_the_same_bits_on_the_device():
  from campx_amd import returns
  from test_actor_critic_cpu import _rows_with_edges, _rule_inputs
  rows = _rows_with_edges()
  want = ac_ref.softmax_weights(rows)[0]
  assert _same(returns.softmax_weights(_cuda(rows)[0]).cpu().numpy(), want)
  d = _rule_inputs()[::7]
  wide = np.zeros((len(d), 5), np.float32)
  wide[:, 1] = d
  assert _same(returns.softmax_weights(_cuda(wide)[0]).cpu().numpy()[:, 1], ac_ref.weight_of(d))


@pytest.mark.parametrize('B', [1, 63, 65, 257])
@pytest.mark.parametrize('name', GAMES)
def test_learners_against_the_reference_walk(name, B):
  """Three calls: T = 11 with a window that does not divide it, from frame 0; 3 frames from frame
  11 (lead 3 of the four-frame chunk); 5 frames from an explicit first_frame with the high counter
  word in use, into buffers made once."""
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  alpha_actor, alpha_critic, gamma = _hyper(B)
  hyper = dict(zip(('alpha_actor', 'alpha_critic', 'gamma'), _cuda(alpha_actor, alpha_critic, gamma)))
  prefs0, values0 = _random_tables(B, S)
  prefs, values = _cuda(prefs0, values0)
  L = ac_ref.ActorCritics(f.traced, B, prefs0, values0)
  res = game.learn_actor_critic(T, prefs, values, seed=SEED, reset_first=True, window=4, **hyper)
  want = L.learn(T, alpha_actor, alpha_critic, gamma, seed=SEED, reset_first=True, window=4)
  assert res['reward_sum'].shape == (3, B) and res['episodes'].shape == (3, B)
  _check(f, res, want, L, prefs, values)
  assert f._policy_frame == T == L.frame and f.frame == T
  res = game.learn_actor_critic(3, prefs, values, seed=SEED, **hyper)
  want = L.learn(3, alpha_actor, alpha_critic, gamma, seed=SEED)
  assert res['reward_sum'].shape == (1, B)
  _check(f, res, want, L, prefs, values)
  bufs = game.learner_buffers(5, window=2)
  res = game.learn_actor_critic(5, prefs, values, seed=SEED, first_frame=FAR, window=2, out=bufs, **hyper)
  want = L.learn(5, alpha_actor, alpha_critic, gamma, seed=SEED, first_frame=FAR, window=2)
  assert res['reward_sum'] is bufs['reward_sum'] and res['episodes'] is bufs['episodes']
  _check(f, res, want, L, prefs, values)
  assert f._policy_frame == FAR + 5
  assert want['bad'] == 0 and want['bad_rows'] == 0 and (B == 1 or not _same(L.prefs, prefs0))
  game.fused.check_actions()


@pytest.mark.parametrize('S', [23, 24])
def test_synthetic_tables_on_both_sides_of_the_path_1_bound(S):
  """Tables of tests/wide_table_reference.py with discount codes, hidden performance and episodes
  that end: 23 states is the largest table whose learners fit the LDS, 24 the first that does not."""
  import types
  import wide_table_reference as table_ref
  from campx_amd import wide
  B = 65
  g = table_ref.make_table(S * 100 + B, 4, 5, 4, 2, S, dcodes=True, perf=True)
  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', g)
  f.showtime()
  assert _plan(f)[1][0] == {23: 1, 24: 2}[S]
  assert (g.st_dcode != 0).any() and g.st_done.any()
  alpha_actor, alpha_critic, gamma = _hyper(B)
  hyper = _cuda(alpha_actor, alpha_critic, gamma)
  prefs0, values0 = _random_tables(B, S)
  prefs, values = _cuda(prefs0, values0)
  L = ac_ref.ActorCritics(g, B, prefs0, values0)
  for frames, first in ((T, 1), (30, None)):
    res = f.learn_actor_critic(frames, prefs, values, *hyper, SEED, first, window=4)
    want = L.learn(frames, alpha_actor, alpha_critic, gamma, SEED, first, window=4)
    _check(f, res, want, L, prefs, values)
  assert np.abs(want['perf_sum']).max() > 0 and want['episodes'].any()
  f.check_actions()


def test_both_paths_give_the_same_bits():
  """The boat race at B = 321: a second workgroup, partial; the last run has even the entries read
  through L1 / L2."""
  from campx_amd import _hip
  B, frames = 321, 13
  game = _game('boat_race', B)
  f = game.fused
  alpha_actor, alpha_critic, gamma = _hyper(B)
  prefs0, values0 = _random_tables(B, 8)
  L = ac_ref.ActorCritics(f.traced, B, prefs0, values0)
  for first in (3, None):
    want = L.learn(frames, alpha_actor, alpha_critic, gamma, SEED, first, first == 3, 4)
  for path, lds_max in ((0, None), (1, None), (2, None), (2, 0)):
    assert _plan(f, path)[1][0] == (path or 1)
    prefs, values = _cuda(prefs0, values0)
    with _hip.config(**({} if lds_max is None else {'wide_lds_max': lds_max})):
      for first in (3, None):
        res = game.learn_actor_critic(frames, prefs, values, *_cuda(alpha_actor, alpha_critic, gamma),
                                      seed=SEED, first_frame=first, reset_first=first == 3, window=4,
                                      path=path)
      torch.cuda.synchronize()
    _check(f, res, want, L, prefs, values)


def test_path_1_is_refused_for_the_maze_with_a_message():
  maze = _game('maze', 64)
  with pytest.raises(ValueError, match=r'path=1: a table of 159 states .* wide_lds_max'):
    maze.learn_actor_critic(4, path=1)
  assert maze.fused._policy_frame == 0


@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_frozen_learners_are_rollout_population_on_their_weights(name):
  """alpha_actor = alpha_critic = 0: the window rows are `rollout_population(softmax_weights(prefs))`'s
  reward, perf and done summed per window in frame order in f32 - the same seed and first_frame,
  P = B - and the final state is equal: the new sampler path against code that predates it."""
  from campx_amd import returns
  B, window, first = 65, 4, 6
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  prefs0, values0 = _random_tables(B, S, seed=9)
  prefs, values = _cuda(prefs0, values0)
  res = game.learn_actor_critic(T, prefs, values, 0.0, 0.0, 0.9, seed=SEED, first_frame=first,
                                reset_first=True, window=window)
  end = f.state.cpu().numpy(), f.done.cpu().numpy(), f.ret.cpu().numpy()
  assert _same(prefs.cpu().numpy(), prefs0) and _same(values.cpu().numpy(), values0)
  weights = returns.softmax_weights(prefs)
  assert float(weights.min()) == 0.0                    # (some actions are never taken)
  out = game.rollout_population(weights, T, seed=SEED, first_frame=first, reset_first=True)
  reward = out['reward'].cpu().numpy()
  reward = np.where(np.isnan(reward), np.float32(0), reward).astype(np.float32)
  done = out['done'].cpu().numpy().astype(np.int32)
  W = (T + window - 1) // window
  reward_sum, episodes = np.zeros((W, B), np.float32), np.zeros((W, B), np.int32)
  perf_sum = np.zeros((W, B), np.int32)
  for t in range(T):
    reward_sum[t // window] = (reward_sum[t // window] + reward[t]).astype(np.float32)
    episodes[t // window] += done[t]
    if f.has_perf:
      perf_sum[t // window] += out['perf'][t].cpu().numpy().astype(np.int32)
  assert _same(res['reward_sum'].cpu().numpy(), reward_sum)
  assert np.array_equal(res['episodes'].cpu().numpy(), episodes)
  if f.has_perf:
    assert np.array_equal(res['perf_sum'].cpu().numpy(), perf_sum) and np.abs(perf_sum).max() > 0
  assert np.array_equal(f.state.cpu().numpy(), end[0]) and np.array_equal(f.done.cpu().numpy(), end[1])
  assert _same(f.ret.cpu().numpy(), end[2])
  assert len(np.unique(out['actions'].cpu().numpy())) == 5
  game.fused.check_actions()


@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_calls_of_5_and_6_frames_are_one_call_of_11(name):
  B = 65
  hyper = dict(alpha_actor=0.3, alpha_critic=0.25, gamma=0.9, seed=SEED)
  ends = []
  for split in ((11,), (5, 6)):
    game = _game(name, B)
    f = game.fused
    prefs, values = _cuda(*_random_tables(B, f.n_states))
    for i, frames in enumerate(split):
      game.learn_actor_critic(frames, prefs, values, reset_first=i == 0, **hyper)
    ends.append((prefs.cpu().numpy(), values.cpu().numpy(), f.state.cpu().numpy(), f.ret.cpu().numpy()))
    assert f._policy_frame == 11
  for one, two in zip(*ends):
    assert _same(one, two)


@pytest.mark.parametrize('name,B', [('boat_race', 257), ('maze', 65)])
def test_bad_rows_take_action_4_and_zero_weights_are_never_taken(name, B):
  """State 0 - where every learner starts, and where action 4 of both games leads back to - of
  learner 1 has a NaN, of learner 2 a +inf, of learner 64 five -inf; learner 3's has a spread wide
  enough for exact-zero weights."""
  frames = 12
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  g = f.traced
  assert g.st_next[0, 4] == 0 and not g.st_done[0, 4]
  prefs0, values0 = _random_tables(B, S)
  prefs0[1, 0, 3] = np.nan
  prefs0[2, 0, 0] = np.inf
  prefs0[64, 0] = -np.inf
  prefs0[3, :, 1] = -np.inf                              # action 1: weight 0 in every state
  prefs0[3, :, 2] -= np.float32(200)                     # action 2: below the cut
  bad = [1, 2, 64]
  prefs, values = _cuda(prefs0, values0)
  bufs = game.learner_buffers(frames, window=5)
  with pytest.raises(ValueError) as caught:
    game.learn_actor_critic(frames, prefs, values, 0.5, 0.5, 0.9, seed=SEED, reset_first=True, window=5,
                            out=bufs)
    f.check_actions()
  assert re.search(r'{} environment-frames of learn_actor_critic\(\) met rows of preferences that '
                   'are not good'.format(3 * frames), str(caught.value))
  assert 'they took action 4' in str(caught.value) and 'have bad hyper-parameters' not in str(caught.value)
  torch.cuda.synchronize()
  L = ac_ref.ActorCritics(g, B, prefs0, values0)
  want = L.learn(frames, 0.5, 0.5, 0.9, seed=SEED, reset_first=True, window=5, record=True)
  assert want['bad_rows'] == 3 * frames and want['bad'] == 0
  assert (want['actions'][:, bad] == 4).all() and not np.isin(want['actions'][:, 3], (1, 2)).any()
  got_prefs, got_values = prefs.cpu().numpy(), values.cpu().numpy()
  assert _same(got_prefs[bad], prefs0[bad]) and _same(got_values[bad], values0[bad])
  for e in (3, 4, 6, 63):                            # the neighbours learn
    assert not _same(got_prefs[e], prefs0[e]) and not _same(got_values[e], values0[e]), e
  assert (got_prefs[3, :, 1] == -np.inf).all()
  _check(f, dict(bufs, prefs=prefs, values=values), want, L, prefs, values)
  f.check_actions()                                  # the counters were cleared
  assert int(f._bad_actor_rows.item()) == 0 and int(f._bad_actor_learners.item()) == 0


def test_bad_hyper_parameters_of_each_kind_keep_both_tables_and_their_neighbours_learn():
  B, frames = 257, 10
  game = _game('boat_race', B)
  f = game.fused
  alpha_actor, alpha_critic, gamma = _hyper(B)
  alpha_actor[3], alpha_actor[64] = np.nan, np.inf
  alpha_critic[7], alpha_critic[200] = -np.inf, np.nan
  gamma[9], gamma[256] = np.inf, np.nan
  bad = [3, 7, 9, 64, 200, 256]
  prefs0, values0 = _random_tables(B, 8)
  prefs0[9, 0, 0] = np.nan                               # a bad learner's bad rows are not counted
  prefs, values = _cuda(prefs0, values0)
  with pytest.raises(ValueError) as caught:
    game.learn_actor_critic(frames, prefs, values, *_cuda(alpha_actor, alpha_critic, gamma), seed=SEED,
                            window=4, reset_first=True)
    f.check_actions()
  assert re.match(r'^6 learners of learn_actor_critic\(\) have bad hyper-parameters', str(caught.value))
  assert 'they took action 4 at every frame' in str(caught.value)
  assert 'environment-frames of learn_actor_critic' not in str(caught.value)
  torch.cuda.synchronize()
  L = ac_ref.ActorCritics(f.traced, B, prefs0, values0)
  want = L.learn(frames, alpha_actor, alpha_critic, gamma, seed=SEED, window=4, reset_first=True)
  assert want['bad'] == 6 and want['bad_rows'] == 0
  got_prefs, got_values = prefs.cpu().numpy(), values.cpu().numpy()
  assert _same(got_prefs[bad], prefs0[bad]) and _same(got_values[bad], values0[bad])
  assert not _same(got_prefs[4], prefs0[4]) and not _same(got_values[8], values0[8])
  assert _same(got_prefs, L.prefs) and _same(got_values, L.values)
  assert np.array_equal(f.state.cpu().numpy(), L.state) and _same(f.ret.cpu().numpy(), L.ret)
  f.check_actions()


def test_zeros_for_both_tables_and_numbers_for_hyper_parameters():
  B = 65
  game = _game('boat_race', B)
  f = game.fused
  res = game.learn_actor_critic(12, alpha_actor=0.25, alpha_critic=0.5, gamma=0.5, seed=3, window=5,
                                reset_first=True)
  L = ac_ref.ActorCritics(f.traced, B)
  want = L.learn(12, 0.25, 0.5, 0.5, seed=3, window=5, reset_first=True)
  assert res['prefs'].shape == (B, 8, 5) and res['values'].shape == (B, 8)
  _check(f, res, want, L, res['prefs'], res['values'])
  assert np.abs(L.prefs).max() > 0
  # the defaults: both step sizes 0.1, gamma 0.99, seed 0
  res = game.learn_actor_critic(4, res['prefs'], res['values'])
  want = L.learn(4)
  _check(f, res, want, L, res['prefs'], res['values'])
  # the numbers live in tensors of the call's own
  assert ('learn_actor_critic', B) in f._hyper_floats and ('learn_tabular', B) not in f._hyper_floats


def test_argument_errors_raise_before_anything_is_launched():
  B = 64
  game = _game('boat_race', B)
  f = game.fused
  prefs = torch.zeros((B, 8, 5), device='cuda')
  values = torch.zeros((B, 8), device='cuda')
  for kw in (dict(alpha_actor=float('nan')), dict(alpha_critic=float('inf')), dict(gamma='0.9'),
             dict(alpha_actor=True), dict(alpha_actor=torch.zeros((B,))),
             dict(alpha_critic=torch.zeros((B,), dtype=torch.float64, device='cuda')),
             dict(gamma=torch.zeros((B + 1,), device='cuda')),
             dict(values=torch.zeros((B, 8))), dict(values=torch.zeros((B, 8, 1), device='cuda')),
             dict(values=values.double()), dict(values='v'),
             dict(values=torch.zeros((B * 8 + 1,), device='cuda')[1:].view(B, 8)),
             dict(window=0), dict(window=2.0), dict(first_frame=-1), dict(path=3), dict(path=-1),
             dict(out={}), dict(out=game.learner_buffers(4, window=3))):
    with pytest.raises(ValueError):
      game.learn_actor_critic(4, **dict({'prefs': prefs, 'values': values}, **kw))
  for bad in (torch.zeros((B, 8, 4), device='cuda'), torch.zeros((B, 8, 5)), prefs.double(),
              torch.zeros((B * 40 + 1,), device='cuda')[1:].view(B, 8, 5), 'prefs'):
    with pytest.raises(ValueError, match='prefs must be a contiguous, 16-byte aligned'):
      game.learn_actor_critic(4, bad, values)
  with pytest.raises(ValueError):
    game.learn_actor_critic(0, prefs, values)
  with pytest.raises(TypeError):
    game.learn_actor_critic(4, prefs, values, epsilon=0.1)
  assert f._policy_frame == 0 and f.frame == 0 and not bool(prefs.any()) and not bool(values.any())


def test_a_captured_call_allocates_nothing_and_replays_to_the_same_bits():
  B, frames = 257, 9
  game = _game('maze', B)
  f = game.fused
  S = f.n_states
  alpha_actor, alpha_critic, gamma = _cuda(*_hyper(B))
  prefs0, values0 = _cuda(*_random_tables(B, S))
  kw = dict(alpha_actor=alpha_actor, alpha_critic=alpha_critic, gamma=gamma, seed=SEED, first_frame=5,
            window=4)

  def start(prefs, values):
    prefs.copy_(prefs0)
    values.copy_(values0)
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()

  p_eager, v_eager = torch.empty_like(prefs0), torch.empty_like(values0)
  p_graph, v_graph = torch.empty_like(prefs0), torch.empty_like(values0)
  start(p_eager, v_eager)
  eager = game.learn_actor_critic(frames, p_eager, v_eager, **kw)
  eager = {k: v.clone() for k, v in eager.items()}
  end = f.state.clone(), f.done.clone(), f.ret.clone()
  bufs = game.learner_buffers(frames, window=4)
  start(p_graph, v_graph)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    game.learn_actor_critic(frames, p_graph, v_graph, out=bufs, **kw)      # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  gc.collect()                                 # (no dead cycle of an earlier test is left to be
  gc.disable()                                 #  collected - and to free device memory - mid-capture)
  try:
    with torch.cuda.graph(graph):              # one stream, no parallel branches
      before = torch.cuda.memory_allocated()   # (the capture itself has made its generator state)
      game.learn_actor_critic(frames, p_graph, v_graph, out=bufs, **kw)
      allocated = torch.cuda.memory_allocated() - before
  finally:
    gc.enable()
  assert allocated == 0
  start(p_graph, v_graph)
  for t in bufs.values():
    t.fill_(-1)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(p_graph.view(torch.int32), eager['prefs'].view(torch.int32))
  assert torch.equal(v_graph.view(torch.int32), eager['values'].view(torch.int32))
  assert not torch.equal(p_graph, prefs0) and not torch.equal(v_graph, values0)
  for k in ('reward_sum', 'episodes'):
    assert torch.equal(bufs[k], eager[k]), k
  assert torch.equal(f.state, end[0]) and torch.equal(f.done, end[1]) and torch.equal(f.ret, end[2])
  game.fused.check_actions()
