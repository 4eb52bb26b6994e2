"""Online tabular learners on the GPU: `WideGame.learn_tabular()` (csrc/k_learn.hip,
`campx::wide_learn`) against tests/learner_reference.py - a numpy walk of the game's state table
under the rule of include/campx_hip.h - bit for bit: q, the three window tensors, state, done, ret.

The games are test_policy_rollout.py's: boat_race (8 states, hidden performance: q in LDS), maze
(159 states: q through L1 / L2, the entries in LDS), pickups (470 states, episodes that end).
Hyper-parameters and tables are ordinary numbers; tests/test_float_edges.py runs the learners on
subnormals, signed zeros, infinities and NaN.
"""

import ctypes
import re

import numpy as np
import pytest
import torch

import learner_reference as learn_ref
import planning_reference as plan_ref
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

GAMES = ['boat_race', 'maze', 'pickups']
SEED = 0x1234567890abcdef
# (T, window, reset_first): the calls start at frames 0, 1, 3, 6 and 14 - both sides of the Philox
# pair and leads 0, 1, 3, 2 and 2 of the four-frame chunk; windows of 1, 3, T (None) and beyond T
CALLS = ((1, None, True), (2, 1, False), (3, 5, False), (8, 3, False), (9, 9, False))
FAR = (1 << 40) + 1


def _hyper(B):
  """Per-learner alpha, gamma, epsilon: epsilon 0 and 1 and alpha 0 and 1 among them, in every
  combination (the periods 4 and 5 are coprime)."""
  e = np.arange(B)
  alpha = np.array([0.0, 1.0, 0.1, 0.5], np.float32)[e % 4]
  epsilon = np.array([0.0, 1.0, 0.1, 0.3, 0.75], np.float32)[e % 5]
  gamma = np.array([0.9, 0.99, 0.5], np.float32)[e % 3]
  return alpha, gamma, epsilon


def _random_q(B, S, seed=0):
  return np.random.RandomState(seed + B + S).uniform(-1, 1, size=(B, S, 5)).astype(np.float32)


def _plan(f, path=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_learn_plan(f.n_states, int(f.has_perf), f.batch,
                                        _hip.config_get('wide_lds_max'), path, plan)
  return code, list(plan)


def _check(f, res, want, L, q):
  assert res['q'] is q and _same(q.cpu().numpy(), L.q), 'q'
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


def test_names_the_kernel_paths_the_games_take():
  paths = {name: _plan(_game(name, 1).fused) for name in GAMES}
  assert paths['boat_race'] == (0, [1, 320 + 48 + 40960, 256, 1])
  assert paths['maze'] == (0, [2, 6368, 256, 1]) and paths['pickups'] == (0, [2, 18800, 256, 1])


@pytest.mark.parametrize('rule', learn_ref.RULES)
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('name', GAMES)
def test_learners_against_the_reference_walk(name, B, rule):
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon = _hyper(B)
  hyper = dict(alpha=torch.from_numpy(alpha).cuda(), gamma=torch.from_numpy(gamma).cuda(),
               epsilon=torch.from_numpy(epsilon).cuda())
  q0 = _random_q(B, S)
  q = torch.from_numpy(q0).cuda()
  L = learn_ref.Learners(f.traced, B, q0)
  frame = 0
  for T, window, reset in CALLS:
    res = game.learn_tabular(T, q, rule=rule, seed=SEED, reset_first=reset, window=window, **hyper)
    want = L.learn(T, alpha, gamma, epsilon, rule=rule, seed=SEED, reset_first=reset, window=window)
    W = 1 if window is None else (T + window - 1) // window
    assert res['reward_sum'].shape == (W, B) and res['episodes'].shape == (W, B)
    _check(f, res, want, L, q)
    frame += T
    assert f._policy_frame == frame == L.frame and f.frame == frame
  assert want['bad'] == 0 and (B == 1 or not _same(L.q, q0))      # (learner 0 has alpha 0)
  # an explicit first_frame: inside a pair, the high counter word in use; into buffers made once
  bufs = game.learner_buffers(5, window=2)
  res = game.learn_tabular(5, q, rule=rule, seed=SEED, first_frame=FAR, window=2, out=bufs, **hyper)
  want = L.learn(5, alpha, gamma, epsilon, rule=rule, seed=SEED, first_frame=FAR, window=2)
  assert res['reward_sum'] is bufs['reward_sum'] and res['episodes'] is bufs['episodes']
  _check(f, res, want, L, q)
  assert f._policy_frame == FAR + 5
  game.fused.check_actions()


@pytest.mark.parametrize('rule', learn_ref.RULES)
@pytest.mark.parametrize('S,B', [(7, 3), (7, 257), (28, 65), (29, 65)])
def test_synthetic_tables_with_discount_codes(S, B, rule):
  """Tables of tests/wide_table_reference.py with discount codes and hidden performance.  Seven
  states: 35 floats per learner, so that a workgroup's piece of q is no multiple of four floats
  (the tail of the 16-byte copies) unless its learners are; 28 states: the largest table whose
  learners fit the LDS, 141 KiB of it; 29: the first that goes through L1 / L2."""
  import types
  import wide_table_reference as table_ref
  from campx_amd import wide
  g = table_ref.make_table(S * 100 + B, 4, 5, 4, 2, S, dcodes=True, perf=True)
  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', g)
  f.showtime()
  assert _plan(f)[1][0] == (1 if S <= 28 else 2) and (g.st_dcode != 0).any()
  alpha, gamma, epsilon = _hyper(B)
  q0 = _random_q(B, S)
  q = torch.from_numpy(q0).cuda()
  L = learn_ref.Learners(g, B, q0)
  for T, first in ((11, 1), (6, None)):
    res = f.learn_tabular(T, q, torch.from_numpy(alpha).cuda(), torch.from_numpy(gamma).cuda(),
                          torch.from_numpy(epsilon).cuda(), rule, SEED, first, window=4)
    want = L.learn(T, alpha, gamma, epsilon, rule, SEED, first, window=4)
    _check(f, res, want, L, q)
  assert np.abs(want['perf_sum']).max() > 0
  f.check_actions()


def test_numbers_for_hyper_parameters_and_zeros_for_q():
  B = 65
  game = _game('boat_race', B)
  f = game.fused
  res = game.learn_tabular(12, alpha=0.25, gamma=0.5, epsilon=0.5, seed=3, window=5, reset_first=True)
  L = learn_ref.Learners(f.traced, B)
  want = L.learn(12, 0.25, 0.5, 0.5, seed=3, window=5, reset_first=True)
  assert res['q'].shape == (B, 8, 5) and res['q'].dtype == torch.float32
  _check(f, res, want, L, res['q'])
  assert np.abs(L.q).max() > 0
  # the defaults: alpha 0.1, gamma 0.99, epsilon 0.1, rule 'q', seed 0, one window
  res = game.learn_tabular(4, res['q'])
  want = L.learn(4, 0.1, 0.99, 0.1)
  _check(f, res, want, L, res['q'])


@pytest.mark.parametrize('rule', learn_ref.RULES)
def test_both_paths_give_the_same_bits(rule):
  """The boat race: q in LDS (path 1), q through L1 / L2 with the entries in LDS (path 2), and -
  with the library told that nothing fits - entries and all through L1 / L2."""
  from campx_amd import _hip
  B, T = 257, 23
  alpha, gamma, epsilon = _hyper(B)
  hyper = dict(alpha=torch.from_numpy(alpha).cuda(), gamma=torch.from_numpy(gamma).cuda(),
               epsilon=torch.from_numpy(epsilon).cuda())
  got = []
  for path, lds_max in ((1, None), (2, None), (2, 0), (0, 0)):
    game = _game('boat_race', B)
    q = torch.from_numpy(_random_q(B, 8)).cuda()
    with _hip.config(**({} if lds_max is None else {'wide_lds_max': lds_max})):
      res = game.learn_tabular(T, q, rule=rule, seed=SEED, first_frame=3, window=4, path=path, **hyper)
      torch.cuda.synchronize()
    got.append({k: v.cpu().numpy() for k, v in res.items()}
               | {'state': game.fused.state.cpu().numpy(), 'ret': game.fused.ret.cpu().numpy()})
  L = learn_ref.Learners(game.fused.traced, B, _random_q(B, 8))
  want = L.learn(T, alpha, gamma, epsilon, rule=rule, seed=SEED, first_frame=3, window=4)
  assert _same(got[0]['q'], L.q) and _same(got[0]['reward_sum'], want['reward_sum'])
  for other in got[1:]:
    for k in got[0]:
      assert _same(got[0][k], other[k]), k


def test_path_1_is_refused_for_the_maze():
  game = _game('maze', 64)
  assert _plan(game.fused, path=1)[0] != 0
  with pytest.raises(ValueError, match='path=1: a table of 159 states with the Q-tables'):
    game.learn_tabular(4, path=1)
  assert game.fused._policy_frame == 0


@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_a_learner_that_does_not_learn_walks_what_rollout_policy_walks(name):
  """alpha = 0, epsilon = 0: the greedy policy of q, played.  The same from `rollout_policy()` with
  the one-hot greedy policy, from the same start."""
  B, T = 64, 37
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  row = np.random.RandomState(7).uniform(-1, 1, size=(S, 5)).astype(np.float32)
  q = torch.from_numpy(np.tile(row, (B, 1, 1))).cuda()
  res = game.learn_tabular(T, q, alpha=0.0, epsilon=0.0, seed=5, reset_first=True)
  assert _same(q.cpu().numpy(), np.tile(row, (B, 1, 1)))
  state, done, ret = f.state.clone(), f.done.clone(), f.ret.clone()
  policy = torch.nn.functional.one_hot(torch.from_numpy(plan_ref.reduce_greedy(row)[1].astype(np.int64)), 5)
  out = game.rollout_policy(policy.float().cuda(), T, seed=5, reset_first=True)
  assert torch.equal(f.state, state) and torch.equal(f.done, done)
  assert _same(f.ret.cpu().numpy(), ret.cpu().numpy())
  reward = out['reward'].cpu().numpy() if out['reward'] is not None else np.zeros((T, B), np.float32)
  total = np.zeros(B, np.float32)
  for t in range(T):
    total = (total + np.where(np.isnan(reward[t]), np.float32(0), reward[t])).astype(np.float32)
  assert _same(res['reward_sum'].cpu().numpy()[0], total)
  assert np.array_equal(res['episodes'].cpu().numpy()[0], out['done'].cpu().numpy().sum(0))
  if f.has_perf:
    assert np.array_equal(res['perf_sum'].cpu().numpy()[0], out['perf'].cpu().numpy().astype(np.int32).sum(0))


def test_bad_learners_are_counted_once_and_keep_their_tables():
  B, T = 257, 10
  game = _game('boat_race', B)
  f = game.fused
  alpha, gamma, epsilon = _hyper(B)
  alpha[3], epsilon[70], gamma[256] = np.nan, 1.5, np.inf
  q0 = _random_q(B, 8)
  q = torch.from_numpy(q0).cuda()
  bufs = game.learner_buffers(T, window=4)
  # (lazily: from the call itself when the flag is already up as it returns, else from the check)
  with pytest.raises(ValueError) as caught:
    game.learn_tabular(T, q, torch.from_numpy(alpha).cuda(), torch.from_numpy(gamma).cuda(),
                       torch.from_numpy(epsilon).cuda(), seed=SEED, window=4, out=bufs)
    f.check_actions()
  assert re.match(r'^3 learners of learn_tabular\(\) have bad hyper-parameters', str(caught.value))
  assert 'they took action 4 at every frame' in str(caught.value)
  torch.cuda.synchronize()
  L = learn_ref.Learners(f.traced, B, q0)
  want = L.learn(T, alpha, gamma, epsilon, seed=SEED, window=4)
  assert want['bad'] == 3
  got = q.cpu().numpy()
  assert _same(got[[3, 70, 256]], q0[[3, 70, 256]]) and not _same(got[5], q0[5])
  _check(f, dict(bufs, q=q), want, L, q)
  game.fused.check_actions()                         # the counters were cleared
  assert int(f._bad_learners.item()) == 0


def test_argument_errors_raise_before_anything_is_launched():
  B = 64
  game = _game('boat_race', B)
  f = game.fused
  q = torch.zeros((B, 8, 5), device='cuda')
  for kw in (dict(alpha=float('nan')), dict(gamma=float('inf')), dict(epsilon=1.5), dict(epsilon=-0.1),
             dict(alpha='0.1'), dict(alpha=torch.zeros((B,))), dict(epsilon=torch.zeros((B + 1,), device='cuda')),
             dict(gamma=torch.zeros((B,), dtype=torch.float64, device='cuda')), dict(rule='sarsa'),
             dict(window=0), dict(window=2.5), dict(first_frame=-1), dict(path=3),
             dict(out={}), dict(out=game.learner_buffers(4, window=3))):
    with pytest.raises(ValueError):
      game.learn_tabular(4, q, **kw)
  for bad_q in (torch.zeros((B, 8, 4), device='cuda'), torch.zeros((B, 8, 5)), q.double(),
                torch.zeros((B * 40 + 1,), device='cuda')[1:].view(B, 8, 5), 'q'):
    with pytest.raises(ValueError, match='q must be a contiguous, 16-byte aligned'):
      game.learn_tabular(4, bad_q)
  with pytest.raises(ValueError):
    game.learn_tabular(0, q)
  assert f._policy_frame == 0 and f.frame == 0 and not bool(q.any())
  assert set(game.learner_buffers(7, window=3)) == {'reward_sum', 'perf_sum', 'episodes'}
  assert game.learner_buffers(7, window=3)['episodes'].shape == (3, B)


def test_a_captured_call_replays_to_the_same_bits():
  B, T = 257, 9
  game = _game('boat_race', B)
  f = game.fused
  alpha, gamma, epsilon = (torch.from_numpy(x).cuda() for x in _hyper(B))
  q0 = torch.from_numpy(_random_q(B, 8)).cuda()
  kw = dict(alpha=alpha, gamma=gamma, epsilon=epsilon, rule='expected_sarsa', seed=SEED, first_frame=5,
            window=4)

  def start(q):
    q.copy_(q0)
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()

  q_eager, q_graph = torch.empty_like(q0), torch.empty_like(q0)
  start(q_eager)
  eager = game.learn_tabular(T, q_eager, **kw)
  eager = {k: v.clone() for k, v in eager.items()}
  end = f.state.clone(), f.done.clone(), f.ret.clone()
  bufs = game.learner_buffers(T, window=4)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    game.learn_tabular(T, q_graph, out=bufs, **kw)       # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                # one stream, no parallel branches
    game.learn_tabular(T, q_graph, out=bufs, **kw)
  start(q_graph)
  for t in bufs.values():
    t.fill_(-1)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(q_graph.view(torch.int32), eager['q'].view(torch.int32))
  for k in ('reward_sum', 'perf_sum', 'episodes'):
    assert torch.equal(bufs[k], eager[k]), k
  assert torch.equal(f.state, end[0]) and torch.equal(f.done, end[1]) and torch.equal(f.ret, end[2])
  game.fused.check_actions()
