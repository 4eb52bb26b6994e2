"""Shared online learners on the GPU: `WideGame.learn_shared()` (csrc/k_learn.hip,
`campx::wide_learn_shared`) against tests/shared_learner_reference.py - a numpy walk of the game's
state table under the rule of include/campx_hip.h - bit for bit: q, the window tensors, clamped,
state, done, ret.

The games are test_policy_rollout.py's: boat_race (8 states, hidden performance), maze (159
states), pickups (470 states, episodes that end).  T is at most 23 frames per call and B at most
2 048."""

import ctypes
import re
import types

import numpy as np
import pytest
import torch

import shared_learner_reference as shared_ref
from float_edges import same_bits_or_nan
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

GAMES = ['boat_race', 'maze', 'pickups']
SEED = 0x1234567890abcdef
# test_learner.py's: (T, window, reset_first); the calls start at frames 0, 1, 3, 6 and 14 - both
# sides of the Philox pair and leads 0, 1, 3, 2 and 2 of the four-frame chunk
CALLS = ((1, None, True), (2, 1, False), (3, 5, False), (8, 3, False), (9, 9, False))
FAR = (1 << 40) + 1
# (n, P): 257 learners of one actor - G = 256 or what fits, and a last workgroup of one learner;
# 85 learners = 255 threads, one idle lane, and a second workgroup with one learner; a short last
# workgroup with whole waves missing; a full 256-thread workgroup; the first size above 256
# threads, not a multiple of 64; the largest workgroup
SHAPES = [(1, 257), (3, 86), (64, 5), (256, 2), (257, 2), (1024, 2)]


def _hyper(P):
  """Per-learner alpha, gamma, epsilon: epsilon 0 and 1 and alpha 0 and 1 among them."""
  m = np.arange(P)
  alpha = np.array([0.5, 1.0, 0.1, 0.0], np.float32)[m % 4]
  epsilon = np.array([0.3, 1.0, 0.1, 0.0, 0.75], np.float32)[m % 5]
  gamma = np.array([0.9, 0.99, 0.5], np.float32)[m % 3]
  return alpha, gamma, epsilon


def _cuda(arrays):
  return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]


def _random_q(P, S, seed=0):
  return np.random.RandomState(seed + P + S).uniform(-1, 1, size=(P, S, 5)).astype(np.float32)


def _plan(f, P, path=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 6)()
  code = _hip.lib.campx_wide_shared_plan(f.n_states, int(f.has_perf), f.batch, P,
                                         _hip.config_get('wide_lds_max'), path, plan)
  return code, list(plan)


def _check(f, res, want, L, q, same=_same):
  assert res['q'] is q and same(q.cpu().numpy(), L.q), 'q'
  assert res['reward_sum'].dtype == torch.float32 and res['episodes'].dtype == torch.int32
  assert _same(res['reward_sum'].cpu().numpy(), want['reward_sum']), 'reward_sum'
  assert np.array_equal(res['episodes'].cpu().numpy(), want['episodes']), 'episodes'
  assert res['clamped'].dtype == torch.int64
  assert np.array_equal(res['clamped'].cpu().numpy(), want['clamped']), 'clamped'
  if f.has_perf:
    assert res['perf_sum'].dtype == torch.int32
    assert np.array_equal(res['perf_sum'].cpu().numpy(), want['perf_sum']), 'perf_sum'
  else:
    assert 'perf_sum' not in res
  assert np.array_equal(f.state.cpu().numpy(), L.state)
  assert np.array_equal(f.done.cpu().numpy(), L.over.astype(np.uint8))
  assert _same(f.ret.cpu().numpy(), L.ret)


def _synthetic(S, B, seed=None):
  import wide_table_reference as table_ref
  from campx_amd import wide
  g = table_ref.make_table(S * 100 + 7 if seed is None else seed, 4, 5, 4, 2, S, dcodes=True, perf=True)
  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', g)
  f.showtime()
  return g, f


@pytest.mark.parametrize('rule', shared_ref.RULES)
@pytest.mark.parametrize('n,P', SHAPES)
@pytest.mark.parametrize('name', GAMES)
def test_shared_learners_against_the_reference_walk(name, n, P, rule):
  B = n * P
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  alpha, gamma, epsilon = _hyper(P)
  ta, tg, te = _cuda((alpha, gamma, epsilon))
  hyper = dict(alpha=ta, gamma=tg, epsilon=te)
  q0 = _random_q(P, S)
  q = torch.from_numpy(q0).cuda()
  L = shared_ref.SharedLearners(f.traced, B, q0)
  frame = 0
  for T, window, reset in CALLS:
    res = game.learn_shared(T, q, rule=rule, seed=SEED, reset_first=reset, window=window, **hyper)
    want = L.learn(T, alpha, gamma, epsilon, rule=rule, seed=SEED, reset_first=reset, window=window)
    W = 1 if window is None else (T + window - 1) // window
    assert res['reward_sum'].shape == (W, B) and res['episodes'].shape == (W, B)
    assert res['clamped'].shape == (P,)
    _check(f, res, want, L, q)
    frame += T
    assert f._policy_frame == frame == L.frame and f.frame == frame
  assert want['bad'] == 0 and not _same(L.q, q0)
  # an explicit first_frame: inside a pair, the high counter word in use; into buffers made once
  bufs = game.shared_learner_buffers(P, 5, window=2)
  res = game.learn_shared(5, q, rule=rule, seed=SEED, first_frame=FAR, window=2, out=bufs, **hyper)
  want = L.learn(5, alpha, gamma, epsilon, rule=rule, seed=SEED, first_frame=FAR, window=2)
  assert res['reward_sum'] is bufs['reward_sum'] and res['clamped'] is bufs['clamped']
  _check(f, res, want, L, q)
  assert f._policy_frame == FAR + 5
  f.check_actions()


@pytest.mark.parametrize('n', [256, 1024])
def test_every_actor_of_a_learner_in_one_bin(n):
  """epsilon = 0, reset_first, equal rows: in frame 0 all n environments of learner 0 are in state
  0 and take the rows' greedy action 1 - n adds to one bin.  The step is alpha times the mean of n
  equal deltas: the delta itself, a multiple of 2^-32.  Learner 1, epsilon = 1, spreads over all
  five actions."""
  P, B = 2, 2 * n
  game = _game('boat_race', B)
  f = game.fused
  g = f.traced
  row = np.array([0.25, 0.5, 0.125, 0.0, -1.0], np.float32)
  q0 = np.tile(row, (P, g.n_states, 1))
  alpha, gamma = np.float32(0.5), np.float32(0.5)
  epsilon = np.array([0.0, 1.0], np.float32)
  r = np.float32(0.0 if np.isnan(g.st_reward[0, 1]) else g.st_reward[0, 1])
  target = r if g.st_done[0, 1] else np.float32(r + np.float32(gamma * g.st_discount[0, 1]) * np.float32(0.5))
  delta = np.float32(target - np.float32(0.5))
  assert delta != 0 and float(delta) * 2.0 ** 32 == round(float(delta) * 2.0 ** 32)
  q = torch.from_numpy(q0).cuda()
  te, = _cuda((epsilon,))
  res = game.learn_shared(1, q, alpha=0.5, gamma=0.5, epsilon=te, seed=SEED, reset_first=True)
  got = q.cpu().numpy()
  assert got[0, 0, 1] == np.float32(np.float32(0.5) + alpha * delta)
  moved = got != q0
  assert moved[0].sum() == 1 and not moved[1, 1:].any()
  L = shared_ref.SharedLearners(g, B, q0)
  want = L.learn(1, 0.5, 0.5, epsilon, seed=SEED, reset_first=True, record=True)
  assert (want['actions'][0, :n] == 1).all() and set(want['actions'][0, n:].tolist()) == {0, 1, 2, 3, 4}
  _check(f, res, want, L, q)
  res = game.learn_shared(3, q, alpha=0.5, gamma=0.5, epsilon=te, seed=SEED)
  want = L.learn(3, 0.5, 0.5, epsilon, seed=SEED)
  _check(f, res, want, L, q)
  f.check_actions()


def _run_paths(f, g, P, T, rule, settings):
  """The same call on a fresh start under each (path, wide_lds_max) of `settings`."""
  from campx_amd import _hip
  B, S = f.batch, f.n_states
  alpha, gamma, epsilon = _hyper(P)
  ta, tg, te = _cuda((alpha, gamma, epsilon))
  got = []
  for path, lds_max in settings:
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()
    q = torch.from_numpy(_random_q(P, S)).cuda()
    with _hip.config(**({} if lds_max is None else {'wide_lds_max': lds_max})):
      res = f.learn_shared(T, q, ta, tg, te, rule, SEED, 3, window=4, path=path)
      torch.cuda.synchronize()
    got.append({k: v.cpu().numpy() for k, v in res.items()}
               | {'state': f.state.cpu().numpy(), 'ret': f.ret.cpu().numpy()})
  L = shared_ref.SharedLearners(g, B, _random_q(P, S))
  want = L.learn(T, alpha, gamma, epsilon, rule=rule, seed=SEED, first_frame=3, window=4)
  assert _same(got[0]['q'], L.q) and _same(got[0]['reward_sum'], want['reward_sum'])
  assert np.array_equal(got[0]['clamped'], want['clamped'])
  assert np.array_equal(got[0]['perf_sum'], want['perf_sum']) and np.array_equal(got[0]['state'], L.state)
  for other in got[1:]:
    for k in got[0]:
      assert _same(got[0][k], other[k]), k


@pytest.mark.parametrize('rule', shared_ref.RULES)
@pytest.mark.parametrize('n,P', [(3, 86), (256, 2)])
def test_both_paths_give_the_same_bits_on_the_boat_race(n, P, rule):
  """LDS (path 1), global with the entries in LDS (path 2), and - with the library told that
  nothing fits - entries and all through L1 / L2; a smaller LDS gives path 1 another G."""
  game = _game('boat_race', n * P)
  f = game.fused
  assert _plan(f, P)[1][0] == 1
  _run_paths(f, f.traced, P, 20, rule, ((1, None), (2, None), (2, 0), (0, 0), (1, 368 + 2 * 640)))
  f.check_actions()


@pytest.mark.parametrize('n,P', [(3, 86), (256, 2)])
def test_both_paths_give_the_same_bits_on_a_table_with_discount_codes(n, P):
  g, f = _synthetic(28, n * P)
  assert (g.st_dcode != 0).any() and f.has_perf and _plan(f, P)[1][0] == 1
  _run_paths(f, g, P, 20, 'expected_sarsa', ((1, None), (2, None), (0, 0)))
  f.check_actions()


@pytest.mark.parametrize('n,P', [(3, 86), (256, 2)])
def test_the_smallest_table_the_plan_sends_to_path_2(n, P):
  """Found from the plan, not hard-coded; path 1 raises there when not even one learner fits, and
  otherwise gives the same bits."""
  from campx_amd import _hip
  B = n * P
  lds_max = _hip.config_get('wide_lds_max')
  plan = (ctypes.c_int64 * 6)()
  S = 1
  while True:
    assert _hip.lib.campx_wide_shared_plan(S, 1, B, P, lds_max, 0, plan) == 0
    if plan[0] == 2:
      break
    S += 1
  assert S > 28
  g, f = _synthetic(S, B)
  assert _plan(f, P)[1][0] == 2
  forced = _plan(f, P, path=1)[0] == 0
  _run_paths(f, g, P, 12, 'q', ((0, None),) + (((1, None),) if forced else ()))
  if not forced:
    with pytest.raises(ValueError, match='path=1: a table of {} states'.format(S)):
      f.learn_shared(4, torch.zeros((P, S, 5), device='cuda'), path=1)
  f.check_actions()


def test_clamped_errors_are_counted_exactly():
  """q0 with 1e30, +-Inf and NaN entries in rows that get visited (the start state's and its
  successors'): learners 0 .. 2; learner 3 has an ordinary table."""
  n, P, T = 64, 4, 12
  game = _game('boat_race', n * P)
  f = game.fused
  S = f.n_states
  q0 = _random_q(P, S)
  q0[0, :, 1::2] = 1e30
  q0[0, :, 0] = -1e30
  q0[1, :, 0], q0[1, :, 3] = np.inf, -np.inf
  q0[2, :, 2] = np.nan
  q0[2, 1::2, 0] = np.nan
  q = torch.from_numpy(q0).cuda()
  L = shared_ref.SharedLearners(f.traced, n * P, q0)
  kw = dict(alpha=0.5, gamma=0.9, epsilon=0.5, seed=SEED, window=5)
  res = game.learn_shared(T, q, reset_first=True, **kw)
  want = L.learn(T, reset_first=True, **kw)
  assert (want['clamped'][:3] > 0).all() and want['clamped'][3] == 0
  _check(f, res, want, L, q, same=same_bits_or_nan)
  # 'clamped' is written, not added to
  res = game.learn_shared(2, q, **kw)
  want = L.learn(2, **kw)
  _check(f, res, want, L, q, same=same_bits_or_nan)
  f.check_actions()


@pytest.mark.parametrize('which,value', [('alpha', np.nan), ('gamma', np.inf), ('epsilon', 1.5)])
def test_a_bad_learner_among_good_ones(which, value):
  n, P, T = 3, 86, 10
  B = n * P
  bad = 85                                 # alone in the last workgroup
  hyper = dict(zip(('alpha', 'gamma', 'epsilon'), _hyper(P)))
  q0 = _random_q(P, 8)

  def run(spoil):
    game = _game('boat_race', B)
    h = {k: v.copy() for k, v in hyper.items()}
    if spoil:
      h[which][bad] = value
      h[which][1] = value
    q = torch.from_numpy(q0).cuda()
    ta, tg, te = _cuda((h['alpha'], h['gamma'], h['epsilon']))
    bufs = game.shared_learner_buffers(P, T, window=4)
    if spoil:
      with pytest.raises(ValueError) as caught:
        game.learn_shared(T, q, ta, tg, te, seed=SEED, window=4, out=bufs)
        game.fused.check_actions()
      assert re.match(r'^2 learners of learn_shared\(\) have bad hyper-parameters', str(caught.value))
      assert 'took action 4 at every frame' in str(caught.value)
    else:
      game.learn_shared(T, q, ta, tg, te, seed=SEED, window=4, out=bufs)
    torch.cuda.synchronize()
    return game, h, q, bufs

  game, h, q, bufs = run(True)
  f = game.fused
  L = shared_ref.SharedLearners(f.traced, B, q0)
  want = L.learn(T, h['alpha'], h['gamma'], h['epsilon'], seed=SEED, window=4)
  assert want['bad'] == 2
  got = q.cpu().numpy()
  assert _same(got[[1, bad]], q0[[1, bad]]) and not _same(got[2], q0[2])
  _check(f, dict(bufs, q=q), want, L, q)
  f.check_actions()                        # the counters were cleared
  assert int(f._bad_shared_learners.item()) == 0
  # its environments walked action 4 from the start
  walk = np.zeros(n, np.int64)
  for _ in range(T):
    walk = np.where(f.traced.st_done[walk, 4] != 0, 0, f.traced.st_next[walk, 4])
  assert np.array_equal(np.where(L.over[bad * n:], 0, L.state[bad * n:]), walk)
  # the good learners' bits are those of a launch without it
  _, _, q_clean, _ = run(False)
  good = [m for m in range(P) if m not in (1, bad)]
  assert _same(got[good], q_clean.cpu().numpy()[good])


def test_numbers_for_the_hyper_parameters_behave_as_tensors_of_the_same_value():
  n, P, T = 16, 4, 12
  B = n * P
  runs = []
  for numbers in (True, False):
    game = _game('boat_race', B)
    q = torch.from_numpy(_random_q(P, 8)).cuda()
    hyper = (0.25, 0.5, 0.5) if numbers else tuple(torch.full((P,), v, device='cuda') for v in (0.25, 0.5, 0.5))
    res = game.learn_shared(T, q, *hyper, seed=3, window=5, reset_first=True)
    runs.append((game.fused, res, q))
  L = shared_ref.SharedLearners(runs[0][0].traced, B, _random_q(P, 8))
  want = L.learn(T, 0.25, 0.5, 0.5, seed=3, window=5, reset_first=True)
  for f, res, q in runs:
    _check(f, res, want, L, q)
  # the defaults: alpha 0.1, gamma 0.99, epsilon 0.1, rule 'q', seed 0, one window
  f, res, q = runs[0]
  res = f.learn_shared(4, q)
  want = L.learn(4, 0.1, 0.99, 0.1)
  _check(f, res, want, L, q)


def test_argument_errors_raise_before_anything_is_launched():
  B, P = 64, 4
  game = _game('boat_race', B)
  f = game.fused
  q = torch.zeros((P, 8, 5), device='cuda')
  f.state.fill_(3)
  for kw in (dict(alpha=float('nan')), dict(gamma=float('inf')), dict(epsilon=1.5), dict(epsilon=-0.1),
             dict(alpha='0.1'), dict(alpha=torch.zeros((P,))), dict(epsilon=torch.zeros((P + 1,), device='cuda')),
             dict(epsilon=torch.zeros((B,), device='cuda')),
             dict(gamma=torch.zeros((P,), dtype=torch.float64, device='cuda')), dict(rule='sarsa'),
             dict(window=0), dict(window=2.5), dict(first_frame=-1), dict(path=3),
             dict(out={}), dict(out=game.shared_learner_buffers(P, 4, window=3)),
             dict(out=game.shared_learner_buffers(2, 4)), dict(out=game.learner_buffers(4)),
             dict(out=game.shared_learner_buffers(P, 4), path=2)):          # no scratch in it
    with pytest.raises(ValueError):
      game.learn_shared(4, q, **kw)
  for bad_q in (None, torch.zeros((P, 8, 4), device='cuda'), torch.zeros((P, 8, 5)), q.double(),
                torch.zeros((8, 5), device='cuda'),
                torch.zeros((P * 40 + 1,), device='cuda')[1:].view(P, 8, 5), 'q'):
    with pytest.raises(ValueError, match='q must be a contiguous, 16-byte aligned'):
      game.learn_shared(4, bad_q)
  with pytest.raises(ValueError, match='do not split into P = 3 equal blocks'):
    game.learn_shared(4, torch.zeros((3, 8, 5), device='cuda'))
  with pytest.raises(ValueError, match='do not split'):
    game.shared_learner_buffers(3, 4)
  big = _game('boat_race', 2050)
  with pytest.raises(ValueError, match='1025 environments per learner are more than one workgroup'):
    big.learn_shared(4, torch.zeros((2, 8, 5), device='cuda'))
  assert big.fused._policy_frame == 0
  with pytest.raises(ValueError):
    game.learn_shared(0, q)
  assert f._policy_frame == 0 and f.frame == 0 and not bool(q.any()) and bool((f.state == 3).all())
  bufs = game.shared_learner_buffers(P, 7, window=3)
  assert set(bufs) == {'reward_sum', 'perf_sum', 'episodes', 'clamped'}
  assert bufs['episodes'].shape == (3, B) and bufs['clamped'].shape == (P,)
  bufs = game.shared_learner_buffers(P, 7, window=3, path=2)
  assert bufs['scratch'].shape == (3 * P * 40,) and bufs['scratch'].dtype == torch.int32


@pytest.mark.parametrize('path', [1, 2])
def test_a_captured_call_replays_to_the_same_bits(path):
  """... which, on path 2, also shows that the scratch is left zero: the replays start from what
  the warm-up and the capture's calls left in it."""
  n, P, T = 64, 5, 9
  B = n * P
  game = _game('boat_race', B)
  f = game.fused
  alpha, gamma, epsilon = _cuda(_hyper(P))
  q0 = torch.from_numpy(_random_q(P, 8)).cuda()
  kw = dict(alpha=alpha, gamma=gamma, epsilon=epsilon, rule='expected_sarsa', seed=SEED, first_frame=5,
            window=4, path=path)

  def start(q):
    q.copy_(q0)
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()

  q_eager, q_graph = torch.empty_like(q0), torch.empty_like(q0)
  start(q_eager)
  eager = game.learn_shared(T, q_eager, **kw)
  eager = {k: v.clone() for k, v in eager.items()}
  end = f.state.clone(), f.done.clone(), f.ret.clone()
  bufs = game.shared_learner_buffers(P, T, window=4, path=path)
  assert ('scratch' in bufs) == (path == 2)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    game.learn_shared(T, q_graph, out=bufs, **kw)         # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                # one stream, no parallel branches
    game.learn_shared(T, q_graph, out=bufs, **kw)
  for _ in range(2):
    start(q_graph)
    for k, t in bufs.items():
      if k != 'scratch':
        t.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(q_graph.view(torch.int32), eager['q'].view(torch.int32))
    for k in ('reward_sum', 'perf_sum', 'episodes', 'clamped'):
      assert torch.equal(bufs[k], eager[k]), k
    assert torch.equal(f.state, end[0]) and torch.equal(f.done, end[1]) and torch.equal(f.ret, end[2])
  if path == 2:
    assert not bool(bufs['scratch'].any())
  f.check_actions()


@pytest.mark.parametrize('rule,epsilon', [('q', 0.5), ('expected_sarsa', 0.5), ('expected_sarsa', 0.0)])
def test_one_actor_per_learner_gives_the_bits_of_learn_tabular(rule, epsilon):
  """The one place where both kernels of csrc/k_learn.hip run on the same input: B = P = 65 (n = 1;
  one short workgroup with absent lanes in either kernel), the integer-valued table of
  test_shared_learner_cpu.py with alpha = gamma = 0.5 and q0 = 0, T = 13 from frame 3 (a chunk with
  a lead and a tail) in windows of 4 (a short last window), each kernel on paths 1 and 2, and a
  second call with `reset_first`.  Each kernel gives the bits of its own reference, `clamped` is all
  zeros, and the window sums, state, done and ret are the same bits across the two kernels.

  q is the same bits across the kernels wherever the quantiser is exact - every delta a multiple
  of 2^-32, which the references show here: under 'q', and under 'expected_sarsa' with epsilon = 0,
  where the bootstrap is (1 * max) + (0 * mean).  Expected SARSA with epsilon = 0.5 rounds: its mean
  is a sum times float32(0.2), so the deltas have bits below 2^-32, the quantised step differs from
  the per-environment learner's by design, and the two REFERENCES disagree on q (asserted below) -
  there each kernel is held to its own.

  The table has 12 states: a workgroup's piece of q is 65 x 60 floats, a multiple of four (any piece
  of it is, 60 being one), so path 1 of learn_tabular() copies it in whole 16-byte groups here."""
  import learner_reference as learn_ref
  from campx_amd import _hip, wide
  from wide_table_reference import integer_table
  B = P = 65
  g = integer_table()
  S = g.n_states
  assert S == 12 and (B * S * 5) % 4 == 0
  kw = dict(alpha=0.5, gamma=0.5, epsilon=epsilon, rule=rule, seed=11, first_frame=3, window=4)
  T = 13

  # the references, once: [call] -> (outputs, q, state, over, ret)
  def walk(L):
    calls = []
    for reset in (False, True):
      L.q[:] = 0
      out = L.learn(T, reset_first=reset, record=True, **kw)
      calls.append((out, L.q.copy(), L.state.copy(), L.over.copy(), L.ret.copy()))
    return calls

  alone = walk(learn_ref.Learners(g, B))
  shared = walk(shared_ref.SharedLearners(g, B, np.zeros((P, S, 5), np.float32)))
  exact = all(np.array_equal(np.ldexp(out['delta'].astype(np.float64), 32),
                             np.rint(np.ldexp(out['delta'].astype(np.float64), 32))) for out, *_ in shared)
  assert exact == (rule == 'q' or epsilon == 0.0)
  for (a, aq, *a_end), (s, sq, *s_end) in zip(alone, shared):
    assert s['clamped'].tolist() == [0] * P and np.abs(aq).max() > 0
    assert _same(aq, sq) == exact
    assert _same(a['reward_sum'], s['reward_sum']) and np.array_equal(a['episodes'], s['episodes'])
    assert np.array_equal(a['perf_sum'], s['perf_sum'])
    assert np.array_equal(a_end[0], s_end[0]) and np.array_equal(a_end[1], s_end[1]) and _same(a_end[2], s_end[2])

  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', g)
  f.showtime()
  plan = (ctypes.c_int64 * 4)()
  for path in (1, 2):
    assert _hip.lib.campx_wide_learn_plan(S, 1, B, _hip.config_get('wide_lds_max'), path, plan) == 0
    assert plan[0] == path and _plan(f, P, path)[1][0] == path
  for method, want in (('learn_tabular', alone), ('learn_shared', shared)):
    for path in (1, 2):
      f.state.zero_()
      f.done.zero_()
      f.ret.zero_()
      for reset, (out, q_end, state, over, ret) in zip((False, True), want):
        q = torch.zeros((P, S, 5), device='cuda')
        res = getattr(f, method)(T, q, reset_first=reset, path=path, **kw)
        where = '{} path {} reset_first={}'.format(method, path, reset)
        assert _same(q.cpu().numpy(), q_end), where
        assert _same(res['reward_sum'].cpu().numpy(), out['reward_sum']), where
        assert np.array_equal(res['perf_sum'].cpu().numpy(), out['perf_sum']), where
        assert np.array_equal(res['episodes'].cpu().numpy(), out['episodes']), where
        assert np.array_equal(f.state.cpu().numpy(), state), where
        assert np.array_equal(f.done.cpu().numpy(), over.astype(np.uint8)), where
        assert _same(f.ret.cpu().numpy(), ret), where
        if method == 'learn_shared':
          assert not bool(res['clamped'].any()), where
  f.check_actions()
