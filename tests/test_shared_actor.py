"""Shared actor-critic learners on the GPU: `WideGame.learn_actor_critic_shared()` (csrc/k_learn.hip,
`campx::wide_learn_actor_shared`) against tests/shared_actor_reference.py - a numpy walk of the
game's state table under the rule of include/campx_hip.h - bit for bit: prefs, values, the window
tensors, clamped, the bad-row count, state, done, ret.

The games are test_policy_rollout.py's: boat_race (8 states, hidden performance), maze (159
states), pickups (470 states, episodes that end).  T is at most 23 frames per call and B at most
2 048, as in tests/test_shared_learner.py, whose shapes and call sequence these are."""

import ctypes
import re

import numpy as np
import pytest
import torch

import shared_actor_reference as sa_ref
from float_edges import same_bits_or_nan
from test_policy_rollout import _game, _same
from test_shared_learner import CALLS, FAR, SEED, SHAPES, _cuda, _synthetic

pytestmark = pytest.mark.gpu

GAMES = ['boat_race', 'maze', 'pickups']


def _hyper(P):
  """Per-learner alpha_actor, alpha_critic, gamma: 0 and 1 among each."""
  m = np.arange(P)
  alpha_actor = np.array([0.5, 1.0, 0.1, 0.0], np.float32)[m % 4]
  alpha_critic = np.array([0.3, 1.0, 0.1, 0.0, 0.75], np.float32)[m % 5]
  gamma = np.array([0.9, 1.0, 0.5, 0.0, 0.99, 0.7, 0.8], np.float32)[m % 7]
  return alpha_actor, alpha_critic, gamma


def _random_tables(P, S, seed=0):
  rng = np.random.RandomState(seed + P + S)
  return (rng.uniform(-2, 2, size=(P, S, 5)).astype(np.float32),
          rng.uniform(-1, 1, size=(P, S)).astype(np.float32))


def _plan(f, P, path=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 6)()
  code = _hip.lib.campx_wide_actor_shared_plan(f.n_states, int(f.has_perf), f.batch, P,
                                               _hip.config_get('wide_lds_max'), path, plan)
  return code, list(plan)


def _check(f, res, want, L, prefs, values, same=_same):
  assert res['prefs'] is prefs and same(prefs.cpu().numpy(), L.prefs), 'prefs'
  assert res['values'] is values and same(values.cpu().numpy(), L.values), 'values'
  assert 'q' not in res
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


@pytest.mark.parametrize('n,P', SHAPES)
@pytest.mark.parametrize('name', GAMES)
def test_shared_actor_critics_against_the_reference_walk(name, n, P):
  B = n * P
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  hyper_np = _hyper(P)
  hyper = dict(zip(('alpha_actor', 'alpha_critic', 'gamma'), _cuda(hyper_np)))
  prefs0, values0 = _random_tables(P, S)
  prefs, values = _cuda((prefs0, values0))
  L = sa_ref.SharedActorCritics(f.traced, B, prefs0, values0)
  frame, bad_rows = 0, 0
  for T, window, reset in CALLS:
    res = game.learn_actor_critic_shared(T, prefs, values, seed=SEED, reset_first=reset, window=window,
                                         **hyper)
    want = L.learn(T, *hyper_np, seed=SEED, reset_first=reset, window=window)
    W = 1 if window is None else (T + window - 1) // window
    assert res['reward_sum'].shape == (W, B) and res['episodes'].shape == (W, B)
    assert res['clamped'].shape == (P,)
    _check(f, res, want, L, prefs, values)
    frame += T
    bad_rows += want['bad_rows']
    assert f._policy_frame == frame == L.frame and f.frame == frame
  assert want['bad'] == 0 and not _same(L.prefs, prefs0) and not _same(L.values, values0)
  # an explicit first_frame: inside a chunk, the high counter word in use; into buffers made once
  bufs = game.shared_actor_buffers(P, 5, window=2)
  res = game.learn_actor_critic_shared(5, prefs, values, seed=SEED, first_frame=FAR, window=2, out=bufs,
                                       **hyper)
  want = L.learn(5, *hyper_np, seed=SEED, first_frame=FAR, window=2)
  assert res['reward_sum'] is bufs['reward_sum'] and res['clamped'] is bufs['clamped']
  _check(f, res, want, L, prefs, values)
  assert f._policy_frame == FAR + 5 and bad_rows + want['bad_rows'] == 0
  f.check_actions()
  assert int(f._bad_shared_actor_rows.item()) == 0 and int(f._bad_shared_actor_learners.item()) == 0


@pytest.mark.parametrize('n', [256, 1024])
def test_every_actor_of_a_learner_in_one_bin(n):
  """`reset_first`, and the reset state's row has one preference 200 above the rest: the others
  get weight +0 by the rule's cut, so in frame 0 all n actors of a learner take action 1 - n adds
  on one accumulator, one owner."""
  P, B = 2, 2 * n
  game = _game('boat_race', B)
  f = game.fused
  g = f.traced
  prefs0, values0 = _random_tables(P, g.n_states)
  prefs0[:, 0] = [0.0, 200.0, 0.0, 0.0, 0.0]
  prefs, values = _cuda((prefs0, values0))
  kw = dict(alpha_actor=0.5, alpha_critic=0.5, gamma=0.5, seed=SEED)
  res = game.learn_actor_critic_shared(1, prefs, values, reset_first=True, **kw)
  L = sa_ref.SharedActorCritics(g, B, prefs0, values0)
  want = L.learn(1, reset_first=True, record=True, **kw)
  assert (want['actions'] == 1).all() and len(set(want['delta'][0, :n].tolist())) == 1
  _check(f, res, want, L, prefs, values)
  got = values.cpu().numpy()
  moved = got != values0
  assert moved[:, 0].all() and not moved[:, 1:].any()
  # pi = (0, 1, 0, 0, 0) and every visitor took action 1: mean_1 - 1 * mean_all = 0
  assert _same(prefs.cpu().numpy(), prefs0)
  res = game.learn_actor_critic_shared(3, prefs, values, **kw)
  want = L.learn(3, **kw)
  _check(f, res, want, L, prefs, values)
  f.check_actions()


def _run_paths(f, g, P, T, settings):
  """The same call on a fresh start under each (path, wide_lds_max) of `settings`; the scratch of
  the runs that have one is all zero afterwards."""
  from campx_amd import _hip
  B, S = f.batch, f.n_states
  hyper_np = _hyper(P)
  hyper = _cuda(hyper_np)
  prefs0, values0 = _random_tables(P, S)
  got, with_scratch = [], 0
  for path, lds_max in settings:
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()
    prefs, values = _cuda((prefs0, values0))
    with _hip.config(**({} if lds_max is None else {'wide_lds_max': lds_max})):
      scratch = None
      for first, frames in ((3, T - 5), (None, 5)):      # two calls: what the first leaves in scratch
        bufs = f.shared_actor_buffers(P, frames, window=4, path=path)
        if scratch is not None:
          bufs['scratch'] = scratch
        scratch = bufs.get('scratch')
        res = f.learn_actor_critic_shared(frames, prefs, values, *hyper, seed=SEED, first_frame=first,
                                          window=4, out=bufs, path=path)
        if 'scratch' in bufs:
          assert not bool(bufs['scratch'].any()), (path, lds_max)
      torch.cuda.synchronize()
    with_scratch += 'scratch' in bufs
    got.append({k: v.cpu().numpy() for k, v in res.items()}
               | {'state': f.state.cpu().numpy(), 'ret': f.ret.cpu().numpy()})
  L = sa_ref.SharedActorCritics(g, B, prefs0, values0)
  L.learn(T - 5, *hyper_np, seed=SEED, first_frame=3, window=4)
  want = L.learn(5, *hyper_np, seed=SEED, window=4)
  assert _same(got[0]['prefs'], L.prefs) and _same(got[0]['values'], L.values)
  assert not _same(L.prefs, prefs0) and _same(got[0]['reward_sum'], want['reward_sum'])
  assert np.array_equal(got[0]['clamped'], want['clamped'])
  assert np.array_equal(got[0]['perf_sum'], want['perf_sum']) and np.array_equal(got[0]['state'], L.state)
  for other in got[1:]:
    for k in got[0]:
      assert _same(got[0][k], other[k]), k
  return with_scratch


@pytest.mark.parametrize('n,P', [(3, 86), (256, 2)])
def test_both_paths_give_the_same_bits_on_the_boat_race(n, P):
  """LDS (path 1), global with the entries in LDS (path 2), and - with the library told that
  nothing fits - entries and all through L1 / L2; a smaller LDS gives path 1 another G."""
  game = _game('boat_race', n * P)
  f = game.fused
  assert _plan(f, P)[1][0] == 1
  settings = ((1, None), (2, None), (2, 0), (0, 0), (1, 368 + 2 * 544))
  assert _run_paths(f, f.traced, P, 20, settings) == 3
  f.check_actions()


@pytest.mark.parametrize('n,P', [(3, 86), (256, 2)])
def test_both_paths_give_the_same_bits_on_a_table_with_discount_codes(n, P):
  g, f = _synthetic(28, n * P)
  assert (g.st_dcode != 0).any() and f.has_perf and _plan(f, P)[1][0] == 1
  assert _run_paths(f, g, P, 20, ((1, None), (2, None), (0, 0))) == 2
  f.check_actions()


@pytest.mark.parametrize('n,P,held', [(1, 1, None), (3, 1, None), (8, 1, None), (1, 64, 3)])
def test_workgroups_of_fewer_than_16_threads_on_a_table_with_discount_codes(n, P, held):
  """A workgroup has G * n threads, down to one: fewer than the 16 discounts it stages.  One
  learner of 1, 3 and 8 actors on either path, and 64 learners of one actor with an LDS that holds
  3 of them on path 1.  The walk meets entries whose discount code is not below the number of
  threads - the elements a fill by `tid < 16` would leave unwritten."""
  from campx_amd import _hip
  B, T = n * P, 20
  g, f = _synthetic(28, B)
  table, per = 1120 + 144, 28 * 68               # entries and perf bytes; a learner's 68 bytes a state
  lds = None if held is None else table + held * per
  with _hip.config(**({} if lds is None else {'wide_lds_max': lds})):
    code, plan = _plan(f, P, path=1)
  threads = n * (held or 1)
  assert code == 0 and plan[:3] == [1, held or 1, threads] and threads < 16
  L = sa_ref.SharedActorCritics(g, B, *_random_tables(P, 28))
  walk = L.learn(T - 5, *_hyper(P), seed=SEED, first_frame=3, record=True)
  met = g.st_dcode[walk['states'], walk['actions'].astype(np.int64)]
  assert met.max() >= threads, (met.max(), threads)
  settings = ((1, lds), (2, lds)) if held else ((1, None), (2, None), (2, 0))
  _run_paths(f, g, P, T, settings)
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
    assert _hip.lib.campx_wide_actor_shared_plan(S, 1, B, P, lds_max, 0, plan) == 0
    if plan[0] == 2:
      break
    S += 1
  assert S > 28
  g, f = _synthetic(S, B)
  assert _plan(f, P)[1][0] == 2
  forced = _plan(f, P, path=1)[0] == 0
  _run_paths(f, g, P, 12, ((0, None),) + (((1, None),) if forced else ()))
  if not forced:
    with pytest.raises(ValueError, match='path=1: a table of {} states'.format(S)):
      f.learn_actor_critic_shared(4, torch.zeros((P, S, 5), device='cuda'),
                                  torch.zeros((P, S), device='cuda'), path=1)
  f.check_actions()


@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_step_sizes_zero_are_rollout_population_on_the_softmax_weights(name):
  """The states, done, ret and window sums of `rollout_population(softmax_weights(prefs), T)` from
  the same seed and frame; prefs and values are unchanged."""
  from campx_amd import returns
  n, P, T, window, first = 16, 5, 23, 4, 6
  B = n * P
  game = _game(name, B)
  f = game.fused
  prefs0, values0 = _random_tables(P, f.n_states, seed=9)
  prefs0[1, :, 2] = -np.inf
  prefs, values = _cuda((prefs0, values0))
  res = game.learn_actor_critic_shared(T, prefs, values, 0.0, 0.0, 0.9, seed=SEED, first_frame=first,
                                       reset_first=True, window=window)
  end = f.state.cpu().numpy(), f.done.cpu().numpy(), f.ret.cpu().numpy()
  assert _same(prefs.cpu().numpy(), prefs0) and _same(values.cpu().numpy(), values0)
  assert not bool(res['clamped'].any())
  out = game.rollout_population(returns.softmax_weights(prefs), T, seed=SEED, first_frame=first,
                                reset_first=True)
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
  f.check_actions()


def test_clamped_errors_are_counted_exactly():
  """values of +-1e30 in states that get visited: learner 0 in every state, with alternating sign;
  learner 1 in the start state alone; learner 2 has a NaN there; learner 3 an ordinary critic."""
  n, P, T = 64, 4, 12
  game = _game('boat_race', n * P)
  f = game.fused
  S = f.n_states
  prefs0, values0 = _random_tables(P, S)
  values0[0, 0::2], values0[0, 1::2] = 1e30, -1e30
  values0[1, 0] = -1e30
  values0[2, 0] = np.nan
  prefs, values = _cuda((prefs0, values0))
  L = sa_ref.SharedActorCritics(f.traced, n * P, prefs0, values0)
  kw = dict(alpha_actor=0.5, alpha_critic=0.5, gamma=0.9, seed=SEED, window=5)
  res = game.learn_actor_critic_shared(T, prefs, values, reset_first=True, **kw)
  want = L.learn(T, reset_first=True, **kw)
  assert (want['clamped'][:3] > 0).all() and want['clamped'][3] == 0 and want['bad_rows'] == 0
  _check(f, res, want, L, prefs, values, same=same_bits_or_nan)
  # 'clamped' is written, not added to
  res = game.learn_actor_critic_shared(2, prefs, values, **kw)
  want = L.learn(2, **kw)
  _check(f, res, want, L, prefs, values, same=same_bits_or_nan)
  f.check_actions()


@pytest.mark.parametrize('which,value', [('alpha_actor', np.nan), ('alpha_critic', -np.inf),
                                         ('gamma', np.inf)])
def test_bad_learners_and_bad_rows_among_good_ones(which, value):
  """Learners 1 and 85 (alone in the last workgroup) have a bad hyper-parameter; the start state's
  row - which action 4 of the boat race leads back to - has a NaN for learner 2 and a +inf for
  learner 3, and learner 1's NaN row is a bad learner's: not counted."""
  n, P, T = 3, 86, 10
  B = n * P
  bad, bad_row = [1, 85], [2, 3]
  names = ('alpha_actor', 'alpha_critic', 'gamma')
  h = dict(zip(names, _hyper(P)))
  h[which][bad] = value
  game = _game('boat_race', B)
  f = game.fused
  g = f.traced
  assert g.st_next[0, 4] == 0 and not g.st_done[0, 4]
  prefs0, values0 = _random_tables(P, 8)
  prefs0[2, 0, 3], prefs0[3, 0, 0], prefs0[1, 0, 1] = np.nan, np.inf, np.nan
  prefs, values = _cuda((prefs0, values0))
  bufs = game.shared_actor_buffers(P, T, window=4)
  with pytest.raises(ValueError) as caught:
    game.learn_actor_critic_shared(T, prefs, values, *_cuda([h[k] for k in names]), seed=SEED,
                                   reset_first=True, window=4, out=bufs)
    f.check_actions()
  text = str(caught.value)
  assert re.search(r'(^|; )2 learners of learn_actor_critic_shared\(\) have bad hyper-parameters', text)
  assert re.search(r'(^|; ){} environment-frames of learn_actor_critic_shared\(\) met rows of '
                   'preferences that are not good'.format(2 * n * T), text)
  assert 'took action 4' in text
  torch.cuda.synchronize()
  L = sa_ref.SharedActorCritics(g, B, prefs0, values0)
  want = L.learn(T, *[h[k] for k in names], seed=SEED, reset_first=True, window=4, record=True)
  assert want['bad'] == 2 and want['bad_rows'] == 2 * n * T
  lanes = [e for m in bad + bad_row for e in range(m * n, (m + 1) * n)]
  assert (want['actions'][:, lanes] == 4).all()
  got_prefs, got_values = prefs.cpu().numpy(), values.cpu().numpy()
  still = bad + bad_row
  assert same_bits_or_nan(got_prefs[still], prefs0[still]) and _same(got_values[still], values0[still])
  assert not _same(got_prefs[4], prefs0[4]) and not _same(got_values[4], values0[4])
  assert not bool(bufs['clamped'][still].any())
  _check(f, dict(bufs, prefs=prefs, values=values), want, L, prefs, values, same=same_bits_or_nan)
  f.check_actions()                        # the counters were cleared
  assert int(f._bad_shared_actor_learners.item()) == 0 and int(f._bad_shared_actor_rows.item()) == 0


def test_numbers_for_the_hyper_parameters_behave_as_tensors_of_the_same_value():
  n, P, T = 16, 4, 12
  B = n * P
  prefs0, values0 = _random_tables(P, 8)
  runs = []
  for numbers in (True, False):
    game = _game('boat_race', B)
    prefs, values = _cuda((prefs0, values0))
    hyper = (0.25, 0.5, 0.75) if numbers else tuple(torch.full((P,), v, device='cuda') for v in (0.25, 0.5, 0.75))
    res = game.learn_actor_critic_shared(T, prefs, values, *hyper, seed=3, window=5, reset_first=True)
    runs.append((game.fused, res, prefs, values))
  L = sa_ref.SharedActorCritics(runs[0][0].traced, B, prefs0, values0)
  want = L.learn(T, 0.25, 0.5, 0.75, seed=3, window=5, reset_first=True)
  for f, res, prefs, values in runs:
    _check(f, res, want, L, prefs, values)
  # the defaults: step sizes 0.1, gamma 0.99, seed 0, one window
  f, res, prefs, values = runs[0]
  res = f.learn_actor_critic_shared(4, prefs, values)
  want = L.learn(4, 0.1, 0.1, 0.99)
  _check(f, res, want, L, prefs, values)


def test_argument_errors_raise_before_anything_is_launched():
  B, P = 64, 4
  game = _game('boat_race', B)
  f = game.fused
  prefs = torch.zeros((P, 8, 5), device='cuda')
  values = torch.zeros((P, 8), device='cuda')
  f.state.fill_(3)
  for kw in (dict(alpha_actor=float('nan')), dict(gamma=float('inf')), dict(alpha_critic=float('-inf')),
             dict(alpha_actor='0.1'), dict(alpha_actor=torch.zeros((P,))),
             dict(alpha_critic=torch.zeros((P + 1,), device='cuda')),
             dict(alpha_critic=torch.zeros((B,), device='cuda')),
             dict(gamma=torch.zeros((P,), dtype=torch.float64, device='cuda')),
             dict(window=0), dict(window=2.5), dict(first_frame=-1), dict(path=3),
             dict(out={}), dict(out=game.shared_actor_buffers(P, 4, window=3)),
             dict(out=game.shared_actor_buffers(2, 4)), dict(out=game.learner_buffers(4)),
             dict(out=game.shared_actor_buffers(P, 4), path=2),           # no scratch in it
             dict(out=dict(game.shared_actor_buffers(P, 4),               # a short scratch
                           scratch=torch.zeros((11 * P * 8 - 1,), dtype=torch.int32, device='cuda')),
                  path=2)):
    with pytest.raises(ValueError):
      game.learn_actor_critic_shared(4, prefs, values, **kw)
  for bad in (None, torch.zeros((P, 8, 4), device='cuda'), torch.zeros((P, 8, 5)), prefs.double(),
              torch.zeros((8, 5), device='cuda'),
              torch.zeros((P * 40 + 1,), device='cuda')[1:].view(P, 8, 5), 'prefs'):
    with pytest.raises(ValueError, match='prefs must be a contiguous, 16-byte aligned'):
      game.learn_actor_critic_shared(4, bad, values)
  for bad in (None, torch.zeros((P, 7), device='cuda'), torch.zeros((P, 8)), values.double(),
              torch.zeros((P + 1, 8), device='cuda'),
              torch.zeros((P * 8 + 1,), device='cuda')[1:].view(P, 8), 'values'):
    with pytest.raises(ValueError, match='values must be a contiguous, 16-byte aligned'):
      game.learn_actor_critic_shared(4, prefs, bad)
  with pytest.raises(ValueError, match='do not split into P = 3 equal blocks'):
    game.learn_actor_critic_shared(4, torch.zeros((3, 8, 5), device='cuda'), torch.zeros((3, 8), device='cuda'))
  with pytest.raises(ValueError, match='do not split'):
    game.shared_actor_buffers(3, 4)
  big = _game('boat_race', 2050)
  with pytest.raises(ValueError, match='1025 environments per learner are more than one workgroup'):
    big.learn_actor_critic_shared(4, torch.zeros((2, 8, 5), device='cuda'), torch.zeros((2, 8), device='cuda'))
  assert big.fused._policy_frame == 0
  maze = _game('maze', 64)
  from campx_amd import _hip
  with _hip.config(wide_lds_max=6368 + 159 * 68 - 1):
    with pytest.raises(ValueError, match=r'path=1: a table of 159 states .* wide_lds_max'):
      maze.learn_actor_critic_shared(4, torch.zeros((4, 159, 5), device='cuda'),
                                     torch.zeros((4, 159), device='cuda'), path=1)
  assert maze.fused._policy_frame == 0
  with pytest.raises(ValueError):
    game.learn_actor_critic_shared(0, prefs, values)
  assert f._policy_frame == 0 and f.frame == 0 and not bool(prefs.any()) and not bool(values.any())
  assert bool((f.state == 3).all())
  bufs = game.shared_actor_buffers(P, 7, window=3)
  assert set(bufs) == {'reward_sum', 'perf_sum', 'episodes', 'clamped'}
  assert bufs['episodes'].shape == (3, B) and bufs['clamped'].shape == (P,)
  bufs = game.shared_actor_buffers(P, 7, window=3, path=2)
  assert bufs['scratch'].shape == (11 * P * 8,) and bufs['scratch'].dtype == torch.int32
  assert not bool(bufs['scratch'].any())


@pytest.mark.parametrize('path', [1, 2])
def test_a_captured_call_replays_to_the_same_bits(path):
  """... which, on path 2, also shows that the scratch is left zero: the replays start from what
  the warm-up and the capture's calls left in it."""
  n, P, T = 64, 5, 9
  B = n * P
  game = _game('boat_race', B)
  f = game.fused
  hyper = dict(zip(('alpha_actor', 'alpha_critic', 'gamma'), _cuda(_hyper(P))))
  prefs0, values0 = _cuda(_random_tables(P, 8))
  kw = dict(seed=SEED, first_frame=5, window=4, path=path, **hyper)

  def start(prefs, values):
    prefs.copy_(prefs0)
    values.copy_(values0)
    f.state.zero_()
    f.done.zero_()
    f.ret.zero_()

  p_eager, v_eager = torch.empty_like(prefs0), torch.empty_like(values0)
  p_graph, v_graph = torch.empty_like(prefs0), torch.empty_like(values0)
  start(p_eager, v_eager)
  eager = game.learn_actor_critic_shared(T, p_eager, v_eager, **kw)
  eager = {k: v.clone() for k, v in eager.items()}
  assert not torch.equal(eager['prefs'], prefs0)
  end = f.state.clone(), f.done.clone(), f.ret.clone()
  bufs = game.shared_actor_buffers(P, T, window=4, path=path)
  assert ('scratch' in bufs) == (path == 2)
  start(p_graph, v_graph)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    game.learn_actor_critic_shared(T, p_graph, v_graph, out=bufs, **kw)      # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                # one stream, no parallel branches
    game.learn_actor_critic_shared(T, p_graph, v_graph, out=bufs, **kw)
  for _ in range(2):
    start(p_graph, v_graph)
    for k, t in bufs.items():
      if k != 'scratch':
        t.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(p_graph.view(torch.int32), eager['prefs'].view(torch.int32))
    assert torch.equal(v_graph.view(torch.int32), eager['values'].view(torch.int32))
    for k in ('reward_sum', 'perf_sum', 'episodes', 'clamped'):
      assert torch.equal(bufs[k], eager[k]), k
    assert torch.equal(f.state, end[0]) and torch.equal(f.done, end[1]) and torch.equal(f.ret, end[2])
  if path == 2:
    assert not bool(bufs['scratch'].any())
  f.check_actions()
