"""Closed-loop rollouts of a population on the GPU: `WideGame.rollout_population()`
(csrc/k_policy.hip, `campx::wide_policy_population`) against tests/population_reference.py -
a host walk of the game's state table under P policies, byte for byte - and against
`rollout_policy()`, member by member.

The games are test_policy_rollout.py's (its docstring): boat_race (8 states, hidden performance,
LDS), maze (159 states), pickups (two planes, episodes that end), porter (5 044 states, the global
path).  The shapes (B, P): (1, 1); (64, 64), one policy per environment; (255, 3), a member
boundary inside a wave; (260, 4), n = 65, workgroups that span members; (512, 2), aligned; (771,
3), n = 257, a boundary that straddles a workgroup.  T = 19, then a continued call of T = 13:
no multiples of four, crossing a chunk of eight.
"""

import ctypes
import re

import numpy as np
import pytest
import torch

import policy_reference as ref
import population_reference as pop_ref
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

GAMES = ['boat_race', 'maze', 'pickups', 'porter']
SHAPES = [(1, 1), (64, 64), (255, 3), (260, 4), (512, 2), (771, 3)]
SEED = 0x1234567890abcdef
T1, T2 = 19, 13
STREAMS = ('actions', 'reward', 'discount', 'done', 'perf')

_POLICIES = {}


def _policies(name, P, S):
  """Random positive weights [P, S, 5], different per member; every fourth row has exact zeros,
  and rows are scaled by 1e-3 and 1e3 in turn.  Computed once per (game, P)."""
  if (name, P) not in _POLICIES:
    rng = np.random.RandomState(len(name) * 1000 + P * 10 + S % 7)
    w = rng.uniform(0.05, 1.0, size=(P * S, 5)).astype(np.float32)
    for s in range(0, P * S, 4):
      w[s, rng.choice(5, size=rng.randint(1, 5), replace=False)] = 0.0
    w[1::3] *= np.float32(1e-3)
    w[2::3] *= np.float32(1e3)
    _POLICIES[(name, P)] = w.reshape(P, S, 5)
  return _POLICIES[(name, P)]


def _plan(f, P, path=0):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_population_plan(f.n_states, int(f.has_perf), f.batch, P,
                                             _hip.config_get('wide_lds_max'), path, plan)
  return code, list(plan)


def _check_against_walk(f, out, want, walker, want_states=True):
  for k in STREAMS + (('states',) if want_states else ()):
    if out.get(k) is None:
      assert k in ('reward', 'perf') and not (f.any_reward if k == 'reward' else f.has_perf), k
      continue
    got = out[k].cpu().numpy()
    assert got.dtype == want[k].dtype, (k, got.dtype)
    assert _same(got, want[k]), k
  assert np.array_equal(f.state.cpu().numpy(), walker.state)
  assert np.array_equal(f.done.cpu().numpy(), walker.over.astype(np.uint8))
  assert _same(f.ret.cpu().numpy(), walker.ret)


def _snapshot(f):
  return f.state.clone(), f.done.clone(), f.ret.clone()


def _restore(f, snap):
  for t, s in zip((f.state, f.done, f.ret), snap):
    t.copy_(s)


def _equal_dicts(a, b, keys=STREAMS + ('states', 'trace')):
  for k in keys:
    if a.get(k) is None or b.get(k) is None:
      assert a.get(k) is None and b.get(k) is None, k
    else:
      assert a[k].shape == b[k].shape and a[k].stride() == b[k].stride(), k
      assert _same(a[k].cpu().numpy(), b[k].cpu().numpy()), k


@pytest.mark.parametrize('padded', [True, False], ids=['padded', 'unpadded'])
@pytest.mark.parametrize('B,P', SHAPES)
@pytest.mark.parametrize('name', GAMES)
def test_population_rollouts_against_the_reference_walk(name, B, P, padded, monkeypatch):
  from campx_amd import fused
  monkeypatch.setattr(fused, 'PAD_ROWS', padded)
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  w = _policies(name, P, S)
  policies = torch.from_numpy(w).cuda()
  walker = pop_ref.PopulationWalker(f.traced, B)
  for T, reset in ((T1, True), (T2, False)):
    out = game.rollout_population(policies, T, seed=SEED, reset_first=reset)
    want = walker.rollout(w, T, seed=SEED, reset_first=reset)
    assert out['actions'].shape == (T, B) and out['states'].shape == (T, B)
    assert out['states'].dtype == torch.int32 and out['trace'].shape == (f._n_planes, T, B)
    assert out['actions'].stride(0) == ((B + 15) // 16 * 16 if padded else B)
    assert out['states'].stride(0) == out['actions'].stride(0)
    _check_against_walk(f, out, want, walker)
    assert want['bad'] == 0
    # 'states' is the flat row: member * S + the game's state
    states = out['states'].cpu().numpy()
    assert np.array_equal(states // S, np.tile(pop_ref.members(B, P), (T, 1)))
  assert f._policy_frame == T1 + T2 and f.frame == T1 + T2
  # the streams are [T, P, n] by unflatten
  assert out['actions'].unflatten(1, (P, B // P)).shape == (T2, P, B // P)
  # without 'states', into buffers allocated once; a tensor that requires grad is detached
  bufs = game.rollout_population_buffers(7, want_states=False)
  assert 'states' not in bufs
  out = game.rollout_population(policies.clone().requires_grad_(), 7, seed=3, out=bufs, want_states=False)
  want = walker.rollout(w, 7, seed=3)
  assert out is bufs
  _check_against_walk(f, out, want, walker, want_states=False)
  f.check_actions()


@pytest.mark.parametrize('B,P', SHAPES)
@pytest.mark.parametrize('name', GAMES)
def test_population_rollouts_against_the_existing_kernel(name, B, P):
  """Member by member: `rollout_policy(policies[m])` on the same B from the same start equals the
  population's columns [m n, (m + 1) n) in every stream, trace included - 'states' differ by
  m S.  `rollout_trace()` of the sampled actions reproduces trace and scalars.  With P = 1 the
  whole dict is `rollout_policy()`'s, and so is the one after the continued call."""
  a, b = _game(name, B), _game(name, B)
  fa, fb = a.fused, b.fused
  S, n = fa.n_states, B // P
  policies = torch.from_numpy(_policies(name, P, S)).cuda()
  start, first = _snapshot(fa), 0
  for T, reset in ((T1, True), (T2, False)):
    out = a.rollout_population(policies, T, seed=SEED, reset_first=reset)
    end = _snapshot(fa)
    for m in range(P):
      _restore(fb, start)
      one = b.rollout_policy(policies[m], T, seed=SEED, first_frame=first, reset_first=reset)
      cols = slice(m * n, (m + 1) * n)
      if P == 1:
        _equal_dicts(out, one)
      for k in STREAMS + ('trace',):
        if one[k] is None:
          assert out[k] is None, k
        else:
          assert _same(out[k][..., cols].cpu().numpy(), one[k][..., cols].cpu().numpy()), (T, m, k)
      assert torch.equal(out['states'][:, cols], one['states'][:, cols] + m * S), (T, m)
      for got, want in zip(end, _snapshot(fb)):
        assert _same(got[cols].cpu().numpy(), want[cols].cpu().numpy()), (T, m)
    # the sampled actions through the open-loop kernel, from the same start
    _restore(fb, start)
    replay = b.rollout_trace(out['actions'].contiguous(), reset_first=reset)
    for k in ('trace', 'reward', 'discount', 'done', 'perf'):
      if replay[k] is None:
        assert out[k] is None, k
      else:
        assert _same(out[k].cpu().numpy(), replay[k].cpu().numpy()), (T, k)
    for got, want in zip(end, _snapshot(fb)):
      assert _same(got.cpu().numpy(), want.cpu().numpy()), T
    start, first = end, first + T
  fa.check_actions()
  fb.check_actions()


@pytest.mark.parametrize('path', [0, 2])
@pytest.mark.parametrize('name', ['boat_race', 'maze'])
def test_one_member_is_the_solo_call_at_a_real_shape(name, path):
  """P = 1 runs the instances without members through the population's entry point: B = 257 (a
  second workgroup of one lane), T = 11 from frame 3 (three skipped frames in front, a ragged last
  chunk).  Every stream, the trace, 'states', state, done and ret are `rollout_policy()`'s, byte
  for byte, on both paths; the plan stages one member."""
  B, T, first = 257, 11, 3
  a, b = _game(name, B), _game(name, B)
  fa, fb = a.fused, b.fused
  policy = torch.from_numpy(_policies(name, 1, fa.n_states)).cuda()
  code, plan = _plan(fa, 1, path)
  assert code == 0 and plan[0] == (path or 1) and plan[2:] == [256, 1]
  # a start that is not the reset: the same 5 frames on both games
  a.rollout_policy(policy[0], 5, seed=7, reset_first=True)
  b.rollout_policy(policy[0], 5, seed=7, reset_first=True)
  got = a.rollout_population(policy, T, seed=SEED, first_frame=first, path=path)
  want = b.rollout_policy(policy[0], T, seed=SEED, first_frame=first)
  _equal_dicts(got, want)
  for x, y in zip(_snapshot(fa), _snapshot(fb)):
    assert _same(x.cpu().numpy(), y.cpu().numpy())
  assert fa._policy_frame == fb._policy_frame == first + T
  fa.check_actions()
  fb.check_actions()


@pytest.mark.parametrize('B,P', SHAPES)
@pytest.mark.parametrize('name', GAMES)
def test_both_paths_agree_and_the_chosen_one_is_the_plans(name, B, P):
  from campx_amd import _hip
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  policies = torch.from_numpy(_policies(name, P, S)).cuda()
  code, plan = _plan(f, P)
  members = int((pop_ref.members(B, P)[np.minimum(np.arange(0, B, 256) + 255, B - 1)]
                 - pop_ref.members(B, P)[np.arange(0, B, 256)] + 1).max())
  need = ((40 * S + 15) // 16 * 16 + 16 * S + ((5 * S + 15) // 16 * 16 if f.has_perf else 0)
          + members * S * 20)
  fits = need <= _hip.config_get('wide_lds_max')
  assert code == 0 and plan == [1 if fits else 2, need if fits else 0, 256, members]
  assert fits == (name != 'porter' and not (name in ('maze', 'pickups') and P == 64)), (need, members)
  runs = {}
  for path in (0, 2) + ((1,) if fits else ()):
    runs[path] = game.rollout_population(policies, T1, seed=SEED, first_frame=2, reset_first=True, path=path)
    runs[path]['final'] = f.state.clone()
  for path in runs:
    _equal_dicts(runs[path], runs[0], keys=STREAMS + ('states', 'trace', 'final'))
  if not fits:
    frame = f._policy_frame
    with pytest.raises(ValueError, match=r'path=1: a table of \d+ states .* does not fit the LDS'):
      game.rollout_population(policies, T1, path=1)
    assert f._policy_frame == frame
    assert _plan(f, P, path=1)[0] != 0
  # the global path by the setting, as a user would force it for every call
  with _hip.config(wide_lds_max=0):
    assert _plan(f, P)[1][0] == 2
    out = game.rollout_population(policies, T1, seed=SEED, first_frame=2, reset_first=True)
  _equal_dicts(out, runs[0])
  f.check_actions()


@pytest.mark.parametrize('B,P', [(260, 4), (64, 64)])
@pytest.mark.parametrize('name', ['boat_race', 'pickups'])
def test_the_learners_chain_serves_all_members_in_one_launch_each(name, B, P):
  from campx_amd import returns
  game = _game(name, B)
  f = game.fused
  S = f.n_states
  w = _policies(name, P, S)
  policies = torch.from_numpy(w).cuda()
  out = game.rollout_population(policies, T1, seed=SEED, reset_first=True)
  states, actions = out['states'].cpu().numpy(), out['actions'].cpu().numpy()
  value = (out['states'] % 5).float() * 0.25 + 1.0            # exact in fixed point
  sums = returns.sum_by_state(out['states'], out['actions'], (value,), n_states=P * S)
  assert int(sums['skipped']) == 0 and int(sums['clamped']) == 0
  count, total = np.zeros((P, S, 5), np.int64), np.zeros((P, S, 5), np.float64)
  member = np.tile(pop_ref.members(B, P), (T1, 1))
  np.add.at(count, (member, states - member * S, actions), 1)
  np.add.at(total, (member, states - member * S, actions), (states % 5) * 0.25 + 1.0)
  assert np.array_equal(sums['count'].cpu().numpy().reshape(P, S, 5), count)
  assert np.array_equal(sums['sums'][0].cpu().numpy().reshape(P, S, 5), total)
  assert count.sum(axis=(1, 2)).tolist() == [T1 * (B // P)] * P
  looked = returns.table_lookup(policies.view(-1, 5), out['states'], out['actions'])
  assert _same(looked.cpu().numpy(), w.reshape(-1, 5)[states, actions])
  critic = torch.arange(P * S, dtype=torch.float32, device='cuda').view(P, S)
  assert torch.equal(critic.view(-1)[out['states'].long()], out['states'].float())
  assert f.ret.view(P, B // P).mean(1).shape == (P,)         # each member's mean episode return
  # the game's own state, for render_states()
  obs = game.render_states(out['states'][3] % S)
  assert obs.shape[0] == B
  f.check_actions()


@pytest.mark.parametrize('kind', ['nan', 'negative', 'all zero'])
@pytest.mark.parametrize('B,P', [(260, 4), (771, 3)])
def test_bad_rows_of_one_member_raise_lazily_with_their_count(B, P, kind):
  T = T1
  game = _game('boat_race', B)
  f = game.fused
  S, n = f.n_states, B // P
  w = _policies('boat_race', P, S).copy()
  rows = {'nan': [np.nan, 1, 1, 1, 1], 'negative': [1, 1, -0.25, 1, 1], 'all zero': [0, 0, 0, 0, 0]}
  w[1, 0] = rows[kind]
  w[1, 3] = rows[kind]
  walker = pop_ref.PopulationWalker(f.traced, B)
  want = walker.rollout(w, T, seed=9, reset_first=True)
  assert want['bad'] >= n and want['bad_by_member'].tolist() == [0, want['bad']] + [0] * (P - 2)
  bufs = game.rollout_population_buffers(T)
  with pytest.raises(ValueError, match='bad policy rows') as e:
    game.rollout_population(torch.from_numpy(w).cuda(), T, seed=9, reset_first=True, out=bufs)
    f.check_actions()
  count = int(re.match(r'(\d+) environment-frames of rollout_population\(\) met bad policy rows '
                       r'\(a weight that is negative or NaN, or a sum that is not a positive finite '
                       r'number\); they took action 4$', str(e.value)).group(1))
  assert count == want['bad']
  torch.cuda.synchronize()
  _check_against_walk(f, bufs, want, walker)
  states, actions = bufs['states'].cpu().numpy(), bufs['actions'].cpu().numpy()
  met = (states == S) | (states == S + 3)                  # member 1's rows 0 and 3
  assert met.sum() == count and (actions[met] == 4).all()
  assert not met[:, :n].any() and not met[:, 2 * n:].any()
  # cleared: nothing left to raise, and good policies raise nothing
  f.check_actions()
  assert int(f._bad_member_rows.item()) == 0 and int(f._bad_rows.item()) == 0
  assert int(f._bad_flag_view[0]) == 0
  game.rollout_population(torch.from_numpy(_policies('boat_race', P, S)).cuda(), T)
  f.check_actions()


def test_eager_errors_and_the_other_tiers():
  from campx_amd import fused
  from campx_amd.games import boat_race, hello_world, maze
  game = _game('boat_race', 64)
  f = game.fused
  S = f.n_states
  good = torch.ones((4, S, 5), device='cuda')
  expected = r'policies must be a contiguous float32 \[P, 8, 5\] tensor'
  for bad in (torch.ones((S, 5), device='cuda'), torch.ones((4, S + 1, 5), device='cuda'),
              torch.ones((4, S, 4), device='cuda'), torch.ones((0, S, 5), device='cuda'),
              torch.ones((4, S, 5), device='cuda', dtype=torch.float64),
              torch.ones((4, S, 5), device='cuda', dtype=torch.float16), torch.ones((4, S, 5)),
              torch.ones((4, 5, S), device='cuda').transpose(1, 2), np.ones((4, S, 5), np.float32)):
    with pytest.raises(ValueError, match=expected):
      game.rollout_population(bad, 4)
  for P in (3, 5, 128):
    with pytest.raises(ValueError, match='do not split into P = {} equal blocks'.format(P)):
      game.rollout_population(torch.ones((P, S, 5), device='cuda'), 4)
  with pytest.raises(ValueError, match='at least one frame'):
    game.rollout_population(good, 0)
  with pytest.raises(ValueError, match='first_frame'):
    game.rollout_population(good, 4, first_frame=-1)
  with pytest.raises(ValueError, match='path must be 0'):
    game.rollout_population(good, 4, path=3)
  for bad_out in (game.rollout_population_buffers(5), game.rollout_population_buffers(4, want_states=False),
                  _game('boat_race', 128).rollout_population_buffers(4), 'no dict'):
    with pytest.raises(ValueError, match='rollout_population_buffers'):
      game.rollout_population(good, 4, out=bad_out)
  assert f._policy_frame == 0 and f.frame == 0                # (nothing ran)
  # the two calls share one frame counter
  game.rollout_policy(torch.ones((S, 5), device='cuda'), 5)
  game.rollout_population(good, 6)
  assert f._policy_frame == 11
  # the other tiers refuse by name; an engine without a tier says so
  plain = boat_race.build(64, 'cuda')
  plain.its_showtime()
  assert type(plain.fused) is fused.FusedGame
  hello = hello_world.build(batch=16, device='cuda')
  hello.its_showtime()
  for engine in (plain, hello):
    for call in (lambda: engine.rollout_population(good, 4), lambda: engine.rollout_population_buffers(4)):
      with pytest.raises(NotImplementedError, match=r'^rollout_population(_buffers)?\(\) is offered by '
                                                    r'the state-table tier only'):
        call()
  with pytest.raises(RuntimeError, match=r'rollout_population\(\) needs a batched Engine'):
    maze.build(16, 16).rollout_population(good, 4)


def _op_args(f, policies, bufs, seed, first_frame, reset_first, path):
  return (f._spec_host, f._tables, f.state, f.done, f.ret, policies, seed, first_frame,
          bufs['reward'], bufs['discount'], bufs['done'], bufs['perf'], bufs['trace'],
          bufs['actions'], bufs.get('states'), f._bad_member_rows, None, reset_first, path)


def test_opcheck():
  f = _game('boat_race', 260).fused
  policies = torch.from_numpy(_policies('boat_race', 4, f.n_states)).cuda()
  bufs = f.rollout_population_buffers(9)
  for path in (0, 2):
    torch.library.opcheck(torch.ops.campx.wide_policy_population.default,
                          _op_args(f, policies, bufs, 5, 6, True, path))          # all four checks
  cpu = [x.cpu() if torch.is_tensor(x) else x for x in _op_args(f, policies, bufs, 5, 6, True, 0)]
  with pytest.raises((NotImplementedError, RuntimeError)):
    torch.ops.campx.wide_policy_population(*cpu)
  # the op checks what the Python call checks: a P that does not divide B
  with pytest.raises(RuntimeError, match='do not split'):
    torch.ops.campx.wide_policy_population(*_op_args(f, policies[:3].contiguous(), bufs, 5, 6, True, 0))


def test_capture_in_a_hip_graph_allocates_nothing_and_replays_the_same_bytes():
  B, P, T = 260, 4, T1
  game = _game('maze', B)
  f = game.fused
  f.validate_actions = False
  w = _policies('maze', P, f.n_states)
  policies = torch.from_numpy(w).cuda()
  bufs = game.rollout_population_buffers(T)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    game.rollout_population(policies, T, seed=21, first_frame=6, reset_first=True, out=bufs)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  before = torch.cuda.memory_stats()['allocation.all.allocated']
  game.rollout_population(policies, T, seed=21, first_frame=6, reset_first=True, out=bufs)
  assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    game.rollout_population(policies, T, seed=21, first_frame=6, reset_first=True, out=bufs)
  kept = []
  for _ in range(2):
    for k in ('actions', 'states', 'reward', 'trace'):
      bufs[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    kept.append({k: v.clone() for k, v in bufs.items() if v is not None})
    kept[-1]['state'] = f.state.clone()
  for k in kept[0]:
    assert _same(kept[0][k].cpu().numpy(), kept[1][k].cpu().numpy()), k
  walker = pop_ref.PopulationWalker(f.traced, B)
  want = walker.rollout(w, T, seed=21, first_frame=6, reset_first=True)
  _check_against_walk(f, bufs, want, walker)
