"""`campx_wide_actor_shared_plan()` - pure host arithmetic - against the header's account of the
bytes, the refusals of `campx_wide_actor_shared_launch()` that are decided before a device is
touched, the op's schema, and the numpy shared actor-critic learners of
tests/shared_actor_reference.py against a frame worked by hand, their quantiser's edges, the
population walk of tests/population_reference.py and themselves in other orders and call
sequences.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import actor_critic_reference as actor_ref
import population_reference as pop_ref
import shared_actor_reference as sa_ref
from test_population_cpu import _Table, _same, _valid_spec
from wide_table_reference import integer_table

F = np.float32
LDS_MAX = 144 * 1024
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h
PER_STATE = 68                           # path 1: sums 40, prefs 20, value 4, visitors 4


def _plan(S, perf, B, P, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 6)()
  code = _hip.lib.campx_wide_actor_shared_plan(S, perf, B, P, lds_max, path, out)
  return code, list(out)


def _table_bytes(S, perf):
  up = lambda x: (x + 15) // 16 * 16
  return up(40 * S) + (up(5 * S) if perf else 0)


def _account(S, perf, B, P, lds_max=LDS_MAX, path=0):
  """The header's account, restated: [path, G, threads, LDS bytes, entries in LDS, copies], or
  None where path 1 is forced and not even one learner fits."""
  n = B // P
  table = _table_bytes(S, perf)
  most = min(P, 256 // n if n <= 256 else 1)
  held = min(most, (lds_max - table) // (S * PER_STATE)) if lds_max >= table else 0
  if path == 1 and held < 1:
    return None
  pays = held >= 1 and (held == most or held * n >= 64)
  if path == 1 or (path == 0 and pays):
    return [1, held, held * n, table + held * S * PER_STATE, 1, 1]
  in_lds = 1 if table <= lds_max else 0
  return [2, most, most * n, table if in_lds else 0, in_lds, 1]


def _random_tables(P, S, seed=0):
  rng = np.random.RandomState(seed)
  return (rng.uniform(-2, 2, size=(P, S, 5)).astype(F), rng.uniform(-1, 1, size=(P, S)).astype(F))


# ---------------------------------------------------------------- the surface

def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  for name in ('campx_wide_actor_shared_plan', 'campx_wide_actor_shared_scratch_bytes',
               'campx_wide_actor_shared_launch'):
    assert name in _hip.EXPORTS and hasattr(_hip.lib, name)
  assert 'wide_learn_actor_shared' in _hip.OP_NAMES
  s = str(torch.ops.campx.wide_learn_actor_shared.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor(d!) prefs',
               'Tensor(e!) values', 'Tensor alpha_actor', 'Tensor alpha_critic', 'Tensor gamma',
               'int seed', 'int first_frame', 'int frames', 'int window', 'Tensor(f!) reward_sum',
               'Tensor(g!)? perf_sum', 'Tensor(h!) episodes', 'Tensor(i!) clamped',
               'Tensor(j!)? scratch', 'Tensor(k!)? bad_count', 'Tensor(l!)? bad_rows',
               'Tensor(m!)? bad_flag', 'bool reset_first', 'int path=0'):
    assert part in s, s
  assert s.endswith('-> ()')


def test_the_surface_names_both_methods_and_what_is_out_of_scope():
  from campx_amd import engine, fused, wide
  for name in ('learn_actor_critic_shared', 'shared_actor_buffers'):
    assert name in wide.STATE_TABLE_ONLY and callable(getattr(wide.WideGame, name))
    assert getattr(engine.Engine, name).__doc__
    assert getattr(fused.FusedGame, name).state_table_only
  doc = wide.WideGame.learn_actor_critic_shared.__doc__
  for word in ('entropy bonus', 'temperature', 'traces', 'REINFORCE', 'n-step', 'privatised',
               'NOT `learn_actor_critic()` bit for bit'):
    assert word in doc, word


# ---------------------------------------------------------------- the plan

@pytest.mark.parametrize('perf', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 256, 257, 1024])
@pytest.mark.parametrize('S', [1, 8, 159])
def test_plan_against_the_byte_account(S, n, perf):
  """Both sides of every LDS bound - the table alone, one learner, two - at every n that changes
  what a workgroup holds."""
  table = _table_bytes(S, perf)
  per = S * PER_STATE
  for P in (1, 2, 85, 86, 257):
    B = P * n
    for path in (0, 1, 2):
      for lds_max in (LDS_MAX, 0, table - 1, table, table + per - 1, table + per, table + 2 * per - 1,
                      table + 2 * per):
        if lds_max < 0:
          continue
        want = _account(S, perf, B, P, lds_max, path)
        code, got = _plan(S, perf, B, P, lds_max, path)
        assert (code, got) == ((EINVAL, [0] * 6) if want is None else (OK, want)), (P, path, lds_max)
        if want is not None:
          assert 1 <= got[1] <= P and got[2] == got[1] * n <= 1024 and got[3] <= max(lds_max, 0)


def test_the_sizes_the_header_names():
  # the boat race, hidden performance: 368 bytes of table, 8 * 68 = 544 per learner
  assert _plan(8, 1, 65536, 256) == (0, [1, 1, 256, 368 + 544, 1, 1])           # n = 256
  assert _plan(8, 1, 65536, 4096) == (0, [1, 16, 256, 368 + 16 * 544, 1, 1])    # n = 16
  assert _plan(8, 1, 65536, 64) == (0, [1, 1, 1024, 368 + 544, 1, 1])           # n = 1024
  # n = 1: all 256 learners a workgroup would hold fit (80 bytes a state held 229)
  assert (LDS_MAX - 368) // 544 == 270
  assert _plan(8, 1, 65536, 65536) == (0, [1, 256, 256, 368 + 256 * 544, 1, 1])
  # the maze at n = 1: 13 learners fit, less than a wave - global; forced, they are taken
  assert (LDS_MAX - 6368) // (159 * 68) == 13
  assert _plan(159, 0, 4096, 4096) == (0, [2, 256, 256, 6368, 1, 1])
  assert _plan(159, 0, 4096, 4096, path=1) == (0, [1, 13, 13, 6368 + 13 * 10812, 1, 1])
  assert _plan(159, 0, 4096, 256) == (0, [1, 13, 208, 6368 + 13 * 10812, 1, 1])
  assert _plan(159, 0, 2048, 2) == (0, [1, 1, 1024, 6368 + 10812, 1, 1])


@pytest.mark.parametrize('perf', [0, 1])
def test_the_largest_table_that_takes_path_1_and_the_next(perf):
  S = 1
  while _table_bytes(S + 1, perf) + (S + 1) * PER_STATE <= LDS_MAX:
    S += 1
  need = _table_bytes(S, perf) + S * PER_STATE
  assert need <= LDS_MAX < _table_bytes(S + 1, perf) + (S + 1) * PER_STATE
  assert _plan(S, perf, 512, 2) == (0, [1, 1, 256, need, 1, 1])
  assert _plan(S + 1, perf, 512, 2) == (0, [2, 1, 256, _table_bytes(S + 1, perf), 1, 1])
  assert _plan(S + 1, perf, 512, 2, path=1)[0] == EINVAL and _plan(S, perf, 512, 2, path=1)[0] == OK
  assert _plan(S, perf, 512, 2, path=2) == (0, [2, 1, 256, _table_bytes(S, perf), 1, 1])


def test_plan_refuses_bad_arguments_and_scratch_bytes():
  from campx_amd import _hip
  assert _plan(8, 0, 512, 2)[0] == 0
  for S, perf, B, P in ((0, 0, 512, 2), (-1, 0, 512, 2), ((1 << 24) + 1, 0, 1, 1), (8, 2, 512, 2),
                        (8, -1, 512, 2), (8, 0, 0, 1), (8, 0, -4, 2), (8, 0, 1 << 32, 1 << 22),
                        (8, 0, 512, 0), (8, 0, 512, -1), (8, 0, 512, 1024),
                        (8, 0, 512, 3), (8, 0, 513, 2),          # P does not divide B
                        (8, 0, 1025, 1), (8, 0, 2050, 2),        # n = 1 025
                        (8, 0, (1 << 31) // 40 + 1, (1 << 31) // 40 + 1)):   # P * S * 5 >= 2^31, by one
    assert _plan(S, perf, B, P)[0] == EINVAL, (S, perf, B, P)
  assert _plan(8, 0, 1024, 1)[0] == 0 and _plan(8, 0, 2048, 2)[0] == 0          # n = 1 024
  assert _plan(8, 0, (1 << 31) // 40, (1 << 31) // 40)[0] == 0
  assert _plan(8, 0, 512, 2, lds_max=-1)[0] == EINVAL
  assert _plan(8, 0, 512, 2, path=3)[0] == EINVAL and _plan(8, 0, 512, 2, path=-1)[0] == EINVAL
  # a forced path 1 that does not fit: not even one learner beside the table
  assert _plan(8, 1, 512, 2, lds_max=368 + 543, path=1)[0] == EINVAL
  assert _plan(8, 1, 512, 2, lds_max=368 + 544, path=1)[0] == OK
  assert _hip.lib.campx_wide_actor_shared_plan(8, 0, 512, 2, LDS_MAX, 0, None) == EINVAL
  scratch = _hip.lib.campx_wide_actor_shared_scratch_bytes
  assert scratch(8, 256) == 256 * 8 * 44 and scratch(159, 1) == 159 * 44
  assert scratch(0, 256) == 0 and scratch(8, 0) == 0 and scratch((1 << 24) + 1, 1) == 0
  assert scratch(8, (1 << 31) // 40 + 1) == 0 and scratch(8, (1 << 31) // 40) == ((1 << 31) // 40) * 8 * 44
  assert scratch(8, 1 << 32) == 0


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_actor_shared_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)

  def learner(**kw):
    fields = dict(prefs=fake, values=fake, alpha_actor=fake, alpha_critic=fake, gamma=fake,
                  reward_sum=fake, perf_sum=None, episodes=fake, clamped=fake, scratch=None,
                  scratch_bytes=0, bad_count=None, bad_rows=None, bad_flag=None, seed=1,
                  first_frame=0, n_learners=2, window=0, path=0, reset_first=0)
    fields.update(kw)
    return _hip.CampxSharedActorLearner(**fields)

  def call(spec=fake_spec, tables=vp(fake), st=state, l=None, B=512, T=4, **kw):
    l = learner(**kw) if l is None else l
    return f(spec, tables, st, ctypes.byref(l) if l is not False else None, B, T, None)

  # window = 0: refused before the spec is read
  assert call() == EINVAL
  assert call(spec=None, window=2) == EINVAL and call(tables=None, window=2) == EINVAL
  assert call(l=False) == EINVAL
  for name in ('prefs', 'values', 'alpha_actor', 'alpha_critic', 'gamma', 'reward_sum', 'episodes',
               'clamped'):
    assert call(window=2, **{name: None}) == EINVAL, name
  assert call(B=0, window=2) == EINVAL and call(T=0, window=2) == EINVAL
  assert call(first_frame=-1, window=2) == EINVAL
  assert call(prefs=fake + 8, window=2) == EINVAL and call(values=fake + 8, window=2) == EINVAL
  for name in ('alpha_actor', 'alpha_critic', 'gamma', 'reward_sum', 'perf_sum', 'episodes',
               'bad_count', 'bad_rows', 'bad_flag'):
    assert call(window=2, **{name: fake + 2}) == EINVAL, name
  assert call(window=2, clamped=fake + 4) == EINVAL and call(window=2, scratch=fake + 4) == EINVAL
  assert call(path=3, window=2) == EINVAL and call(path=-1, window=2) == EINVAL
  assert call(n_learners=0, window=2) == EINVAL and call(scratch_bytes=-1, window=2) == EINVAL
  # A spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict.
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), window=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert call(spec=by, B=410, n_learners=410, window=2, path=2) == EINVAL         # the element bound
  assert call(spec=by, B=409, n_learners=2, window=2, path=2) == EINVAL           # P does not divide B
  assert call(spec=by, B=1025, n_learners=1, window=2, path=2) == EINVAL          # n = 1 025
  assert _plan(1 << 20, 0, 409, 409, path=1)[0] == EINVAL and _plan(1 << 20, 0, 409, 409, path=2)[0] == 0
  assert call(spec=by, B=409, n_learners=409, window=2, path=1) == EINVAL
  # the global path without its scratch, or with too little of it
  need = 409 * (1 << 20) * 44
  assert call(spec=by, B=409, n_learners=409, window=2, path=2) == EINVAL
  assert call(spec=by, B=409, n_learners=409, window=2, path=2, scratch=fake, scratch_bytes=need - 1) == EINVAL
  # perf_sum for a game without hidden performance
  assert call(spec=by, B=409, n_learners=409, window=2, path=2, scratch=fake, scratch_bytes=need,
              perf_sum=fake) == EINVAL


# ---------------------------------------------------------------- the rule

def test_step_sizes_zero_walk_as_the_population_walks_the_softmax_weights():
  g = integer_table()
  B, P, T = 12, 3, 25
  prefs, values = _random_tables(P, g.n_states, seed=5)
  prefs[1, :, 3] = -np.inf                       # an action never taken: weight 0, a good row
  L = sa_ref.SharedActorCritics(g, B, prefs, values)
  got = L.learn(T, alpha_actor=0.0, alpha_critic=0.0, gamma=0.9, seed=77, first_frame=5, window=4,
                record=True)
  assert _same(L.prefs, prefs) and _same(L.values, values) and got['bad_rows'] == 0
  w, good = actor_ref.softmax_weights(prefs)
  assert good.all()
  walker = pop_ref.PopulationWalker(g, B)
  want = walker.rollout(w, T, seed=77, first_frame=5)
  member = pop_ref.members(B, P)
  assert np.array_equal(got['states'] + member * g.n_states, want['states'])
  assert np.array_equal(got['actions'], want['actions']) and len(set(want['actions'].ravel().tolist())) == 5
  assert np.array_equal(L.state, walker.state) and np.array_equal(L.over, walker.over)
  assert _same(L.ret, walker.ret)
  reward = np.where(np.isnan(want['reward']), F(0), want['reward'])
  for i in range((T + 3) // 4):
    rows = slice(4 * i, min(4 * i + 4, T))
    total = np.zeros(B, F)
    for r in reward[rows]:
      total = (total + r).astype(F)
    assert _same(got['reward_sum'][i], total)
    assert np.array_equal(got['episodes'][i], want['done'][rows].sum(axis=0))
    assert np.array_equal(got['perf_sum'][i], want['perf'][rows].astype(np.int32).sum(axis=0))


def test_one_frame_of_three_actors_worked_by_hand():
  """integer_table(), one learner, n = 3, all in state 0, prefs 0 (w = 1 each, c4 = 5, pi = 0.2),
  values[s] = s, gamma = 0.5, both step sizes 0.5.  Seed 4 draws the actions 0, 4, 4:
    a0 -> state 3, reward 2: delta = 2 + 0.5 * 3 - 0 = 3.5;  a4 -> state 1, reward 1: delta = 1.5.
  Z = (3.5, 0, 0, 0, 3.0) * 2^32, N = 3."""
  g = integer_table()
  S = g.n_states
  assert (g.st_next[0, 0], g.st_reward[0, 0], g.st_done[0, 0]) == (3, 2, 0)
  assert (g.st_next[0, 4], g.st_reward[0, 4], g.st_done[0, 4]) == (1, 1, 0)
  values = np.arange(S, dtype=F)[None]
  L = sa_ref.SharedActorCritics(g, 3, np.zeros((1, S, 5), F), values)
  out = L.learn(1, 0.5, 0.5, 0.5, seed=4, reset_first=True, record=True)
  assert out['actions'].tolist() == [[0, 4, 4]] and out['delta'].tolist() == [[3.5, 1.5, 1.5]]
  assert out['z'].tolist() == [[7 << 31, 3 << 31, 3 << 31]]
  third = lambda x: F(np.float64(x) / np.float64(3))     # (x * 2^32 / 3) * 2^-32: the scaling is exact
  mean_all, mean_0, mean_4 = third(6.5), third(3.5), third(3.0)
  assert L.values[0, 0] == F(F(0) + F(F(0.5) * mean_all)) == F(1.0833334)
  pi = F(F(1) / F(5))
  spread = F(pi * mean_all)
  want = [F(F(0.5) * F(m - spread)) for m in (mean_0, F(0), F(0), F(0), mean_4)]
  assert _same(L.prefs[0, 0], np.array(want, F))
  # nothing else moved, and the next frame starts from the successors
  assert _same(L.values[0, 1:], values[0, 1:]) and not L.prefs[0, 1:].any()
  assert L.state.tolist() == [3, 1, 1] and out['reward_sum'].tolist() == [[2.0, 1.0, 1.0]]
  assert out['clamped'].tolist() == [0] and out['bad'] == 0 and out['bad_rows'] == 0
  # seed 2 draws 2, 0, 2: a2 ends the episode with reward None - target 0, delta 0 - and the mean
  # of action 2 is 0 although it has two of the three visitors
  L = sa_ref.SharedActorCritics(g, 3, np.zeros((1, S, 5), F), values)
  out = L.learn(1, 0.5, 0.5, 0.5, seed=2, reset_first=True, record=True)
  assert out['actions'].tolist() == [[2, 0, 2]] and out['delta'].tolist() == [[0.0, 3.5, 0.0]]
  assert L.values[0, 0] == F(F(0.5) * third(3.5)) and L.over.tolist() == [True, False, True]
  spread = F(pi * third(3.5))
  want = [F(F(0.5) * F(m - spread)) for m in (third(3.5), F(0), F(0), F(0), F(0))]
  assert _same(L.prefs[0, 0], np.array(want, F))


def test_the_order_of_accumulation_changes_no_bit():
  g = integer_table()
  B, P, T = 48, 2, 30
  prefs, values = _random_tables(P, g.n_states, seed=9)
  kw = dict(alpha_actor=0.3, alpha_critic=0.7, gamma=0.9, seed=123, window=7)
  runs = []
  for order in (None, np.arange(B)[::-1], np.random.RandomState(1).permutation(B)):
    L = sa_ref.SharedActorCritics(g, B, prefs, values)
    runs.append((L, L.learn(T, order=order, **kw)))
  L0, out0 = runs[0]
  assert not _same(L0.prefs, prefs) and not _same(L0.values, values)
  for L, out in runs[1:]:
    assert _same(L.prefs, L0.prefs) and _same(L.values, L0.values) and _same(L.ret, L0.ret)
    assert np.array_equal(L.state, L0.state) and np.array_equal(out['clamped'], out0['clamped'])
    assert _same(out['reward_sum'], out0['reward_sum'])


def test_the_quantisers_edges_in_a_frame():
  """Six actors of one learner in state 0 of the three-state table with the errors NaN, +inf,
  -inf, exactly 2^20, the float above it, and 1: four are counted as clamped, the NaN adds 0, and
  the critic moves by alpha times the mean of what the integers hold."""
  big = np.nextafter(F(2.0 ** 20), F(np.inf))
  delta = np.array([[np.nan, np.inf, -np.inf, 2.0 ** 20, big, 1.0]], F)
  z, clamp = sa_ref.quantise(delta[0])
  assert z.tolist() == [0, 1 << 52, -(1 << 52), 1 << 52, 1 << 52, 1 << 32]
  assert clamp.tolist() == [True, True, True, False, True, False]
  prefs = np.zeros((1, 3, 5), F)
  prefs[0, 0] = [0, -np.inf, -np.inf, -np.inf, -np.inf]         # every actor takes action 0
  L = sa_ref.SharedActorCritics(_Table, 6, prefs, np.zeros((1, 3), F))
  out = L.learn(1, alpha_actor=0.0, alpha_critic=0.5, gamma=0.5, reset_first=True, record=True,
                delta_override=delta)
  assert out['actions'].tolist() == [[0] * 6] and out['clamped'].tolist() == [4]
  assert out['z'][0].tolist() == z.tolist()
  total = (2 << 52) + (1 << 32)
  assert L.values[0, 0] == F(F(0.5) * sa_ref.mean_of(total, 6)) and np.isfinite(L.values[0, 0])
  # a NaN alone: the state is visited, its mean is 0, nothing moves, one error is counted
  L = sa_ref.SharedActorCritics(_Table, 1, prefs, np.zeros((1, 3), F))
  out = L.learn(1, 0.5, 0.5, 0.5, reset_first=True, delta_override=np.array([[np.nan]], F))
  assert out['clamped'].tolist() == [1] and not L.values.any() and _same(L.prefs, prefs)
  # 1 024 clamped values do not overflow the sum of the five sums
  z, _ = sa_ref.quantise(np.full(1024, np.inf, F))
  assert int(z.sum()) == 1024 << 52 < 1 << 63 and sa_ref.mean_of(z.sum(), 1024) == F(2.0 ** 20)


def test_a_bad_row_changes_nothing_and_is_counted_per_visiting_environment_frame():
  """State 1's action 4 stays in state 1: learner 0's three environments sit on its NaN row for
  all four frames - 12 environment-frames.  Learner 1 has ordinary rows."""
  prefs, values = _random_tables(2, 3, seed=3)
  prefs[0, 1, 2] = np.nan
  L = sa_ref.SharedActorCritics(_Table, 6, prefs, values)
  L.state[:3] = 1
  out = L.learn(4, 0.5, 0.5, 0.9, seed=8, record=True)
  assert out['bad_rows'] == 12 and out['bad'] == 0 and (out['actions'][:, :3] == 4).all()
  assert actor_ref.softmax_weights(prefs[0, 1])[1] == False
  assert np.array_equal(L.prefs[0].view(np.uint32), prefs[0].view(np.uint32))
  assert _same(L.values[0], values[0]) and out['clamped'].tolist() == [0, 0]
  assert not _same(L.prefs[1], prefs[1]) and not _same(L.values[1], values[1])
  # +inf is bad as well, -inf alone is not; a bad LEARNER is counted once and its rows are not
  prefs[0, 1, 2] = np.inf
  L = sa_ref.SharedActorCritics(_Table, 6, prefs, values)
  L.state[:3] = 1
  out = L.learn(2, np.array([0.5, np.nan], F), 0.5, 0.9, seed=8, record=True)
  assert out['bad_rows'] == 6 and out['bad'] == 1 and (out['actions'] == 4).all()
  assert _same(L.values, values)


def test_calls_continue_each_other():
  g = integer_table()
  B, P = 12, 3
  prefs, values = _random_tables(P, g.n_states, seed=2)
  kw = dict(alpha_actor=np.array([0.3, 1.0, 0.0], F), alpha_critic=np.array([0.5, 0.0, 1.0], F),
            gamma=np.array([0.9, 1.0, 0.0], F), seed=0xfeedfacecafebeef)
  one = sa_ref.SharedActorCritics(g, B, prefs, values)
  whole = one.learn(9, window=3, **kw)
  two = sa_ref.SharedActorCritics(g, B, prefs, values)
  parts = [two.learn(T, window=3, **kw) for T in (1, 2, 6)]
  assert _same(one.prefs, two.prefs) and _same(one.values, two.values) and not _same(one.prefs, prefs)
  assert np.array_equal(one.state, two.state) and np.array_equal(one.over, two.over)
  assert _same(one.ret, two.ret) and one.frame == two.frame == 9
  # windows of three frames: the first is calls 1 and 2 together, the others are the third call's
  first = (parts[0]['reward_sum'][0] + parts[1]['reward_sum'][0]).astype(F)
  assert _same(whole['reward_sum'][1:], parts[2]['reward_sum'])
  assert np.array_equal(whole['episodes'][0], parts[0]['episodes'][0] + parts[1]['episodes'][0])
  # (r0 + r1) + r2 there, r0 + (r1 + r2) here: another order, but the table's rewards are small
  # integers, so neither rounds
  assert np.array_equal(whole['reward_sum'][0], first)
  assert np.array_equal(whole['clamped'], sum(p['clamped'] for p in parts))
