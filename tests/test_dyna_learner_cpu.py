"""`campx_wide_dyna_plan()` - pure host arithmetic - against the header's account of the bytes, the
refusals of `campx_wide_dyna_launch()` that are decided before a device is touched, the op's schema,
and the numpy learners of tests/dyna_learner_reference.py on their own: against
tests/learner_reference.py at planning = 0, two calls against one, a table worked by hand, the
model's invariants, and one check that planning does what it is for.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import dyna_learner_reference as dyna_ref
import learner_reference as learn_ref
from test_population_cpu import _Table, _same, _valid_spec
from test_trace_learner_cpu import _TwoStates

F = np.float32
LDS_MAX = 144 * 1024
THREADS = 256
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h


def _plan(S, perf, B, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_dyna_plan(S, perf, B, lds_max, path, out)
  return code, list(out)


def _table_bytes(S, perf):
  up = lambda x: (x + 15) // 16 * 16
  return up(40 * S) + (up(5 * S) if perf else 0)


def _words(S):
  return (5 * S + 31) // 32


def _need(S, perf):
  """The header's account of path 1: the table, and per learner q (20 bytes a state), the list (16
  bits an element: 10 bytes a state) and the bitmap."""
  return _table_bytes(S, perf) + THREADS * (S * 20 + S * 10 + 4 * _words(S))


def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  for name in ('campx_wide_dyna_plan', 'campx_wide_dyna_launch'):
    assert name in _hip.EXPORTS and hasattr(_hip.lib, name)
  assert 'wide_learn_dyna' in _hip.OP_NAMES and _hip.DYNA_MAX_PLANNING == 1024
  s = str(torch.ops.campx.wide_learn_dyna.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor(d!) q',
               'Tensor(e!) seen', 'Tensor(f!) n_seen', 'Tensor planning', 'Tensor alpha', 'Tensor gamma',
               'Tensor epsilon', 'int rule', 'int seed', 'int first_frame', 'int frames', 'int window',
               'Tensor(g!) reward_sum', 'Tensor(h!)? perf_sum', 'Tensor(i!) episodes',
               'Tensor(j!)? marks', 'Tensor(k!)? bad_count', 'Tensor(l!)? bad_flag', 'bool reset_first',
               'int path=0'):
    assert part in s, s
  assert s.endswith('-> ()')


def test_the_surface_names_the_methods():
  from campx_amd import engine, wide
  for name in ('learn_dyna', 'dyna_buffers'):
    assert name in wide.STATE_TABLE_ONLY and callable(getattr(wide.WideGame, name))
    assert getattr(engine.Engine, name).__doc__ and getattr(wide.WideGame, name).__doc__
  doc = wide.WideGame.learn_dyna.__doc__
  assert 'UNIFORMLY FROM THE SEEN PAIRS' in doc and 'planning' in doc and 'model' in doc


@pytest.mark.parametrize('perf', [0, 1])
def test_both_sides_of_the_path_1_bound(perf):
  """144 KiB: q, list and bitmap of 256 learners fit beside the table up to 18 states."""
  assert _need(18, perf) <= LDS_MAX < _need(19, perf)
  for B in (1, 65, 65536):
    assert _plan(18, perf, B) == (0, [1, _need(18, perf), THREADS, 1, 3])
    assert _plan(19, perf, B) == (0, [2, _table_bytes(19, perf), THREADS, 1, 3])
  assert _plan(19, perf, 65, path=1)[0] == EINVAL
  # the same bound, moved by the setting: one byte less and the learners go through L1 / L2
  need = _need(18, perf)
  assert _plan(18, perf, 65, lds_max=need)[1][:2] == [1, need]
  assert _plan(18, perf, 65, lds_max=need - 1)[1][:2] == [2, _table_bytes(18, perf)]
  assert _plan(18, perf, 65, lds_max=need - 1, path=1)[0] == EINVAL
  assert _plan(19, perf, 65, lds_max=_need(19, perf))[1][:2] == [1, _need(19, perf)]
  # the bitmap's words: 32 pairs each
  for S, words in ((1, 1), (6, 1), (7, 2), (12, 2), (13, 3), (159, 25)):
    assert _words(S) == words and _plan(S, perf, 65)[1][4] == words


def test_the_boat_race_s_words_and_the_games_beyond_the_bound():
  assert _need(8, 1) == 320 + 48 + 256 * (160 + 80 + 8)
  assert _plan(8, 1, 65536) == (0, [1, 320 + 48 + 63488, THREADS, 1, 2])
  assert _plan(159, 0, 65536) == (0, [2, 6368, THREADS, 1, 25])                # the maze
  assert _plan(470, 0, 65536) == (0, [2, 18800, THREADS, 1, 74])               # pickups
  assert _plan(1 << 16, 0, 8) == (0, [2, 0, THREADS, 0, 10240])                # not even the entries fit
  # a list element is 16 bits on path 1: no setting takes more than 65 536 pairs there
  assert _plan(13108, 0, 8, lds_max=1 << 40)[1][0] == 2 and _plan(13107, 0, 8, lds_max=1 << 40)[1][0] == 1


def test_forced_paths():
  table = _table_bytes(8, 1)
  assert _plan(8, 1, 65, path=1) == (0, [1, _need(8, 1), THREADS, 1, 2])
  assert _plan(8, 1, 65, path=2) == (0, [2, table, THREADS, 1, 2])
  assert _plan(8, 1, 65, path=2, lds_max=table - 1) == (0, [2, 0, THREADS, 0, 2])
  assert _plan(8, 1, 65, lds_max=0) == (0, [2, 0, THREADS, 0, 2])
  assert _plan(8, 1, 65, path=1, lds_max=0)[0] == EINVAL


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  assert _plan(8, 0, 512)[0] == 0
  for S, perf, B in ((0, 0, 512), (-1, 0, 512), ((1 << 24) + 1, 0, 1), (8, 2, 512), (8, -1, 512),
                     (8, 0, 0), (8, 0, -4), (8, 0, 1 << 32),
                     (8, 0, (1 << 31) // 40 + 1),            # B * S * 5 >= 2^31, by one learner
                     (1 << 24, 0, 26)):
    assert _plan(S, perf, B)[0] == EINVAL, (S, perf, B)
  assert _plan(8, 0, (1 << 31) // 40)[0] == 0 and _plan(1 << 24, 0, 25)[0] == 0
  assert _plan(8, 0, 512, lds_max=-1)[0] == EINVAL
  assert _plan(8, 0, 512, path=3)[0] == EINVAL and _plan(8, 0, 512, path=-1)[0] == EINVAL
  assert _hip.lib.campx_wide_dyna_plan(8, 0, 512, LDS_MAX, 0, None) == EINVAL


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_dyna_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)

  def learner(**kw):
    fields = dict(q=fake, alpha=fake, gamma=fake, epsilon=fake, reward_sum=fake, perf_sum=None,
                  episodes=fake, bad_count=None, bad_flag=None, seed=1, first_frame=0, window=0, rule=0,
                  path=0, reset_first=0, seen=fake, n_seen=fake, planning=fake, marks=fake)
    fields.update(kw)
    return _hip.CampxDynaLearner(**fields)

  def call(spec=fake_spec, tables=vp(fake), st=state, l=None, B=512, T=4, **kw):
    l = learner(**kw) if l is None else l
    return f(spec, tables, st, ctypes.byref(l) if l is not False else None, B, T, None)

  # window = 0: refused before the spec is read (every call below that is not about the window
  # would reach the fake spec if it were not refused first)
  assert call() == EINVAL
  assert call(l=False) == EINVAL
  assert call(spec=None, window=2) == EINVAL and call(tables=None, window=2) == EINVAL
  for name in ('q', 'alpha', 'gamma', 'epsilon', 'reward_sum', 'episodes', 'seen', 'n_seen', 'planning'):
    assert call(window=2, **{name: None}) == EINVAL, name
  for name in ('q', 'seen'):
    assert call(window=2, **{name: fake + 4}) == EINVAL and call(window=2, **{name: fake + 8}) == EINVAL
  for name in ('alpha', 'gamma', 'epsilon', 'reward_sum', 'perf_sum', 'episodes', 'bad_count',
               'bad_flag', 'n_seen', 'planning', 'marks'):
    assert call(window=2, **{name: fake + 2}) == EINVAL, name
  assert call(B=0, window=2) == EINVAL and call(T=0, window=2) == EINVAL
  assert call(first_frame=-1, window=2) == EINVAL
  assert call(rule=2, window=2) == EINVAL and call(path=3, window=2) == EINVAL
  # a spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), window=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert call(spec=by, B=410, window=2) == EINVAL                       # the element bound
  assert _plan(1 << 20, 0, 409, path=1)[0] == EINVAL and _plan(1 << 20, 0, 409, path=2)[0] == 0
  assert call(spec=by, B=409, window=2, path=1) == EINVAL
  assert call(spec=by, B=409, window=2, path=2, marks=None) == EINVAL   # path 2 needs its scratch
  assert call(spec=by, B=409, window=2, path=0, marks=None) == EINVAL   # ... planned or forced
  assert call(spec=by, B=409, window=2, path=2, perf_sum=fake) == EINVAL


# ---------------------------------------------------------------- the reference itself

def _random_q(B, seed=0, S=3):
  return np.random.RandomState(seed).uniform(-1, 1, size=(B, S, 5)).astype(F)


def _first_visits(states, actions, e):
  order = []
  for s, a in zip(states[:, e].tolist(), actions[:, e].tolist()):
    if s * 5 + a not in order:
      order.append(s * 5 + a)
  return order


@pytest.mark.parametrize('rule', dyna_ref.RULES)
def test_planning_zero_is_the_one_step_learner_and_records_first_visits(rule):
  B, T = 12, 40
  q = _random_q(B)
  kw = dict(alpha=0.3, gamma=0.8, epsilon=0.25, rule=rule, seed=0xfeedfacecafebeef, window=7)
  one = learn_ref.Learners(_Table, B, q)
  want = one.learn(T, record=True, **kw)
  two = dyna_ref.DynaLearners(_Table, B, q)
  got = two.learn_dyna(T, planning=0, **kw)
  assert _same(one.q, two.q) and not _same(one.q, q)
  for k in ('reward_sum', 'perf_sum', 'episodes'):
    assert _same(want[k], got[k]), k
  assert np.array_equal(one.state, two.state) and np.array_equal(one.over, two.over)
  assert _same(one.ret, two.ret) and one.frame == two.frame
  for e in range(B):
    order = _first_visits(want['states'], want['actions'], e)
    assert two.n_seen[e] == len(order) > 1 and two.seen[e, :len(order)].tolist() == order
    assert not two.seen[e, len(order):].any()


@pytest.mark.parametrize('rule', dyna_ref.RULES)
def test_two_calls_learn_what_one_call_learns(rule):
  B, T1, T2 = 9, 7, 11
  q = _random_q(B, seed=2)
  planning = np.arange(B) % 7
  kw = dict(planning=planning, alpha=0.3, gamma=0.8, epsilon=0.25, rule=rule, seed=77)
  one, two = (dyna_ref.DynaLearners(_Table, B, q) for _ in range(2))
  one.learn_dyna(T1 + T2, **kw)
  two.learn_dyna(T1, **kw)
  assert two.n_seen.all()
  two.learn_dyna(T2, **kw)
  assert _same(one.q, two.q) and not _same(one.q, q)
  assert _same(one.seen, two.seen) and _same(one.n_seen, two.n_seen)
  assert np.array_equal(one.state, two.state) and _same(one.ret, two.ret)
  # ... and planning changed what was learnt
  none = dyna_ref.DynaLearners(_Table, B, q)
  none.learn_dyna(T1 + T2, **dict(kw, planning=0))
  assert _same(none.q[0], one.q[0]) and not _same(none.q[1], one.q[1])


def test_three_frames_by_hand_with_two_planning_updates_each():
  """The two-state table of test_trace_learner_cpu.py.  epsilon = 1, seed 18: the actions drawn are
  0, 0, 1.  alpha = gamma = 0.5, planning = 2, q[0] = [0, 1, 0, 0, 0], q[1] = [2, 0, 0, 0, 0].  The
  planning words (x0, x1 of block 0) of learner 0 are 0x5b49bb5d, 0xcb030238 at frame 0,
  0x6305d1d4, 0xf441d7e3 at frame 1 and 0x1fa08b69, 0x8b3bd6b3 at frame 2."""
  blocks = [dyna_ref.planning_words(18, np.arange(1), f, 0)[0, :2].tolist() for f in range(3)]
  assert blocks == [[0x5b49bb5d, 0xcb030238], [0x6305d1d4, 0xf441d7e3], [0x1fa08b69, 0x8b3bd6b3]]
  q = np.array([[[0, 1, 0, 0, 0], [2, 0, 0, 0, 0]]], F)
  L = dyna_ref.DynaLearners(_TwoStates, 1, q)
  kw = dict(planning=2, alpha=0.5, gamma=0.5, epsilon=1.0, seed=18, record=True)
  out = L.learn_dyna(1, **kw)
  # frame 0: state 0, a0 -> state 1, reward 0.  target 0 + (0.5 * 1) * max q[1] = 1, delta 1:
  # q[0, 0] = 0.5.  Pair 0 is new: seen = [0].  Both planning steps can only draw index
  # (x * 1) >> 32 = 0, pair 0: target 1 again, delta 0.5 -> q[0, 0] = 0.75; delta 0.25 -> 0.875.
  assert out['states'].tolist() == [[0]] and out['actions'].tolist() == [[0]]
  assert out['planned'][0].tolist() == [[0], [0]]
  assert L.q.tolist() == [[[0.875, 1, 0, 0, 0], [2, 0, 0, 0, 0]]]
  assert L.n_seen.tolist() == [1] and L.seen[0, :1].tolist() == [0]
  out = L.learn_dyna(1, **kw)
  # frame 1: state 1, a0, reward 1, DONE: target 1, delta -1: q[1, 0] = 1.5.  Pair 5 is new:
  # seen = [0, 5].  k = 0: (0x6305d1d4 * 2) >> 32 = 0, pair 0: target (0.5 * 1) * 1.5 = 0.75, delta
  # 0.75 - 0.875 = -0.125: q[0, 0] = 0.8125.  k = 1: (0xf441d7e3 * 2) >> 32 = 1, pair 5: DONE,
  # target 1, delta -0.5: q[1, 0] = 1.25.
  assert out['states'].tolist() == [[1]] and out['actions'].tolist() == [[0]]
  assert out['planned'][0].tolist() == [[0], [5]] and out['episodes'].tolist() == [[1]]
  assert L.q.tolist() == [[[0.8125, 1, 0, 0, 0], [1.25, 0, 0, 0, 0]]]
  assert L.n_seen.tolist() == [2] and L.seen[0, :2].tolist() == [0, 5] and L.over.tolist() == [True]
  out = L.learn_dyna(1, **kw)
  # frame 2: a new episode, state 0, a1 stays in state 0, reward 0: target (0.5 * 1) * max q[0] =
  # 0.5 (the row before the write: its maximum is q[0, 1] = 1 itself), delta -0.5: q[0, 1] = 0.75.
  # Pair 1 is new: seen = [0, 5, 1].  k = 0: (0x1fa08b69 * 3) >> 32 = 0, pair 0: target
  # 0.5 * 1.25 = 0.625, delta -0.1875: q[0, 0] = 0.71875.  k = 1: (0x8b3bd6b3 * 3) >> 32 = 1, pair
  # 5: target 1, delta -0.25: q[1, 0] = 1.125.
  assert out['states'].tolist() == [[0]] and out['actions'].tolist() == [[1]]
  assert out['planned'][0].tolist() == [[0], [5]]
  assert L.q.tolist() == [[[0.71875, 0.75, 0, 0, 0], [1.125, 0, 0, 0, 0]]]
  assert L.n_seen.tolist() == [3] and L.seen[0].tolist() == [0, 5, 1, 0, 0, 0, 0, 0, 0, 0]
  assert L.state.tolist() == [0] and L.ret.tolist() == [0.0] and L.frame == 3


def test_the_list_never_repeats_and_never_exceeds_the_table():
  B, T = 16, 300
  L = dyna_ref.DynaLearners(_Table, B, _random_q(B, seed=3))
  L.learn_dyna(T, planning=3, alpha=0.3, gamma=0.8, epsilon=0.5, seed=5)
  assert L.n_seen.max() == 15 and (L.n_seen <= 15).all()         # some learner met every pair
  for e in range(B):
    listed = L.seen[e, :L.n_seen[e]].tolist()
    assert len(set(listed)) == len(listed) and all(0 <= i < 15 for i in listed)
  # a list given with repeats that is already full takes no more, and is sampled as given
  full = np.zeros((1, 15), np.int32)
  M = dyna_ref.DynaLearners(_Table, 1, _random_q(1), full, np.array([15], np.int32))
  out = M.learn_dyna(20, planning=4, epsilon=1.0, seed=5, record=True)
  assert M.n_seen.tolist() == [15] and not M.seen.any() and len(np.unique(out['actions'])) > 1
  assert all((p == 0).all() for p in out['planned'])


def test_the_planning_stream_is_unrelated_to_exploration_s():
  """Same seed, learner and frame: the exploration block has fourth counter word 1 and the pair of
  frames in its second, the planning blocks words 2, 3, ... and the frame itself."""
  seed, env = 0x1234567890abcdef, np.arange(64)
  for f in (0, 1, 2, 7, (1 << 40) + 1):
    x0, x1 = learn_ref.words(seed, env, f)
    blocks = [dyna_ref.planning_words(seed, env, f, b) for b in range(3)]
    for b in blocks:
      assert not np.isin(b, np.stack([x0, x1])).any()
    assert not np.array_equal(blocks[0], blocks[1]) and not np.array_equal(blocks[1], blocks[2])
    # (e, f, k): another learner, frame or block is another word
    assert len(np.unique(np.concatenate([b.ravel() for b in blocks]))) == 3 * 64 * 4
  a = dyna_ref.planning_words(seed, env, 5, 0)
  assert not np.array_equal(a, dyna_ref.planning_words(seed, env, 4, 0))
  assert not np.array_equal(a, dyna_ref.planning_words(seed, env, 5 + (1 << 32), 0))
  assert not np.array_equal(a, dyna_ref.planning_words(seed + 1, env, 5, 0))
  # the mean of idx / n_seen over many draws is near one half
  at = (a.astype(np.uint64) * np.uint64(7)) >> np.uint64(32)
  assert at.max() == 6 and at.min() == 0


def test_bad_planning_and_bad_models_leave_everything_untouched_and_are_counted_once():
  B, T = 8, 10
  q0 = _random_q(B, seed=4)
  seen = np.zeros((B, 15), np.int32)
  seen[:, :3] = [4, 9, 14]
  n_seen = np.full(B, 3, np.int32)
  planning = np.full(B, 2, np.int64)
  planning[1], planning[2] = -1, 1025                  # outside 0 .. 1024
  n_seen[3], n_seen[4] = -1, 16                        # outside 0 .. 15
  seen[5, 1], seen[6, 2] = 15, -1                      # a listed pair outside the table
  seen[7, 3] = 99                                      # beyond n_seen: never read
  assert dyna_ref.bad_models(seen, n_seen, 15).tolist() == [False] * 3 + [True] * 4 + [False]
  L = dyna_ref.DynaLearners(_Table, B, q0, seen, n_seen)
  out = L.learn_dyna(T, planning=planning, alpha=0.5, gamma=0.5, epsilon=0.3, seed=9, record=True)
  assert out['bad'] == 6
  bad = [1, 2, 3, 4, 5, 6]
  assert (out['actions'][:, bad] == 4).all()
  assert _same(L.q[bad], q0[bad]) and _same(L.seen[bad], seen[bad]) and _same(L.n_seen[bad], n_seen[bad])
  for e in (0, 7):
    assert not _same(L.q[e], q0[e]) and L.n_seen[e] > 3 and L.seen[e, :3].tolist() == [4, 9, 14]
  assert L.seen[7, 3] != 99                            # (overwritten by the fourth pair it met)
  # planning = 1024 is allowed; a bad alpha is bad here too
  assert dyna_ref.DynaLearners(_Table, 1).learn_dyna(1, planning=1024)['bad'] == 0
  assert dyna_ref.DynaLearners(_Table, 1).learn_dyna(1, alpha=np.inf)['bad'] == 1


def test_planning_ends_more_episodes_from_the_same_experience():
  """The 16x16 maze of test_learner.py (159 states, -1 a step, 49 at the goal), 16 learners, 1 500
  frames each from zero tables, alpha 0.5, gamma 0.95, epsilon 0.3, seed 7: with planning = 20 the
  learners end 12 episodes in total, with planning = 0 none - the reward of the first goal a
  learner stumbles on reaches the start within a few frames instead of one state per episode."""
  from campx_amd import tabulate
  from campx_amd.games import maze
  g = tabulate.trace(maze.build(16, 16))
  assert g.n_states == 159
  totals = []
  for n in (0, 20):
    L = dyna_ref.DynaLearners(g, 16)
    out = L.learn_dyna(1500, planning=n, alpha=0.5, gamma=0.95, epsilon=0.3, seed=7, reset_first=True)
    totals.append(int(out['episodes'].sum()))
  assert totals == [0, 12] and totals[1] > totals[0]
