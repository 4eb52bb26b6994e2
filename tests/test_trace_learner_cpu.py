"""`campx_wide_traces_plan()` - pure host arithmetic - against the header's account of the bytes,
the refusals of `campx_wide_traces_launch()` that are decided before a device is touched, the op's
schema, and the numpy learners of tests/trace_learner_reference.py on their own: against
tests/learner_reference.py at lam = 0, accumulating against replacing, and a table worked by hand.
No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import learner_reference as learn_ref
import trace_learner_reference as trace_ref
from test_population_cpu import _Table, _same, _valid_spec

F = np.float32
LDS_MAX = 144 * 1024
THREADS = 256
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h


def _plan(S, perf, B, lds_max=LDS_MAX, path=0, team=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_traces_plan(S, perf, B, lds_max, path, team, out)
  return code, list(out)


def _table_bytes(S, perf):
  up = lambda x: (x + 15) // 16 * 16
  return up(40 * S) + (up(5 * S) if perf else 0)


def _need(S, perf, L):
  """The header's account of path 1: the table, and q and z - 8 bytes per entry - of 256 / L learners."""
  return _table_bytes(S, perf) + (THREADS // L) * S * 5 * 8


def _smallest_team(S, perf, lds_max=LDS_MAX):
  for L in (1, 2, 4, 8, 16, 32, 64, 128, 256):
    if _need(S, perf, L) <= lds_max:
      return L
  return None


def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  for name in ('campx_wide_traces_plan', 'campx_wide_traces_launch'):
    assert name in _hip.EXPORTS and hasattr(_hip.lib, name)
  assert 'wide_learn_traces' in _hip.OP_NAMES
  assert _hip.TRACE_KINDS == {'accumulating': 0, 'replacing': 1}
  s = str(torch.ops.campx.wide_learn_traces.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor(d!) q',
               'Tensor(e!) traces', 'Tensor alpha', 'Tensor gamma', 'Tensor epsilon', 'Tensor lam',
               'int rule', 'int trace', 'int seed', 'int first_frame', 'int frames', 'int window',
               'Tensor(f!) reward_sum', 'Tensor(g!)? perf_sum', 'Tensor(h!) episodes',
               'Tensor(i!)? bad_count', 'Tensor(j!)? bad_flag', 'bool reset_first', 'int path=0',
               'int team=0'):
    assert part in s, s
  assert s.endswith('-> ()')


def test_the_surface_names_the_method():
  from campx_amd import engine, wide
  assert 'learn_traces' in wide.STATE_TABLE_ONLY and callable(wide.WideGame.learn_traces)
  assert engine.Engine.learn_traces.__doc__
  doc = wide.WideGame.learn_traces.__doc__
  assert 'Q(lambda)' in doc and 'replacing' in doc and 'team' in doc


@pytest.mark.parametrize('perf', [0, 1])
@pytest.mark.parametrize('small,L', [(14, 1), (28, 2), (56, 4)])
def test_both_sides_of_every_team_boundary(small, L, perf):
  """144 KiB: one lane per learner up to 14 states, two up to 28, four up to 56."""
  assert _smallest_team(small, perf) == L and _smallest_team(small + 1, perf) == 2 * L
  for B in (1, 65, 65536):
    assert _plan(small, perf, B) == (0, [1, L, _need(small, perf, L), THREADS, 1])
    assert _plan(small + 1, perf, B) == (0, [1, 2 * L, _need(small + 1, perf, 2 * L), THREADS, 1])
  # the same boundary, moved by the setting: one byte less and the team doubles
  need = _need(small, perf, L)
  assert _plan(small, perf, 65, lds_max=need)[1][:3] == [1, L, need]
  assert _plan(small, perf, 65, lds_max=need - 1)[1][:3] == [1, 2 * L, _need(small, perf, 2 * L)]
  # a forced team that does not fit goes through L1 / L2 unless path 1 is forced too
  table = _table_bytes(small + 1, perf)
  assert _plan(small + 1, perf, 65, team=L) == (0, [2, L, table, THREADS, 1])
  assert _plan(small + 1, perf, 65, team=L, path=1)[0] == EINVAL
  assert _plan(small + 1, perf, 65, team=2 * L, path=1)[0] == 0


def test_the_boat_race_s_words_and_the_sizes_the_header_names():
  assert _need(8, 1, 1) == 320 + 48 + 81920
  assert _plan(8, 1, 65536) == (0, [1, 1, 320 + 48 + 81920, THREADS, 1])
  assert _plan(159, 0, 65536) == (0, [1, 16, 6368 + 16 * 159 * 40, THREADS, 1])       # the maze
  assert _plan(470, 0, 65536) == (0, [1, 64, 18800 + 4 * 470 * 40, THREADS, 1])       # pickups
  # one learner per workgroup up to roughly 1 800 states; beyond, the global path, the largest team
  S = 1
  while _need(S + 1, 0, 256) <= LDS_MAX:
    S += 1
  assert S == 1843 and 1700 < S < 1900
  assert _plan(S, 0, 512) == (0, [1, 256, _need(S, 0, 256), THREADS, 1])
  assert _plan(S + 1, 0, 512) == (0, [2, 256, _table_bytes(S + 1, 0), THREADS, 1])
  assert _plan(S + 1, 0, 512, path=1)[0] == EINVAL
  assert _plan(1 << 16, 0, 8) == (0, [2, 256, 0, THREADS, 0])     # not even the entries fit


@pytest.mark.parametrize('team', [1, 2, 4, 8, 16, 32, 64, 128, 256])
def test_forced_paths_and_teams(team):
  table = _table_bytes(8, 1)
  assert _plan(8, 1, 65, team=team) == (0, [1, team, _need(8, 1, team), THREADS, 1])
  assert _plan(8, 1, 65, team=team, path=1) == (0, [1, team, _need(8, 1, team), THREADS, 1])
  assert _plan(8, 1, 65, team=team, path=2) == (0, [2, team, table, THREADS, 1])
  assert _plan(8, 1, 65, team=team, path=2, lds_max=table - 1) == (0, [2, team, 0, THREADS, 0])
  assert _plan(8, 1, 65, team=team, lds_max=0) == (0, [2, team, 0, THREADS, 0])
  assert _plan(8, 1, 65, team=team, path=1, lds_max=_need(8, 1, team) - 1)[0] == EINVAL


def test_an_unforced_team_on_a_forced_path():
  assert _plan(8, 1, 65, path=2) == (0, [2, 256, _table_bytes(8, 1), THREADS, 1])
  assert _plan(29, 1, 65, path=1) == (0, [1, 4, _need(29, 1, 4), THREADS, 1])
  assert _plan(8, 1, 65, path=1, lds_max=0)[0] == EINVAL


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  assert _plan(8, 0, 512)[0] == 0
  for team in (-1, 3, 5, 6, 12, 100, 257, 512):
    assert _plan(8, 0, 512, team=team)[0] == EINVAL, team
  for S, perf, B in ((0, 0, 512), (-1, 0, 512), ((1 << 24) + 1, 0, 1), (8, 2, 512), (8, -1, 512),
                     (8, 0, 0), (8, 0, -4), (8, 0, 1 << 32),
                     (8, 0, (1 << 31) // 40 + 1),            # B * S * 5 >= 2^31, by one learner
                     (1 << 24, 0, 26)):
    assert _plan(S, perf, B)[0] == EINVAL, (S, perf, B)
  assert _plan(8, 0, (1 << 31) // 40)[0] == 0 and _plan(1 << 24, 0, 25)[0] == 0
  assert _plan(8, 0, 512, lds_max=-1)[0] == EINVAL
  assert _plan(8, 0, 512, path=3)[0] == EINVAL and _plan(8, 0, 512, path=-1)[0] == EINVAL
  assert _hip.lib.campx_wide_traces_plan(8, 0, 512, LDS_MAX, 0, 0, None) == EINVAL


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_traces_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)

  def learner(**kw):
    fields = dict(q=fake, traces=fake, alpha=fake, gamma=fake, epsilon=fake, lam=fake, reward_sum=fake,
                  perf_sum=None, episodes=fake, bad_count=None, bad_flag=None, seed=1, first_frame=0,
                  window=0, rule=0, path=0, reset_first=0, trace=0, team=0)
    fields.update(kw)
    return _hip.CampxTraceLearner(**fields)

  def call(spec=fake_spec, tables=vp(fake), st=state, l=None, B=512, T=4, **kw):
    l = learner(**kw) if l is None else l
    return f(spec, tables, st, ctypes.byref(l) if l is not False else None, B, T, None)

  # window = 0: refused before the spec is read (every call below that is not about the window
  # would reach the fake spec if it were not refused first)
  assert call() == EINVAL
  assert call(l=False) == EINVAL
  assert call(spec=None, window=2) == EINVAL and call(tables=None, window=2) == EINVAL
  for name in ('q', 'traces', 'alpha', 'gamma', 'epsilon', 'lam', 'reward_sum', 'episodes'):
    assert call(window=2, **{name: None}) == EINVAL, name
  for name in ('q', 'traces'):
    assert call(window=2, **{name: fake + 4}) == EINVAL and call(window=2, **{name: fake + 8}) == EINVAL
  for name in ('alpha', 'gamma', 'epsilon', 'lam', 'reward_sum', 'perf_sum', 'episodes', 'bad_count',
               'bad_flag'):
    assert call(window=2, **{name: fake + 2}) == EINVAL, name
  assert call(B=0, window=2) == EINVAL and call(T=0, window=2) == EINVAL
  assert call(first_frame=-1, window=2) == EINVAL
  assert call(rule=2, window=2) == EINVAL and call(path=3, window=2) == EINVAL
  assert call(trace=2, window=2) == EINVAL and call(trace=-1, window=2) == EINVAL
  # a spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), window=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert call(spec=by, B=410, window=2) == EINVAL                       # the element bound
  assert _plan(1 << 20, 0, 409, path=1)[0] == EINVAL and _plan(1 << 20, 0, 409, path=2)[0] == 0
  assert call(spec=by, B=409, window=2, path=1) == EINVAL
  assert call(spec=by, B=409, window=2, path=2, team=3) == EINVAL
  assert call(spec=by, B=409, window=2, path=2, team=512) == EINVAL
  assert call(spec=by, B=409, window=2, path=2, perf_sum=fake) == EINVAL


# ---------------------------------------------------------------- the reference itself

def _random_q(B, seed=0):
  return np.random.RandomState(seed).uniform(-1, 1, size=(B, 3, 5)).astype(F)


@pytest.mark.parametrize('kind', trace_ref.KINDS)
@pytest.mark.parametrize('rule', trace_ref.RULES)
def test_lam_zero_is_the_one_step_learner_bit_for_bit(rule, kind):
  B, T = 12, 40
  q = _random_q(B)
  kw = dict(alpha=0.3, gamma=0.8, epsilon=0.25, rule=rule, seed=0xfeedfacecafebeef, window=7)
  one = learn_ref.Learners(_Table, B, q)
  want = one.learn(T, **kw)
  # whatever the traces held: at lam = 0 the first decay clears them - but not before frame 0
  two = trace_ref.TraceLearners(_Table, B, q)
  got = two.learn_traces(T, lam=0.0, trace=kind, **kw)
  assert _same(one.q, two.q) and not _same(one.q, q)
  for k in ('reward_sum', 'perf_sum', 'episodes'):
    assert _same(want[k], got[k]), k
  assert np.array_equal(one.state, two.state) and np.array_equal(one.over, two.over)
  assert _same(one.ret, two.ret) and one.frame == two.frame
  assert not two.z.any()


def test_replacing_equals_accumulating_where_no_pair_repeats_inside_a_trace_s_life():
  """Greedy walks of the all-zero table from state 0: a0 to state 1, a0 again and the episode ends
  (traces zeroed) - no (state, action) is met twice within an episode; with random tables and
  exploration pairs repeat, and the two kinds part."""
  B, T = 4, 12
  a, r = (trace_ref.TraceLearners(_Table, B) for _ in range(2))
  kw = dict(lam=0.9, alpha=0.5, gamma=0.5, epsilon=0.0, reset_first=True, record=True)
  out = a.learn_traces(T, trace='accumulating', **kw)
  r.learn_traces(T, trace='replacing', **kw)
  assert out['states'][:4].T.tolist() == [[0, 1, 0, 1]] * B and not out['actions'].any()
  assert _same(a.q, r.q) and _same(a.z, r.z) and a.q.any()
  a, r = (trace_ref.TraceLearners(_Table, B, _random_q(B)) for _ in range(2))
  kw = dict(lam=0.9, alpha=0.5, gamma=0.9, epsilon=0.5, seed=3, rule='expected_sarsa')
  a.learn_traces(40, trace='accumulating', **kw)
  r.learn_traces(40, trace='replacing', **kw)
  assert not _same(a.q, r.q) and r.z.max() <= 1


class _TwoStates(object):
  """State 0: a0 -> state 1, the rest stay, reward 0.  State 1: a0 -> state 0, reward 1, DONE; the
  rest stay, reward 0."""
  n_states = 2
  st_next = np.array([[1, 0, 0, 0, 0], [0, 1, 1, 1, 1]], np.int32)
  st_reward = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], F)
  st_done = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], np.uint8)
  st_discount = (1.0 - st_done).astype(F)
  st_perf = np.zeros((2, 5), np.int8)


def test_three_frames_by_hand_the_cut_and_the_end_of_an_episode():
  """epsilon = 1, seed 18: the actions drawn are 0, 0, 1.  alpha = gamma = lam = 0.5, every trace 1
  to begin with, q[0] = [0, 1, 0, 0, 0], q[1] = [2, 0, 0, 0, 0]."""
  q = np.array([[[0, 1, 0, 0, 0], [2, 0, 0, 0, 0]]], F)
  L = trace_ref.TraceLearners(_TwoStates, 1, q, np.ones((1, 2, 5), F))
  kw = dict(lam=0.5, alpha=0.5, gamma=0.5, epsilon=1.0, seed=18)
  out = L.learn_traces(1, record=True, **kw)
  # frame 0: state 0, a0, old 0 is not the row's maximum 1: CUT, every trace 0.  target
  # 0 + (0.5 * 1) * max q[1] = 1, delta 1, step 0.5.  Bump z[0, 0] = 1: q[0, 0] = 0.5, nothing else
  # moves (the traces that were 1 are cut).  Decay c = (0.5 * 1) * 0.5: z[0, 0] = 0.25.
  assert out['actions'].tolist() == [[0]] and out['cut'].tolist() == [[True]]
  assert out['delta'].tolist() == [[1.0]] and out['step'].tolist() == [[0.5]]
  assert L.q.tolist() == [[[0.5, 1, 0, 0, 0], [2, 0, 0, 0, 0]]]
  assert L.z.tolist() == [[[0.25, 0, 0, 0, 0], [0, 0, 0, 0, 0]]]
  out = L.learn_traces(1, record=True, **kw)
  # frame 1: state 1, a0, old 2 is the maximum: no cut.  DONE: target 1, delta -1, step -0.5.
  # Bump z[1, 0] = 1.  Sweep: q[0, 0] = 0.5 + (-0.5 * 0.25) = 0.375, q[1, 0] = 1.5.  The episode
  # ended: every trace 0.
  assert out['states'].tolist() == [[1]] and out['actions'].tolist() == [[0]]
  assert out['cut'].tolist() == [[False]] and out['delta'].tolist() == [[-1.0]]
  assert L.q.tolist() == [[[0.375, 1, 0, 0, 0], [1.5, 0, 0, 0, 0]]]
  assert not L.z.any() and L.over.tolist() == [True] and out['episodes'].tolist() == [[1]]
  out = L.learn_traces(1, record=True, **kw)
  # frame 2: a new episode, state 0, a1, old 1 is the maximum: no cut; stays in state 0.  target
  # 0 + 0.5 * 1 (row 0 before the sweep), delta -0.5, step -0.25: q[0, 1] = 0.75, z[0, 1] = 0.25.
  assert out['states'].tolist() == [[0]] and out['actions'].tolist() == [[1]]
  assert out['cut'].tolist() == [[False]] and out['delta'].tolist() == [[-0.5]]
  assert L.q.tolist() == [[[0.375, 0.75, 0, 0, 0], [1.5, 0, 0, 0, 0]]]
  assert L.z.tolist() == [[[0, 0.25, 0, 0, 0], [0, 0, 0, 0, 0]]]
  assert L.state.tolist() == [0] and L.ret.tolist() == [0.0] and L.frame == 3
  # expected SARSA never cuts: frame 0 again, and the traces that were 1 move with (0, 0)
  L = trace_ref.TraceLearners(_TwoStates, 1, q, np.ones((1, 2, 5), F))
  out = L.learn_traces(1, record=True, rule='expected_sarsa', **kw)
  # bootstrap (0 * 2) + (1 * (2 * 0.2f)); z[0, 0] = 2 (accumulating), the rest 1
  b = F(F(2) * F(0.2))
  step = F(F(0.5) * F(F(0.5) * b))
  assert out['cut'].tolist() == [[False]] and out['step'][0, 0] == step
  assert L.q[0, 0, 0] == F(step * F(2)) and L.q[0, 1, 1] == step and L.q[0, 0, 1] == F(F(1) + step)
  assert L.z[0, 0].tolist() == [0.5, 0.25, 0.25, 0.25, 0.25]


def test_an_entry_with_a_zero_trace_keeps_its_bits_and_a_nan_trace_counts():
  q = np.array([[[0.5, -0.0, 0, 0, 0], [2, -0.0, 0, 0, 0]]], F)
  z = np.zeros((1, 2, 5), F)
  z[0, 1, 2], z[0, 1, 3] = -0.0, np.nan
  L = trace_ref.TraceLearners(_TwoStates, 1, q, z)
  L.learn_traces(1, lam=0.5, alpha=0.5, gamma=0.5, epsilon=0.0, rule='expected_sarsa')
  assert np.signbit(L.q[0, 0, 1]) and np.signbit(L.q[0, 1, 1]) and L.q[0, 1, 2] == 0
  assert not np.signbit(L.q[0, 1, 2]) and np.isnan(L.q[0, 1, 3]) and np.isnan(L.z[0, 1, 3])
  assert L.q[0, 0, 0] != F(0.5) and np.signbit(L.z[0, 1, 2])        # 0.25 * -0 is -0


def test_reset_first_zeroes_the_traces_of_good_learners_only():
  B = 4
  lam = np.array([0.5, np.nan, 1.5, 1.0], F)
  assert trace_ref.bad_learners(np.full(B, 0.5, F), np.full(B, 0.5, F), np.full(B, 0.1, F),
                                lam).tolist() == [False, True, True, False]
  q, z = _random_q(B), np.abs(_random_q(B, seed=1))
  L = trace_ref.TraceLearners(_Table, B, q, z)
  out = L.learn_traces(1, lam=lam, alpha=0.5, gamma=0.5, epsilon=0.1, rule='expected_sarsa',
                       reset_first=True, record=True)
  assert out['bad'] == 2 and out['actions'][0, 1:3].tolist() == [4, 4]
  assert _same(L.q[1:3], q[1:3]) and _same(L.z[1:3], z[1:3])
  for e in (0, 3):
    assert np.count_nonzero(L.z[e]) == 1 and np.count_nonzero(L.q[e] != q[e]) == 1


@pytest.mark.parametrize('kind', trace_ref.KINDS)
@pytest.mark.parametrize('rule', trace_ref.RULES)
def test_two_calls_learn_what_one_call_learns(rule, kind):
  B, T1, T2 = 9, 7, 11
  q = _random_q(B, seed=2)
  kw = dict(lam=0.8, trace=kind, alpha=0.3, gamma=0.8, epsilon=0.25, rule=rule, seed=77)
  one, two = (trace_ref.TraceLearners(_Table, B, q) for _ in range(2))
  one.learn_traces(T1 + T2, **kw)
  two.learn_traces(T1, **kw)
  assert two.z.any()
  two.learn_traces(T2, **kw)
  assert _same(one.q, two.q) and _same(one.z, two.z) and not _same(one.q, q)
  assert np.array_equal(one.state, two.state) and _same(one.ret, two.ret)
