"""`campx_wide_learn_plan()` - pure host arithmetic - against the header's account of the bytes,
the refusals of `campx_wide_learn_launch()` that are decided before a device is touched, the op's
schema, and the numpy learners of tests/learner_reference.py against a table worked by hand and
against `policy_reference.PolicyWalker`.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import learner_reference as learn_ref
import policy_reference as ref
from test_population_cpu import _Table, _same, _valid_spec

F = np.float32
LDS_MAX = 144 * 1024
THREADS = 256
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h


def _plan(S, perf, B, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_learn_plan(S, perf, B, lds_max, path, out)
  return code, list(out)


def _table_bytes(S, perf):
  """The header's account: the entries and - hidden performance - its bytes, each rounded up to 16."""
  up = lambda x: (x + 15) // 16 * 16
  return up(40 * S) + (up(5 * S) if perf else 0)


def _need(S, perf):
  """... plus, on path 1, the Q-tables of a workgroup's 256 learners, 20 bytes per state each."""
  return _table_bytes(S, perf) + THREADS * S * 20


def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  assert 'campx_wide_learn_plan' in _hip.EXPORTS and 'campx_wide_learn_launch' in _hip.EXPORTS
  assert hasattr(_hip.lib, 'campx_wide_learn_plan') and hasattr(_hip.lib, 'campx_wide_learn_launch')
  assert 'wide_learn' in _hip.OP_NAMES
  assert _hip.LEARN_RULES == {'q': 0, 'expected_sarsa': 1}
  assert _hip.config_get('wide_lds_max') == LDS_MAX
  s = str(torch.ops.campx.wide_learn.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor(d!) q', 'Tensor alpha',
               'Tensor gamma', 'Tensor epsilon', 'int rule', 'int seed', 'int first_frame',
               'int frames', 'int window', 'Tensor(e!) reward_sum', 'Tensor(f!)? perf_sum',
               'Tensor(g!) episodes', 'Tensor(h!)? bad_count', 'Tensor(i!)? bad_flag',
               'bool reset_first', 'int path=0'):
    assert part in s, s
  assert s.endswith('-> ()')


def test_the_surface_names_both_methods():
  from campx_amd import engine, wide
  for name in ('learn_tabular', 'learner_buffers'):
    assert name in wide.STATE_TABLE_ONLY and callable(getattr(wide.WideGame, name))
    assert getattr(engine.Engine, name).__doc__
  doc = wide.WideGame.learn_tabular.__doc__
  assert 'SARSA proper' in doc and 'atomics' in doc


@pytest.mark.parametrize('perf', [0, 1])
@pytest.mark.parametrize('S', [1, 8, 159])
def test_plan_against_the_byte_account(S, perf):
  need, table = _need(S, perf), _table_bytes(S, perf)
  fits = need <= LDS_MAX
  assert fits == (S < 159)
  for B in (1, 255, 256, 65536):
    assert _plan(S, perf, B) == (0, [1, need, THREADS, 1] if fits else [2, table, THREADS, 1]), (S, B)
    # both sides of the bound, and the forced paths
    assert _plan(S, perf, B, lds_max=need) == (0, [1, need, THREADS, 1])
    assert _plan(S, perf, B, lds_max=need - 1) == (0, [2, table, THREADS, 1])
    assert _plan(S, perf, B, lds_max=need, path=2) == (0, [2, table, THREADS, 1])
    assert _plan(S, perf, B, lds_max=need, path=1) == (0, [1, need, THREADS, 1])
    assert _plan(S, perf, B, lds_max=need - 1, path=1)[0] == EINVAL
    # the entries stay in LDS on the global path exactly when they alone fit
    assert _plan(S, perf, B, lds_max=table, path=2) == (0, [2, table, THREADS, 1])
    assert _plan(S, perf, B, lds_max=table - 1, path=2) == (0, [2, 0, THREADS, 0])
    assert _plan(S, perf, B, lds_max=table - 1) == (0, [2, 0, THREADS, 0])


def test_the_sizes_the_header_names():
  assert _need(8, 1) == 320 + 48 + 40960                 # the boat race: three workgroups to a CU
  assert _plan(8, 1, 65536)[1][:2] == [1, 41328]
  assert _plan(159, 0, 65536) == (0, [2, 6368, THREADS, 1])        # the maze: q through L1 / L2
  assert _plan(159, 0, 65536, path=1)[0] == EINVAL


@pytest.mark.parametrize('perf', [0, 1])
def test_the_largest_table_that_fits_and_the_next(perf):
  S = 1
  while _need(S + 1, perf) <= LDS_MAX:
    S += 1
  assert S == 28
  assert _plan(S, perf, 512) == (0, [1, _need(S, perf), THREADS, 1])
  assert _plan(S + 1, perf, 512) == (0, [2, _table_bytes(S + 1, perf), THREADS, 1])
  assert _plan(S + 1, perf, 512, path=1)[0] == EINVAL and _plan(S, perf, 512, path=1)[0] == 0
  assert _plan(S, perf, 512, path=2) == (0, [2, _table_bytes(S, perf), THREADS, 1])


def test_wide_lds_max_zero_forces_global_and_path_1_is_refused_then():
  for B in (512, 64):
    assert _plan(8, 1, B, lds_max=0) == (0, [2, 0, THREADS, 0])
    assert _plan(8, 1, B, lds_max=0, path=2) == (0, [2, 0, THREADS, 0])
    assert _plan(8, 1, B, lds_max=0, path=1)[0] == EINVAL


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  assert _plan(8, 0, 512)[0] == 0
  for S, perf, B in ((0, 0, 512), (-1, 0, 512), ((1 << 24) + 1, 0, 1), (8, 2, 512), (8, -1, 512),
                     (8, 0, 0), (8, 0, -4), (8, 0, 1 << 32),
                     (8, 0, (1 << 31) // 40 + 1),            # B * S * 5 >= 2^31, by one learner
                     (1 << 24, 0, 26)):
    assert _plan(S, perf, B)[0] == EINVAL, (S, perf, B)
  assert ((1 << 31) // 40) * 40 < 1 << 31 and _plan(8, 0, (1 << 31) // 40)[0] == 0
  assert (1 << 24) * 5 * 25 < 1 << 31 and _plan(1 << 24, 0, 25)[0] == 0
  assert _plan(8, 0, 512, lds_max=-1)[0] == EINVAL
  assert _plan(8, 0, 512, path=3)[0] == EINVAL and _plan(8, 0, 512, path=-1)[0] == EINVAL
  assert _hip.lib.campx_wide_learn_plan(8, 0, 512, LDS_MAX, 0, None) == EINVAL


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_learn_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)

  def learner(**kw):
    fields = dict(q=fake, alpha=fake, gamma=fake, epsilon=fake, reward_sum=fake, perf_sum=None,
                  episodes=fake, bad_count=None, bad_flag=None, seed=1, first_frame=0, window=0,
                  rule=0, path=0, reset_first=0)
    fields.update(kw)
    return _hip.CampxLearner(**fields)

  def call(spec=fake_spec, tables=vp(fake), st=state, l=None, B=512, T=4, **kw):
    l = learner(**kw) if l is None else l
    return f(spec, tables, st, ctypes.byref(l) if l is not False else None, B, T, None)

  # window = 0: refused before the spec is read (every call below that is not about the window
  # would reach the fake spec if it were not refused first)
  assert call() == EINVAL
  assert call(window=-1) == EINVAL
  assert call(spec=None, window=2) == EINVAL and call(tables=None, window=2) == EINVAL
  assert call(l=False) == EINVAL
  assert call(st=_hip.CampxState(pos=None, done=fake), window=2) == EINVAL
  assert call(st=_hip.CampxState(pos=fake, done=None), window=2) == EINVAL
  for name in ('q', 'alpha', 'gamma', 'epsilon', 'reward_sum', 'episodes'):
    assert call(window=2, **{name: None}) == EINVAL, name
  assert call(B=0, window=2) == EINVAL and call(T=0, window=2) == EINVAL
  assert call(B=1 << 32, window=2) == EINVAL
  assert call(first_frame=-1, window=2) == EINVAL
  assert call(first_frame=(1 << 63) - 4, window=2) == EINVAL            # first_frame + T past 2^63 - 1
  assert call(q=fake + 4, window=2) == EINVAL and call(q=fake + 8, window=2) == EINVAL
  for name in ('alpha', 'gamma', 'epsilon', 'reward_sum', 'perf_sum', 'episodes', 'bad_count', 'bad_flag'):
    assert call(window=2, **{name: fake + 2}) == EINVAL, name
  assert call(st=_hip.CampxState(pos=fake + 2, done=fake), window=2) == EINVAL
  assert call(st=_hip.CampxState(pos=fake, done=fake, ret=fake + 1), window=2) == EINVAL
  assert call(rule=2, window=2) == EINVAL and call(rule=-1, window=2) == EINVAL
  assert call(path=3, window=2) == EINVAL and call(path=-1, window=2) == EINVAL
  # A spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict.
  # That it does pass: an all-zero spec is refused as a spec, this one is not.
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), window=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert (1 << 20) * 5 * 410 >= 1 << 31 > (1 << 20) * 5 * 409
  assert call(spec=by, B=410, window=2) == EINVAL                       # the element bound
  assert call(spec=by, B=410, window=2, path=2) == EINVAL
  # the control: only the plan knows that 2^20 states do not fit the LDS of a workgroup
  assert _plan(1 << 20, 0, 409, path=1)[0] == EINVAL and _plan(1 << 20, 0, 409, path=2)[0] == 0
  assert call(spec=by, B=409, window=2, path=1) == EINVAL
  # perf_sum for a game without hidden performance
  assert call(spec=by, B=409, window=2, path=2, perf_sum=fake) == EINVAL


# ---------------------------------------------------------------- the reference itself

def _q(rows):
  """[1, 3, 5] from three rows."""
  return np.array([rows], F)


def test_q_learning_by_hand_ties_done_frames_and_windows():
  """epsilon = 0: greedy.  All-zero rows tie: action 0.  State 0 a0 -> state 1, reward 1; state 1
  a0 -> state 2, reward 1, DONE: its target is the reward alone, and the next frame starts from
  row 0."""
  L = learn_ref.Learners(_Table, 1)
  out = L.learn(4, alpha=0.5, gamma=0.5, epsilon=0.0, window=3, record=True, reset_first=True)
  assert out['states'].T.tolist() == [[0, 1, 0, 1]] and out['actions'].T.tolist() == [[0, 0, 0, 0]]
  # frame 0: target 1 + 0.5 * max q[1] = 1        -> q[0, 0] = 0.5
  # frame 1: done, target 1                        -> q[1, 0] = 0.5
  # frame 2: target 1 + 0.5 * 0.5 = 1.25           -> q[0, 0] = 0.5 + 0.5 * 0.75 = 0.875
  # frame 3: done, target 1                        -> q[1, 0] = 0.5 + 0.5 * 0.5 = 0.75
  assert L.q.tolist() == [[[0.875, 0, 0, 0, 0], [0.75, 0, 0, 0, 0], [0, 0, 0, 0, 0]]]
  assert out['reward_sum'].tolist() == [[3.0], [1.0]] and out['episodes'].tolist() == [[1], [1]]
  assert out['perf_sum'].tolist() == [[0], [0]] and out['bad'] == 0 and not out['explored'].any()
  assert L.state.tolist() == [2] and L.over.tolist() == [True] and L.ret.tolist() == [2.0]
  assert L.frame == 4 and out['reward_sum'].dtype == F and out['episodes'].dtype == np.int32


def test_a_frame_that_stays_in_its_state_bootstraps_from_the_row_before_the_update():
  """State 0 a2 -> state 0, reward -1: n == s, and the bootstrap is max q[0] as it stood."""
  L = learn_ref.Learners(_Table, 1, _q([[0, 0, 1, 0, 0], [0] * 5, [0] * 5]))
  out = L.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0, record=True)
  # target -1 + 0.5 * 1 (not 0.5 * the updated 0.25) = -0.5; delta -1.5; q = 1 - 0.75
  assert out['actions'].tolist() == [[2]] and L.q[0, 0].tolist() == [0, 0, 0.25, 0, 0]
  out = L.learn(2, alpha=0.5, gamma=0.5, epsilon=0.0, record=True)
  # target -1 + 0.5 * 0.25 = -0.875; delta -1.125; q = 0.25 - 0.5625 = -0.3125; then zeros tie: a0
  assert out['actions'].T.tolist() == [[2, 0]] and L.q[0, 0, 2] == F(-0.3125)
  assert L.q[0, 0, 0] == F(0.5) and L.state.tolist() == [1]


def test_a_reward_of_none_counts_as_zero():
  """State 0 a3 -> state 1, reward None."""
  L = learn_ref.Learners(_Table, 1, _q([[0, 0, 0, 1, 0], [0, 0, 2, 0, 0], [0] * 5]))
  out = L.learn(1, alpha=0.25, gamma=0.5, epsilon=0.0, record=True)
  # target 0 + 0.5 * 2 = 1; delta 0; q stays 1
  assert out['actions'].tolist() == [[3]] and L.q[0, 0].tolist() == [0, 0, 0, 1, 0]
  assert out['reward_sum'].tolist() == [[0.0]] and L.ret.tolist() == [0.0] and L.state.tolist() == [1]
  L = learn_ref.Learners(_Table, 1, _q([[0, 0, 0, 1, 0], [0, 0, 4, 0, 0], [0] * 5]))
  L.learn(1, alpha=0.25, gamma=0.5, epsilon=0.0)
  assert L.q[0, 0, 3] == F(1.25) and not np.isnan(L.q).any()       # target 2, delta 1


def test_expected_sarsa_by_hand():
  """epsilon = 1 always explores and bootstraps from the mean: rows [1 .. 5] have m = 15 * 0.2f = 3
  in float32.  epsilon = 0 bootstraps from the maximum alone, as Q-learning does."""
  rows = np.tile(np.arange(1, 6, dtype=F), (1, 3, 1))
  L = learn_ref.Learners(_Table, 1, rows)
  out = L.learn(1, alpha=0.5, gamma=0.5, epsilon=1.0, rule='expected_sarsa', seed=5, record=True)
  assert out['explored'].all()
  a = int(out['actions'][0, 0])
  x0, x1 = learn_ref.words(5, [0], 0)
  assert a == ((int(x1[0]) >> 8) * 5) >> 24
  r = 0.0 if np.isnan(_Table.st_reward[0, a]) else float(_Table.st_reward[0, a])
  target = r + 0.5 * 3.0                        # (no entry of state 0 ends the episode)
  assert L.q[0, 0, a] == F((a + 1) + 0.5 * (target - (a + 1)))
  for rule in learn_ref.RULES:
    L = learn_ref.Learners(_Table, 1, rows)
    L.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0, rule=rule)
    # greedy: a4 of state 0 -> state 0, reward 0; target 0.5 * 5; delta -2.5
    assert L.q[0, 0].tolist() == [1, 2, 3, 4, 3.75], rule


def test_the_random_words_are_a_stream_of_their_own():
  """Counter word 3 is 1; frames 2g and 2g + 1 share a block, frame 2g + 2 does not."""
  env = np.arange(4, dtype=np.uint64)
  key = np.array([7, 0], np.uint32)
  for f in (0, 1, 6, 7, (1 << 40) + 1):
    g = f >> 1
    counter = np.stack([env, np.full_like(env, g & 0xffffffff), np.full_like(env, g >> 32),
                        np.ones_like(env)], axis=-1).astype(np.uint32)
    block = ref.philox4x32_10(counter, key)
    x0, x1 = learn_ref.words(7, env, f)
    assert np.array_equal(x0, block[:, 2 * (f & 1)]) and np.array_equal(x1, block[:, 2 * (f & 1) + 1])
  # rollout_policy()'s word of the same seed, learner and block is another
  assert not np.array_equal(learn_ref.words(7, env, 0)[0], ref.words(7, env, 0))


def _random_q(B, seed=0):
  return np.random.RandomState(seed).uniform(-1, 1, size=(B, 3, 5)).astype(F)


@pytest.mark.parametrize('rule', learn_ref.RULES)
def test_alpha_zero_leaves_q_bit_identical(rule):
  q = _random_q(16)
  L = learn_ref.Learners(_Table, 16, q)
  L.learn(40, alpha=0.0, gamma=0.9, epsilon=0.3, rule=rule, seed=3)
  assert _same(L.q, q)


def test_alpha_and_epsilon_zero_walk_the_one_hot_greedy_policy():
  B, T = 8, 33
  q = np.tile(_random_q(1, seed=4), (B, 1, 1))
  greedy = plan_greedy(q[0])
  policy = np.zeros((3, 5), F)
  policy[np.arange(3), greedy] = 1.0
  L, walker = learn_ref.Learners(_Table, B, q), ref.PolicyWalker(_Table, B)
  out = L.learn(T, alpha=0.0, gamma=0.9, epsilon=0.0, seed=9, record=True, reset_first=True)
  want = walker.rollout(policy, T, seed=9, reset_first=True)
  assert np.array_equal(out['actions'], want['actions']) and np.array_equal(out['states'], want['states'])
  assert np.array_equal(L.state, walker.state) and np.array_equal(L.over, walker.over)
  assert _same(L.ret, walker.ret)
  assert np.array_equal(out['episodes'][0], want['done'].sum(0).astype(np.int32))
  assert np.array_equal(out['perf_sum'][0], want['perf'].astype(np.int32).sum(0))


def plan_greedy(q):
  import planning_reference
  return planning_reference.reduce_greedy(q)[1].astype(np.int64)


def test_epsilon_zero_never_explores_and_epsilon_one_always_does():
  B, T = 32, 24
  eps = np.where(np.arange(B) % 2 == 0, F(0), F(1))
  L = learn_ref.Learners(_Table, B, _random_q(B))
  out = L.learn(T, alpha=0.1, gamma=0.9, epsilon=eps, seed=1, record=True)
  assert not out['explored'][:, 0::2].any() and out['explored'][:, 1::2].all()
  # the explorers' actions are the random ones, and all five turn up
  for t in (0, 1, 23):
    x1 = learn_ref.words(1, np.arange(B), t)[1]
    assert np.array_equal(out['actions'][t, 1::2], (((x1 >> 8).astype(np.uint64) * 5) >> 24)[1::2])
  assert set(np.unique(out['actions'][:, 1::2])) == {0, 1, 2, 3, 4}


def test_bad_learners_take_action_4_and_keep_their_tables():
  B = 6
  q = _random_q(B)
  alpha = np.array([0.5, np.nan, 0.5, 0.5, 0.5, 0.5], F)
  gamma = np.array([0.9, 0.9, np.inf, 0.9, 0.9, 0.9], F)
  eps = np.array([0.2, 0.2, 0.2, 1.5, -0.1, 0.2], F)
  assert learn_ref.bad_learners(alpha, gamma, eps).tolist() == [False, True, True, True, True, False]
  L = learn_ref.Learners(_Table, B, q)
  out = L.learn(10, alpha=alpha, gamma=gamma, epsilon=eps, seed=2, record=True)
  assert out['bad'] == 4 and (out['actions'][:, 1:5] == 4).all()
  assert _same(L.q[1:5], q[1:5]) and not _same(L.q[0], q[0]) and not _same(L.q[5], q[5])
  # the neighbours learn what they learn alone (the counter is the absolute learner)
  alone = learn_ref.Learners(_Table, B, q)
  alone.learn(10, alpha=0.5, gamma=0.9, epsilon=0.2, seed=2)
  assert _same(L.q[[0, 5]], alone.q[[0, 5]])


@pytest.mark.parametrize('rule', learn_ref.RULES)
@pytest.mark.parametrize('T1', [7, 8])
def test_two_calls_learn_what_one_call_learns(T1, rule):
  B, T2 = 9, 11
  q = _random_q(B, seed=T1)
  kw = dict(alpha=0.3, gamma=0.8, epsilon=0.25, rule=rule, seed=0xfeedfacecafebeef)
  one, two = learn_ref.Learners(_Table, B, q), learn_ref.Learners(_Table, B, q)
  whole = one.learn(T1 + T2, window=T1, **kw)
  first = two.learn(T1, **kw)
  second = two.learn(T2, window=T1, **kw)
  assert _same(one.q, two.q) and not _same(one.q, q)
  assert np.array_equal(one.state, two.state) and np.array_equal(one.over, two.over)
  assert _same(one.ret, two.ret) and one.frame == two.frame == T1 + T2
  # windows count from each call's own frame 0
  assert _same(whole['reward_sum'][0], first['reward_sum'][0])
  assert _same(whole['reward_sum'][1], second['reward_sum'][0])
  assert np.array_equal(whole['episodes'][1:], second['episodes'])
  # an explicit first_frame, high counter word in use
  a, b = learn_ref.Learners(_Table, B, q), learn_ref.Learners(_Table, B, q)
  a.learn(5, first_frame=(1 << 40) + 1, **kw)
  b.learn(2, first_frame=(1 << 40) + 1, **kw)
  b.learn(3, **kw)
  assert _same(a.q, b.q) and a.frame == b.frame == (1 << 40) + 6
