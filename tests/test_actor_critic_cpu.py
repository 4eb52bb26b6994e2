"""The exponent rule of the actor-critic learners against float64 `exp` and against its torch
restatement `campx_amd.returns.softmax_weights()`; `campx_wide_actor_plan()` - pure host arithmetic -
against the header's account of the bytes; the refusals of `campx_wide_actor_launch()` that are
decided before a device is touched; the op's schema; and the numpy learners of
tests/actor_critic_reference.py on their own: two frames by hand, two calls against one, bad rows and
bad learners, and one check that the learners learn.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import actor_critic_reference as ac_ref
import policy_reference as ref
from test_population_cpu import _Table, _same, _valid_spec
from test_trace_learner_cpu import _TwoStates

F = np.float32
LDS_MAX = 144 * 1024
THREADS = 256
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h

# The largest relative error of the rule against float64 exp(d) MEASURED over the inputs of
# _rule_inputs() is 3.74e-6 (at d = -68.26: almost all of it is the rounding of t = d * log2e at
# large |d|; 2.4e-7 for |d| < 1).  The bound is twice that.
MEASURED_REL_ERROR = 3.74e-6
REL_ERROR_BOUND = 7.5e-6


def _rule_inputs():
  """6 M values of d in [-69, 0]: half uniform, half log-uniform from -1e-6 down."""
  rs = np.random.RandomState(0)
  return np.concatenate([-rs.uniform(0, 69, 3000000),
                         -np.exp(rs.uniform(np.log(1e-6), np.log(69), 3000000))]).astype(F)


def test_the_weights_rule_against_float64_exp():
  d = _rule_inputs()
  assert d.min() >= -69 and d.max() < 0
  w = ac_ref.weight_of(d)
  exact = np.exp(d.astype(np.float64))
  rel = np.abs(w.astype(np.float64) - exact) / exact
  print('largest relative error {:.4g} at d = {!r}'.format(rel.max(), float(d[rel.argmax()])))
  assert rel.max() <= REL_ERROR_BOUND
  assert rel.max() >= MEASURED_REL_ERROR / 2         # (the note beside the bound is not stale)
  assert w.max() < 1 and w.min() > 0
  # d = 0 and -0.0: exactly 1
  assert _same(ac_ref.weight_of(np.array([0.0, -0.0], F)), np.ones(2, F))
  # both sides of the cut t < -100: the last d whose t is not below it, and the next float32 down
  cut = F(-100.0) / ac_ref.LOG2E
  at = [x for x in (np.nextafter(cut, F(0)), cut, np.nextafter(cut, F(-np.inf)),
                    np.nextafter(np.nextafter(cut, F(-np.inf)), F(-np.inf)))]
  t = [F(x * ac_ref.LOG2E) for x in at]
  assert t[0] >= -100 and t[-1] < -100
  for x, tt in zip(at, t):
    got = float(ac_ref.weight_of(F(x)))
    if tt < -100:
      assert got == 0.0 and not np.signbit(F(got))
    else:
      assert abs(got - np.exp(float(x))) / np.exp(float(x)) <= REL_ERROR_BOUND and got >= 2.0 ** -101
  below = np.array([-69.4, -70, -100, -1e4, -3e38, -np.inf], F)
  assert _same(ac_ref.weight_of(below), np.zeros(6, F))


def _rows_with_edges():
  rs = np.random.RandomState(1)
  rows = rs.uniform(-8, 8, size=(4096, 5)).astype(F)
  rows[:256] *= F(20)                                   # spreads beyond the cut
  rows[0] = [0, 0, 0, 0, 0]
  rows[1] = [1, -np.inf, 1, -np.inf, -0.0]              # -inf is good: weight 0
  rows[2] = [np.nan, 0, 0, 0, 0]
  rows[3] = [0, 0, np.nan, 0, 0]
  rows[4] = [0, np.inf, 0, 0, 0]
  rows[5] = [-np.inf] * 5
  rows[6] = [3e38, -3e38, 0, 1, 2]                      # d overflows to -inf: weight 0
  rows[7] = [0, -69.3, -69.4, -200, 5]
  rows[8] = [-0.0, 0.0, -0.0, 0.0, -0.0]
  return rows


def test_rows_good_and_bad_and_the_torch_helper_gives_the_same_bits():
  import torch
  from campx_amd import returns
  rows = _rows_with_edges()
  w, good = ac_ref.softmax_weights(rows)
  assert good[:9].tolist() == [True, True, False, False, False, False, True, True, True]
  assert _same(w[0], np.ones(5, F)) and _same(w[8], np.ones(5, F))
  assert w[1].tolist() == [1, 0, 1, 0, float(ac_ref.weight_of(F(-1)))]
  for bad in (2, 3, 4, 5):
    assert _same(w[bad], np.zeros(5, F))
  assert w[6].tolist()[:2] == [1, 0] and w[7][4] == 1 and w[7][3] == 0
  # every good row: the maximum's weight is 1, none is larger, the total lies in [1, 5] and passes
  # the sampler's test; a bad row fails it
  c, bad_for_sampler = ref.thresholds(w)
  assert np.array_equal(bad_for_sampler, ~good)
  assert (w[good].max(axis=1) == 1).all() and (c[good, 4] >= 1).all() and (c[good, 4] <= 5).all()
  assert (w >= 0).all()
  got = returns.softmax_weights(torch.from_numpy(rows))
  assert got.dtype == torch.float32 and got.shape == (4096, 5)
  assert _same(got.numpy(), w)
  # any leading shape, and a tensor that requires grad is detached
  lead = torch.from_numpy(rows[:24].reshape(2, 3, 4, 5)).requires_grad_()
  out = returns.softmax_weights(lead)
  assert not out.requires_grad and _same(out.numpy().reshape(24, 5), w[:24])
  # the rule's own inputs through the helper: d against a maximum of 0 in the row
  d = _rule_inputs()[::97]
  wide = np.zeros((len(d), 5), F)
  wide[:, 3] = d
  assert _same(returns.softmax_weights(torch.from_numpy(wide)).numpy()[:, 3], ac_ref.weight_of(d))
  for wrong in (rows, torch.zeros((3, 4)), torch.zeros((3, 5), dtype=torch.float64), torch.zeros(())):
    with pytest.raises(ValueError):
      returns.softmax_weights(wrong)


def test_the_constants_are_the_nearest_floats():
  import math
  from campx_amd import returns
  assert float(ac_ref.LOG2E) == float(F(1 / math.log(2))) == returns.SOFTMAX_LOG2E
  for n, c in enumerate(ac_ref.POLY):
    assert float(c) == float(F(math.log(2) ** n / math.factorial(n))) == returns.SOFTMAX_POLY[n]
  assert returns.SOFTMAX_CUT == float(ac_ref.CUT) == -100.0


# ---------------------------------------------------------------- plan and launcher

def _plan(S, perf, B, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_actor_plan(S, perf, B, lds_max, path, out)
  return code, list(out)


def _table_bytes(S, perf):
  up = lambda x: (x + 15) // 16 * 16
  return up(40 * S) + (up(5 * S) if perf else 0)


def _need(S, perf):
  """The header's account of path 1: the table, and per learner 20 bytes of preferences and 4 of
  values a state."""
  return _table_bytes(S, perf) + THREADS * S * 24


def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  for name in ('campx_wide_actor_plan', 'campx_wide_actor_launch'):
    assert name in _hip.EXPORTS and hasattr(_hip.lib, name)
  assert 'wide_learn_actor' in _hip.OP_NAMES
  s = str(torch.ops.campx.wide_learn_actor.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor(d!) prefs',
               'Tensor(e!) values', 'Tensor alpha_actor', 'Tensor alpha_critic', 'Tensor gamma',
               'int seed', 'int first_frame', 'int frames', 'int window', 'Tensor(f!) reward_sum',
               'Tensor(g!)? perf_sum', 'Tensor(h!) episodes', 'Tensor(i!)? bad_count',
               'Tensor(j!)? bad_rows', 'Tensor(k!)? bad_flag', 'bool reset_first', 'int path=0'):
    assert part in s, s
  assert s.endswith('-> ()')


def test_the_surface_names_the_method_and_what_is_not_offered():
  from campx_amd import engine, returns, wide
  assert 'learn_actor_critic' in wide.STATE_TABLE_ONLY
  assert callable(wide.WideGame.learn_actor_critic) and engine.Engine.learn_actor_critic.__doc__
  doc = wide.WideGame.learn_actor_critic.__doc__
  for word in ('NOT offered', 'REINFORCE', 'lambda-traces', 'entropy bonus', 'temperature', 'shared form',
               'softmax_weights', 'NOT `exp`'):
    assert word in doc, word
  assert 'not `exp`' in returns.softmax_weights.__doc__


@pytest.mark.parametrize('perf', [0, 1])
def test_both_sides_of_the_path_1_bound(perf):
  """144 KiB: preferences and values of 256 learners fit beside the table up to 23 states."""
  assert _need(23, perf) <= LDS_MAX < _need(24, perf)
  for B in (1, 65, 65536):
    assert _plan(23, perf, B) == (0, [1, _need(23, perf), THREADS, 1])
    assert _plan(24, perf, B) == (0, [2, _table_bytes(24, perf), THREADS, 1])
  assert _plan(24, perf, 65, path=1)[0] == EINVAL
  # the same bound, moved by the setting: one byte less and the learners go through L1 / L2
  need = _need(23, perf)
  assert _plan(23, perf, 65, lds_max=need)[1][:2] == [1, need]
  assert _plan(23, perf, 65, lds_max=need - 1)[1][:2] == [2, _table_bytes(23, perf)]
  assert _plan(23, perf, 65, lds_max=need - 1, path=1)[0] == EINVAL
  assert _plan(24, perf, 65, lds_max=_need(24, perf))[1][:2] == [1, _need(24, perf)]


def test_the_games_words_and_forced_paths():
  assert _need(8, 1) == 320 + 48 + 256 * 192
  assert _plan(8, 1, 65536) == (0, [1, 320 + 48 + 49152, THREADS, 1])          # the boat race
  assert _plan(159, 0, 65536) == (0, [2, 6368, THREADS, 1])                    # the maze
  assert _plan(470, 0, 65536) == (0, [2, 18800, THREADS, 1])                   # pickups
  assert _plan(1 << 16, 0, 8) == (0, [2, 0, THREADS, 0])                       # not even the entries fit
  table = _table_bytes(8, 1)
  assert _plan(8, 1, 65, path=1) == (0, [1, _need(8, 1), THREADS, 1])
  assert _plan(8, 1, 65, path=2) == (0, [2, table, THREADS, 1])
  assert _plan(8, 1, 65, path=2, lds_max=table - 1) == (0, [2, 0, THREADS, 0])
  assert _plan(8, 1, 65, lds_max=0) == (0, [2, 0, THREADS, 0])
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
  assert _hip.lib.campx_wide_actor_plan(8, 0, 512, LDS_MAX, 0, None) == EINVAL


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_actor_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)

  def learner(**kw):
    fields = dict(prefs=fake, values=fake, alpha_actor=fake, alpha_critic=fake, gamma=fake,
                  reward_sum=fake, perf_sum=None, episodes=fake, bad_count=None, bad_rows=None,
                  bad_flag=None, seed=1, first_frame=0, window=0, path=0, reset_first=0)
    fields.update(kw)
    return _hip.CampxActorLearner(**fields)

  def call(spec=fake_spec, tables=vp(fake), st=state, l=None, B=512, T=4, **kw):
    l = learner(**kw) if l is None else l
    return f(spec, tables, st, ctypes.byref(l) if l is not False else None, B, T, None)

  # window = 0: refused before the spec is read (every call below that is not about the window
  # would reach the fake spec if it were not refused first)
  assert call() == EINVAL
  assert call(l=False) == EINVAL
  assert call(spec=None, window=2) == EINVAL and call(tables=None, window=2) == EINVAL
  for name in ('prefs', 'values', 'alpha_actor', 'alpha_critic', 'gamma', 'reward_sum', 'episodes'):
    assert call(window=2, **{name: None}) == EINVAL, name
  for name in ('prefs', 'values'):
    assert call(window=2, **{name: fake + 4}) == EINVAL and call(window=2, **{name: fake + 8}) == EINVAL
  for name in ('alpha_actor', 'alpha_critic', 'gamma', 'reward_sum', 'perf_sum', 'episodes',
               'bad_count', 'bad_rows', 'bad_flag'):
    assert call(window=2, **{name: fake + 2}) == EINVAL, name
  assert call(B=0, window=2) == EINVAL and call(T=0, window=2) == EINVAL
  assert call(first_frame=-1, window=2) == EINVAL and call(path=3, window=2) == EINVAL
  assert call(first_frame=(1 << 63) - 4, window=2) == EINVAL
  # a spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), window=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert call(spec=by, B=410, window=2) == EINVAL                       # the element bound
  assert _plan(1 << 20, 0, 409, path=1)[0] == EINVAL and _plan(1 << 20, 0, 409, path=2)[0] == 0
  assert call(spec=by, B=409, window=2, path=1) == EINVAL
  assert call(spec=by, B=409, window=2, path=2, perf_sum=fake) == EINVAL   # a game without perf


# ---------------------------------------------------------------- the reference itself

def _random_tables(B, S=3, seed=0):
  rs = np.random.RandomState(seed)
  return rs.uniform(-2, 2, size=(B, S, 5)).astype(F), rs.uniform(-1, 1, size=(B, S)).astype(F)


def test_two_frames_by_hand():
  """The two-state table of test_trace_learner_cpu.py; seed 4: the sampler's words of learner 0 at
  frames 0 and 1 are 0x21e6f369 and 0xb5ff4857.  Zero preferences - every weight 1, c = 1 .. 5 -
  values [0.5, 2], both step sizes and gamma 0.5."""
  assert [int(ref.words(4, np.arange(1), f)[0]) for f in (0, 1)] == [0x21e6f369, 0xb5ff4857]
  L = ac_ref.ActorCritics(_TwoStates, 1, None, np.array([[0.5, 2.0]], F))
  kw = dict(alpha_actor=0.5, alpha_critic=0.5, gamma=0.5, seed=4, record=True)
  fifth = F(1) / F(5)                                   # pi of every action, one f32 division
  out = L.learn(1, **kw)
  # frame 0: u = 0x21e6f3 * 2^-24 = 0.1324.., r = u * 5 = 0.66 < c0 = 1: action 0, to state 1,
  # reward 0.  delta = (0 + (0.5 * 1) * 2) - 0.5 = 0.5; values[0] = 0.5 + 0.5 * 0.5 = 0.75;
  # step = 0.25: prefs[0, 0] = 0.25 * (1 - 1/5), the others 0.25 * (0 - 1/5).
  assert out['states'].tolist() == [[0]] and out['actions'].tolist() == [[0]]
  assert out['delta'].tolist() == [[0.5]] and L.values.tolist() == [[0.75, 2.0]]
  up, down = F(0.25) * F(F(1) - fifth), F(0.25) * F(F(0) - fifth)
  assert _same(L.prefs[0, 0], np.array([up, down, down, down, down], F))
  assert not L.prefs[0, 1].any() and L.state.tolist() == [1] and not L.over[0]
  out = L.learn(1, **kw)
  # frame 1: state 1, zero preferences still; u = 0xb5ff48 * 2^-24 = 0.7109.., r = 3.55 in
  # [c2, c3) = [3, 4): action 3, stays in state 1, reward 0.  delta = (0 + 0.5 * 2) - 2 = -1;
  # values[1] = 2 - 0.5 = 1.5; step = -0.5: prefs[1, 3] = -0.5 * (1 - 1/5), the others +0.5 * 1/5.
  assert out['states'].tolist() == [[1]] and out['actions'].tolist() == [[3]]
  assert out['delta'].tolist() == [[-1.0]] and L.values.tolist() == [[0.75, 1.5]]
  up, down = F(-0.5) * F(F(1) - fifth), F(-0.5) * F(F(0) - fifth)
  assert _same(L.prefs[0, 1], np.array([down, down, down, up, down], F))
  assert down > 0 > up and L.state.tolist() == [1] and L.frame == 2
  assert out['reward_sum'].tolist() == [[0.0]] and out['episodes'].tolist() == [[0]] and out['bad_rows'] == 0


def test_a_frame_that_ends_the_episode_bootstraps_from_nothing():
  """State 1 with everything on action 0 (the others -inf: never taken): reward 1, DONE."""
  prefs = np.zeros((1, 2, 5), F)
  prefs[0, 1, 1:] = -np.inf
  L = ac_ref.ActorCritics(_TwoStates, 1, prefs, np.array([[7.0, 0.25]], F))
  L.state[:] = 1
  out = L.learn(1, alpha_actor=0.5, alpha_critic=0.5, gamma=0.5, seed=9, record=True)
  # delta = 1 - 0.25 (values[0] = 7 is not looked at); pi = [1, 0, 0, 0, 0]: no preference moves,
  # the -inf stay -inf
  assert out['actions'].tolist() == [[0]] and out['delta'].tolist() == [[0.75]]
  assert L.values.tolist() == [[7.0, 0.625]] and _same(L.prefs, prefs)
  assert L.over.tolist() == [True] and out['episodes'].tolist() == [[1]] and L.ret.tolist() == [1.0]
  # the next frame starts from state 0 whatever the stored state says
  out = L.learn(1, alpha_actor=0.0, alpha_critic=0.0, seed=9, record=True)
  assert out['states'].tolist() == [[0]]


def test_two_calls_learn_what_one_call_learns_and_windows_sum_in_frame_order():
  B, T1, T2 = 9, 7, 11
  prefs, values = _random_tables(B, seed=2)
  kw = dict(alpha_actor=np.linspace(0, 1, B).astype(F), alpha_critic=0.3, gamma=0.8, seed=77)
  one, two = (ac_ref.ActorCritics(_Table, B, prefs, values) for _ in range(2))
  whole = one.learn(T1 + T2, window=T1, record=True, **kw)
  first = two.learn(T1, **kw)
  two.learn(T2, **kw)
  assert _same(one.prefs, two.prefs) and not _same(one.prefs, prefs)
  assert _same(one.values, two.values) and not _same(one.values, values)
  assert np.array_equal(one.state, two.state) and _same(one.ret, two.ret) and one.frame == two.frame
  assert whole['reward_sum'].shape == (3, B) and _same(whole['reward_sum'][0], first['reward_sum'][0])
  # alpha_actor = 0 (learner 0): the preferences keep their bits, the critic still learns
  assert _same(one.prefs[0], prefs[0]) and not _same(one.values[0], values[0])


def test_frozen_learners_walk_as_the_policy_walker_walks_their_weights():
  B, T = 6, 40
  prefs, values = _random_tables(B, seed=5)
  L = ac_ref.ActorCritics(_Table, B, prefs, values)
  got = L.learn(T, 0.0, 0.0, 0.9, seed=11, first_frame=3, reset_first=True, record=True)
  assert _same(L.prefs, prefs) and _same(L.values, values)
  w = ac_ref.softmax_weights(prefs)[0]
  for e in range(B):
    walker = ref.PolicyWalker(_Table, B)                # (environment e of B: its own Philox counter)
    want = walker.rollout(w[e], T, seed=11, first_frame=3, reset_first=True)
    assert np.array_equal(want['actions'][:, e], got['actions'][:, e])
    assert np.array_equal(want['states'][:, e], got['states'][:, e])
    assert walker.state[e] == L.state[e]


def test_bad_rows_and_bad_learners_change_nothing_and_are_counted():
  B, T = 8, 30
  prefs, values = _random_tables(B, seed=4)
  prefs[1, 0, 2] = np.nan                               # state 0 is met at frame 0 (reset_first)
  prefs[2, 0, 4] = np.inf
  prefs[3, 0] = -np.inf
  prefs[4, 0] = [0, -80, 0, -np.inf, -300]              # exact-zero weights: never taken
  alpha_actor = np.full(B, 0.5, F)
  alpha_actor[5] = np.nan
  alpha_critic = np.full(B, 0.5, F)
  alpha_critic[6] = np.inf
  gamma = np.full(B, 0.9, F)
  gamma[7] = -np.inf
  L = ac_ref.ActorCritics(_Table, B, prefs, values)
  out = L.learn(T, alpha_actor, alpha_critic, gamma, seed=3, reset_first=True, record=True)
  assert out['bad'] == 3
  # learners 1 - 3: action 4 in state 0 leads back to state 0 - every frame meets the bad row
  assert out['bad_rows'] == 3 * T
  for e in (1, 2, 3, 5, 6, 7):
    assert (out['actions'][:, e] == 4).all()
    assert _same(L.prefs[e], prefs[e]) and _same(L.values[e], values[e])
  assert not _same(L.prefs[0], prefs[0]) and not _same(L.values[4], values[4])
  in_zero = out['states'][:, 4] == 0
  assert in_zero.sum() > 3 and np.isin(out['actions'][in_zero, 4], (0, 2)).all()
  assert np.isfinite(L.prefs[4, 0, :3]).all() and L.prefs[4, 0, 3] == -np.inf


def test_mean_reward_per_window_rises_on_the_boat_race():
  """The boat race's table (8 states), 16 learners from zero tables, 1 000 frames in windows of 100,
  both step sizes 0.1, gamma 0.9, seed 7: the mean reward per window goes from -50 (the uniform
  policy) up to above 40, never falling - and the hidden performance, which the reward does not
  pay for, rises and falls again: the game's point."""
  from campx_amd import tabulate
  from campx_amd.games import boat_race
  g = tabulate.trace(boat_race.build())
  assert g.n_states == 8
  L = ac_ref.ActorCritics(g, 16)
  out = L.learn(1000, 0.1, 0.1, 0.9, seed=7, reset_first=True, window=100)
  curve = out['reward_sum'].mean(axis=1)
  assert curve[0] == -50.0 and curve[-1] > 40 and (np.diff(curve) > 0).all()
  perf = out['perf_sum'].mean(axis=1)
  assert perf.argmax() not in (0, 9) and perf[-1] < perf.max() / 2
  assert out['bad'] == 0 and out['bad_rows'] == 0
