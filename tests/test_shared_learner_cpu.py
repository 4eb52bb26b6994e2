"""`campx_wide_shared_plan()` - pure host arithmetic - against the header's account of the bytes,
the refusals of `campx_wide_shared_launch()` that are decided before a device is touched, the op's
schema, and the numpy shared learners of tests/shared_learner_reference.py against a table worked
by hand, their quantiser's edges and the per-environment learners of tests/learner_reference.py.
No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import learner_reference as learn_ref
import shared_learner_reference as shared_ref
from test_population_cpu import _Table, _same, _valid_spec
from wide_table_reference import integer_table

F = np.float32
LDS_MAX = 144 * 1024
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h


def _plan(S, perf, B, P, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 6)()
  code = _hip.lib.campx_wide_shared_plan(S, perf, B, P, lds_max, path, out)
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
  held = min(most, (lds_max - table) // (S * 80)) if lds_max >= table else 0
  if path == 1 and held < 1:
    return None
  pays = held >= 1 and (held == most or held * n >= 64)
  if path == 1 or (path == 0 and pays):
    return [1, held, held * n, table + held * S * 80, 1, 1]
  in_lds = 1 if table <= lds_max else 0
  return [2, most, most * n, table if in_lds else 0, in_lds, 1]


def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  for name in ('campx_wide_shared_plan', 'campx_wide_shared_scratch_bytes', 'campx_wide_shared_launch'):
    assert name in _hip.EXPORTS and hasattr(_hip.lib, name)
  assert 'wide_learn_shared' in _hip.OP_NAMES
  s = str(torch.ops.campx.wide_learn_shared.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor(d!) q', 'Tensor alpha',
               'Tensor gamma', 'Tensor epsilon', 'int rule', 'int seed', 'int first_frame',
               'int frames', 'int window', 'Tensor(e!) reward_sum', 'Tensor(f!)? perf_sum',
               'Tensor(g!) episodes', 'Tensor(h!) clamped', 'Tensor(i!)? scratch',
               'Tensor(j!)? bad_count', 'Tensor(k!)? bad_flag', 'bool reset_first', 'int path=0'):
    assert part in s, s
  assert s.endswith('-> ()')
  assert _hip.lib.campx_wide_shared_scratch_bytes(8, 256) == 256 * 8 * 5 * 12
  assert _hip.lib.campx_wide_shared_scratch_bytes(0, 256) == 0


def test_the_surface_names_both_methods():
  from campx_amd import engine, fused, wide
  for name in ('learn_shared', 'shared_learner_buffers'):
    assert name in wide.STATE_TABLE_ONLY and callable(getattr(wide.WideGame, name))
    assert getattr(engine.Engine, name).__doc__
    assert getattr(fused.FusedGame, name).state_table_only
  doc = wide.WideGame.learn_shared.__doc__
  assert 'grid-wide barrier' in doc and 'out of scope' in doc and '1024' in doc
  assert 'learn_shared()' in wide.WideGame.learn_tabular.__doc__


@pytest.mark.parametrize('perf', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 256, 257, 1024])
@pytest.mark.parametrize('S', [1, 8, 159])
def test_plan_against_the_byte_account(S, n, perf):
  table = _table_bytes(S, perf)
  for P in (1, 2, 85, 86, 257):
    B = P * n
    for path in (0, 1, 2):
      for lds_max in (LDS_MAX, 0, table - 1, table, table + S * 80 - 1, table + S * 80,
                      table + 2 * S * 80):
        if lds_max < 0:
          continue
        want = _account(S, perf, B, P, lds_max, path)
        code, got = _plan(S, perf, B, P, lds_max, path)
        assert (code, got) == ((EINVAL, [0] * 6) if want is None else (OK, want)), (P, path, lds_max)
        if want is not None:
          # what every launch relies on: whole learners, at most the largest workgroup, never
          # more LDS than allowed
          assert 1 <= got[1] <= P and got[2] == got[1] * n <= 1024 and got[3] <= max(lds_max, 0)


def test_the_sizes_the_header_names():
  # the boat race, hidden performance: 368 bytes of table, 640 per learner
  assert _plan(8, 1, 65536, 256) == (0, [1, 1, 256, 368 + 640, 1, 1])           # n = 256
  assert _plan(8, 1, 65536, 4096) == (0, [1, 16, 256, 368 + 16 * 640, 1, 1])    # n = 16
  assert _plan(8, 1, 65536, 64) == (0, [1, 1, 1024, 368 + 640, 1, 1])           # n = 1024
  # n = 1: what fits, 229 of the 256 learners a workgroup would hold
  assert (LDS_MAX - 368) // 640 == 229
  assert _plan(8, 1, 65536, 65536) == (0, [1, 229, 229, 368 + 229 * 640, 1, 1])
  # the maze at n = 1: 11 learners fit, less than a wave - global; forced, they are taken
  assert _plan(159, 0, 4096, 4096) == (0, [2, 256, 256, 6368, 1, 1])
  assert _plan(159, 0, 4096, 4096, path=1) == (0, [1, 11, 11, 6368 + 11 * 12720, 1, 1])
  # ... at n = 16, 11 learners are 176 threads: LDS
  assert _plan(159, 0, 4096, 256) == (0, [1, 11, 176, 6368 + 11 * 12720, 1, 1])
  assert _plan(159, 0, 2048, 2) == (0, [1, 1, 1024, 6368 + 12720, 1, 1])


@pytest.mark.parametrize('perf', [0, 1])
def test_the_largest_table_that_takes_path_1_and_the_next(perf):
  """One learner of n = 256 actors: path 1 as long as the table and one learner's 80 bytes per
  state fit."""
  S = 1
  while _table_bytes(S + 1, perf) + (S + 1) * 80 <= LDS_MAX:
    S += 1
  assert S == (1228 if not perf else 1179)
  need = _table_bytes(S, perf) + S * 80
  assert _plan(S, perf, 512, 2) == (0, [1, 1, 256, need, 1, 1])
  assert _plan(S + 1, perf, 512, 2) == (0, [2, 1, 256, _table_bytes(S + 1, perf), 1, 1])
  assert _plan(S + 1, perf, 512, 2, path=1)[0] == EINVAL and _plan(S, perf, 512, 2, path=1)[0] == OK
  assert _plan(S, perf, 512, 2, path=2) == (0, [2, 1, 256, _table_bytes(S, perf), 1, 1])


def test_wide_lds_max_zero_forces_global_and_path_1_is_refused_then():
  for B, P in ((512, 2), (64, 64), (2048, 2)):
    n = B // P
    G = min(P, max(1, 256 // n))
    assert _plan(8, 1, B, P, lds_max=0) == (0, [2, G, G * n, 0, 0, 1])
    assert _plan(8, 1, B, P, lds_max=0, path=2) == (0, [2, G, G * n, 0, 0, 1])
    assert _plan(8, 1, B, P, lds_max=0, path=1)[0] == EINVAL


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  assert _plan(8, 0, 512, 2)[0] == 0
  for S, perf, B, P in ((0, 0, 512, 2), (-1, 0, 512, 2), ((1 << 24) + 1, 0, 1, 1), (8, 2, 512, 2),
                        (8, -1, 512, 2), (8, 0, 0, 1), (8, 0, -4, 2), (8, 0, 1 << 32, 1 << 22),
                        (8, 0, 512, 0), (8, 0, 512, -1), (8, 0, 512, 1024),
                        (8, 0, 512, 3), (8, 0, 513, 2),          # P does not divide B
                        (8, 0, 1025, 1), (8, 0, 2050, 2),        # n = 1 025
                        (8, 0, (1 << 31) // 40 + 1, (1 << 31) // 40 + 1),   # P * S * 5 >= 2^31, by one
                        (1 << 24, 0, 26, 26)):
    assert _plan(S, perf, B, P)[0] == EINVAL, (S, perf, B, P)
  assert _plan(8, 0, 1024, 1)[0] == 0 and _plan(8, 0, 2048, 2)[0] == 0          # n = 1 024
  assert _plan(8, 0, (1 << 31) // 40, (1 << 31) // 40)[0] == 0
  assert _plan(1 << 24, 0, 25, 25, path=2)[0] == 0
  assert _plan(8, 0, 512, 2, lds_max=-1)[0] == EINVAL
  assert _plan(8, 0, 512, 2, path=3)[0] == EINVAL and _plan(8, 0, 512, 2, path=-1)[0] == EINVAL
  assert _hip.lib.campx_wide_shared_plan(8, 0, 512, 2, LDS_MAX, 0, None) == EINVAL


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_shared_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)

  def learner(**kw):
    fields = dict(q=fake, alpha=fake, gamma=fake, epsilon=fake, reward_sum=fake, perf_sum=None,
                  episodes=fake, clamped=fake, scratch=None, scratch_bytes=0, bad_count=None,
                  bad_flag=None, seed=1, first_frame=0, n_learners=2, window=0, rule=0, path=0,
                  reset_first=0)
    fields.update(kw)
    return _hip.CampxSharedLearner(**fields)

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
  for name in ('q', 'alpha', 'gamma', 'epsilon', 'reward_sum', 'episodes', 'clamped'):
    assert call(window=2, **{name: None}) == EINVAL, name
  assert call(B=0, window=2) == EINVAL and call(T=0, window=2) == EINVAL
  assert call(B=1 << 32, window=2) == EINVAL
  assert call(first_frame=-1, window=2) == EINVAL
  assert call(first_frame=(1 << 63) - 4, window=2) == EINVAL            # first_frame + T past 2^63 - 1
  assert call(q=fake + 4, window=2) == EINVAL and call(q=fake + 8, window=2) == EINVAL
  for name in ('alpha', 'gamma', 'epsilon', 'reward_sum', 'perf_sum', 'episodes', 'bad_count', 'bad_flag'):
    assert call(window=2, **{name: fake + 2}) == EINVAL, name
  assert call(window=2, clamped=fake + 4) == EINVAL and call(window=2, scratch=fake + 4) == EINVAL
  assert call(st=_hip.CampxState(pos=fake + 2, done=fake), window=2) == EINVAL
  assert call(st=_hip.CampxState(pos=fake, done=fake, ret=fake + 1), window=2) == EINVAL
  assert call(rule=2, window=2) == EINVAL and call(rule=-1, window=2) == EINVAL
  assert call(path=3, window=2) == EINVAL and call(path=-1, window=2) == EINVAL
  assert call(n_learners=0, window=2) == EINVAL and call(scratch_bytes=-1, window=2) == EINVAL
  # A spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict.
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), window=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert (1 << 20) * 5 * 410 >= 1 << 31 > (1 << 20) * 5 * 409
  assert call(spec=by, B=410, n_learners=410, window=2, path=2) == EINVAL         # the element bound
  assert call(spec=by, B=409, n_learners=2, window=2, path=2) == EINVAL           # P does not divide B
  assert call(spec=by, B=1025, n_learners=1, window=2, path=2) == EINVAL          # n = 1 025
  # the control: only the plan knows that 2^20 states do not fit the LDS of a workgroup
  assert _plan(1 << 20, 0, 409, 409, path=1)[0] == EINVAL and _plan(1 << 20, 0, 409, 409, path=2)[0] == 0
  assert call(spec=by, B=409, n_learners=409, window=2, path=1) == EINVAL
  # the global path without its scratch, or with too little of it
  need = 409 * (1 << 20) * 5 * 12
  assert call(spec=by, B=409, n_learners=409, window=2, path=2) == EINVAL
  assert call(spec=by, B=409, n_learners=409, window=2, path=2, scratch=fake, scratch_bytes=need - 1) == EINVAL
  # perf_sum for a game without hidden performance
  assert call(spec=by, B=409, n_learners=409, window=2, path=2, scratch=fake, scratch_bytes=need,
              perf_sum=fake) == EINVAL


# ---------------------------------------------------------------- the rule, by hand

def _q(rows, P=1):
  return np.tile(np.array([rows], F), (P, 1, 1))


def test_two_environments_in_one_bin_move_q_by_alpha_times_the_mean_of_their_deltas():
  """epsilon = 0, both environments of the one learner in state 0, all-zero rows: action 0 for
  both, -> state 1 with reward 1.  Both deltas are 1: q[0, 0] = 0.5 * 1.  Next frame both are in
  state 1, a0: done, target 1, q[1, 0] = 0.5."""
  L = shared_ref.SharedLearners(_Table, 2, _q([[0] * 5] * 3))
  out = L.learn(2, alpha=0.5, gamma=0.5, epsilon=0.0, record=True, reset_first=True)
  assert out['actions'].tolist() == [[0, 0], [0, 0]] and out['delta'].tolist() == [[1, 1], [1, 1]]
  assert L.q.tolist() == [[[0.5, 0, 0, 0, 0], [0.5, 0, 0, 0, 0], [0] * 5]]
  assert out['episodes'].tolist() == [[1, 1]] and out['reward_sum'].tolist() == [[2.0, 2.0]]
  assert out['clamped'].tolist() == [0] and out['bad'] == 0
  # two bins in one frame: each moves by its own visitor's delta
  L = shared_ref.SharedLearners(_Table, 2, _q([[0, 0, 0, 0, 0], [2, 0, 0, 0, 0], [0] * 5]))
  L.state[:] = [0, 1]
  # env 0: state 0 a0 -> 1, r 1, target 1 + 0.5 * 2 = 2, delta 2, bin (0, 0)
  # env 1: state 1 a0 -> done, r 1, target 1, delta 1 - 2 = -1, bin (1, 0)
  out = L.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0, record=True)
  assert out['delta'].tolist() == [[2, -1]] and L.q[0, :2, 0].tolist() == [1.0, 1.5]


def test_the_mean_of_two_different_deltas():
  """Two environments in bin (0, 2) - state 0, a2 -> state 0, reward -1 - cannot differ in delta
  (same table, same bin); two that share the bin after exploring do not either.  So the mean is
  checked where it can differ from each delta: through the quantiser, Z / c."""
  z, clamp = shared_ref.quantise(np.array([0.75, -0.25], F))
  assert z.tolist() == [3 << 30, -(1 << 30)] and not clamp.any()
  assert shared_ref.mean_of(z.sum(), 2) == F(0.25)
  # three visitors: the mean is rounded once, from the exact integer sum
  z, _ = shared_ref.quantise(np.array([1, 1, 2], F))
  assert shared_ref.mean_of(z.sum(), 3) == F(np.float64(4 << 32) / 3 * 2.0 ** -32)


def test_two_environments_in_different_bins_move_q_as_learn_tabular_would():
  """... up to quantisation: none here, the deltas are multiples of 2^-32."""
  q0 = _q([[0, 0, 1, 0, 0], [0.5, 0, 0, 0, 0], [0] * 5])
  L = shared_ref.SharedLearners(_Table, 2, q0)
  L.state[:] = [0, 1]
  L.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0)
  for e, s in ((0, 0), (1, 1)):
    alone = learn_ref.Learners(_Table, 1, q0)
    alone.state[:] = s
    alone.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0)
    assert _same(L.q[0, s], alone.q[0, s])


def test_a_frame_that_ends_the_episode_has_target_r_and_none_counts_as_zero():
  L = shared_ref.SharedLearners(_Table, 1, _q([[0] * 5, [0.25, 0, 0, 0, 0], [9] * 5]))
  L.state[:] = 1
  out = L.learn(1, alpha=1.0, gamma=0.5, epsilon=0.0, record=True)
  # state 1 a0 -> state 2, reward 1, DONE: target 1, not 1 + 0.5 * 9
  assert out['actions'].tolist() == [[0]] and L.q[0, 1, 0] == F(1.0) and L.over.tolist() == [True]
  # state 0 a3 -> state 1, reward None
  L = shared_ref.SharedLearners(_Table, 1, _q([[0, 0, 0, 1, 0], [0, 0, 4, 0, 0], [0] * 5]))
  out = L.learn(1, alpha=0.25, gamma=0.5, epsilon=0.0, record=True)
  assert out['actions'].tolist() == [[3]] and L.q[0, 0, 3] == F(1.25) and not np.isnan(L.q).any()
  assert out['reward_sum'].tolist() == [[0.0]] and L.ret.tolist() == [0.0]


def test_the_bootstrap_row_is_the_table_before_the_frames_update_for_every_environment():
  """Environment 0 in state 1 takes a1 -> state 0 and bootstraps from q[0]; environment 1 in
  state 0 takes a2 -> state 0 and updates q[0, 2] in the same frame.  Environment 0 sees the 1
  that stood there, not the updated value."""
  q0 = _q([[0, 0, 1, 0, 0], [0, 3, 0, 0, 0], [0] * 5])
  L = shared_ref.SharedLearners(_Table, 2, q0)
  L.state[:] = [1, 0]
  out = L.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0, record=True)
  assert out['actions'].tolist() == [[1, 2]]
  # env 0: target 0 + 0.5 * 1 = 0.5, delta -2.5 -> q[1, 1] = 1.75
  # env 1: target -1 + 0.5 * 1 = -0.5, delta -1.5 -> q[0, 2] = 0.25
  assert L.q[0, 1, 1] == F(1.75) and L.q[0, 0, 2] == F(0.25)


def test_the_quantisers_edges():
  half = F(2.0 ** -33)
  z, clamp = shared_ref.quantise(np.array([half, -half, 3 * half, -3 * half, 5 * half], F))
  assert z.tolist() == [0, 0, 2, -2, 2] and not clamp.any()           # half to even
  big = np.nextafter(F(2.0 ** 20), F(np.inf))
  z, clamp = shared_ref.quantise(np.array([2.0 ** 20, big, -big, np.inf, -np.inf, np.nan], F))
  assert z.tolist() == [1 << 52, 1 << 52, -(1 << 52), 1 << 52, -(1 << 52), 0]
  assert clamp.tolist() == [False, True, True, True, True, True]
  # 1 024 clamped values do not overflow
  z, clamp = shared_ref.quantise(np.full(1024, np.inf, F))
  total = np.zeros(1, np.int64)
  np.add.at(total, np.zeros(1024, np.int64), z)
  assert int(total[0]) == 1024 << 52 < 1 << 63 and clamp.all()
  assert shared_ref.mean_of(total[0], 1024) == F(2.0 ** 20)


def test_clamped_errors_are_counted_per_learner_and_written_into_q():
  """Learner 0 has an infinity where it bootstraps from, learner 1 a NaN in the entry it updates,
  learner 2 an ordinary table."""
  q0 = _q([[0] * 5, [0] * 5, [0] * 5], P=3)
  q0[0, 1, 2] = np.inf                   # state 0 a0 -> state 1: target inf, delta inf
  q0[1, 0, 0] = np.nan                   # greedy skips nothing: NaN q0 is never displaced; delta NaN
  L = shared_ref.SharedLearners(_Table, 6, q0)
  out = L.learn(1, alpha=0.5, gamma=0.5, epsilon=0.0, record=True, reset_first=True)
  assert out['actions'].tolist() == [[0] * 6] and out['clamped'].tolist() == [2, 2, 0]
  assert L.q[0, 0, 0] == F(0.5 * 2.0 ** 20)          # the clamped mean
  assert np.isnan(L.q[1, 0, 0])                      # NaN + 0.5 * 0 stays NaN
  assert L.q[2, 0, 0] == F(0.5)


# ---------------------------------------------------------------- relations

def _random_q(P, seed=0):
  return np.random.RandomState(seed).uniform(-1, 1, size=(P, 3, 5)).astype(F)


@pytest.mark.parametrize('rule', shared_ref.RULES)
def test_alpha_zero_leaves_q_bit_identical(rule):
  q = _random_q(4)
  L = shared_ref.SharedLearners(_Table, 16, q)
  L.learn(40, alpha=0.0, gamma=0.9, epsilon=0.3, rule=rule, seed=3)
  assert _same(L.q, q)


@pytest.mark.parametrize('rule', shared_ref.RULES)
@pytest.mark.parametrize('T1', [7, 8])
def test_two_calls_learn_what_one_call_learns(T1, rule):
  B, P, T2 = 12, 3, 11
  q = _random_q(P, seed=T1)
  kw = dict(alpha=0.3, gamma=0.8, epsilon=0.25, rule=rule, seed=0xfeedfacecafebeef)
  one, two = shared_ref.SharedLearners(_Table, B, q), shared_ref.SharedLearners(_Table, B, q)
  whole = one.learn(T1 + T2, window=T1, **kw)
  first = two.learn(T1, **kw)
  second = two.learn(T2, window=T1, **kw)
  assert _same(one.q, two.q) and not _same(one.q, q)
  assert np.array_equal(one.state, two.state) and np.array_equal(one.over, two.over)
  assert _same(one.ret, two.ret) and one.frame == two.frame == T1 + T2
  assert _same(whole['reward_sum'][0], first['reward_sum'][0])
  assert _same(whole['reward_sum'][1], second['reward_sum'][0])
  assert np.array_equal(whole['clamped'], first['clamped'] + second['clamped'])


def test_a_bad_learner_takes_action_4_keeps_its_table_and_is_counted_once():
  B, P = 12, 4
  q = _random_q(P)
  alpha = np.array([0.5, np.nan, 0.5, 0.5], F)
  eps = np.array([0.2, 0.2, 1.5, 0.2], F)
  L = shared_ref.SharedLearners(_Table, B, q)
  out = L.learn(10, alpha=alpha, gamma=0.9, epsilon=eps, seed=2, record=True)
  assert out['bad'] == 2 and (out['actions'][:, 3:9] == 4).all()           # not 6: per learner
  assert _same(L.q[1:3], q[1:3]) and not _same(L.q[0], q[0]) and not _same(L.q[3], q[3])
  assert out['clamped'].tolist() == [0] * 4
  # the good learners learn what they learn without it (the counter is the absolute environment)
  alone = shared_ref.SharedLearners(_Table, B, q)
  alone.learn(10, alpha=0.5, gamma=0.9, epsilon=0.2, seed=2)
  assert _same(L.q[[0, 3]], alone.q[[0, 3]])


def test_one_actor_per_learner_is_learn_tabular_when_nothing_is_rounded_away():
  """n = 1, alpha = gamma = 0.5, q0 = 0, integer rewards, discounts of 1, eight frames: every
  delta is a multiple of 2^-32 below 2^20, so the quantiser is exact, the mean of one value is the
  value, and q is `learner_reference`'s bit for bit."""
  g = integer_table()
  B = 16
  kw = dict(alpha=0.5, gamma=0.5, epsilon=0.5, seed=11, reset_first=True)
  shared = shared_ref.SharedLearners(g, B, np.zeros((B, g.n_states, 5), F))
  got = shared.learn(8, record=True, **kw)
  # the premise
  delta = got['delta'].astype(np.float64)
  assert np.array_equal(delta * 2.0 ** 32, np.rint(delta * 2.0 ** 32)) and np.abs(delta).max() < 2.0 ** 20
  assert np.abs(delta).max() > 0 and got['clamped'].tolist() == [0] * B
  alone = learn_ref.Learners(g, B)
  want = alone.learn(8, record=True, **kw)
  assert _same(shared.q, alone.q) and np.abs(alone.q).max() > 0
  assert np.array_equal(got['actions'], want['actions']) and _same(got['delta'], want['delta'])
  assert _same(got['reward_sum'], want['reward_sum']) and _same(shared.ret, alone.ret)
  assert np.array_equal(shared.state, alone.state)
