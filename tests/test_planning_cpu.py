"""The planning rule's numpy restatement (tests/planning_reference.py) on a table worked by hand,
and `campx_wide_sweeps_plan()`, pure host code, at the sizes where the choice of path changes.
No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import planning_reference as plan_ref

F = np.float32
NAN = np.nan

# Three states, gamma 0.5, no discount codes.  (next, reward, done) per action:
#   state 0   a0 (1, 1)   a1 (2, 0)   a2 (0, -1)   a3 (1, None)   a4 (0, 0)
#   state 1   a0 (2, 1, DONE)   a1 (0, 0)   a2 (1, 1)   a3 (2, -1)   a4 (1, 0)
#   state 2   a0 .. a3 (2, 0)   a4 (0, 1)
NEXT = np.array([[1, 2, 0, 1, 0], [2, 0, 1, 2, 1], [2, 2, 2, 2, 0]], np.int32)
REWARD = np.array([[1, 0, -1, NAN, 0], [1, 0, 1, -1, 0], [0, 0, 0, 0, 1]], F)
DONE = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.uint8)
DISCOUNT = plan_ref.frame_discount(np.zeros((3, 5), np.int64), DONE, [1.0] * 16)
GAMMA = 0.5
FOUR_MOVES = np.array([[2, 2, 2, 2, 0]] * 3, F)             # uniform over the moves, total 8
ONE_HOT = np.array([[4, 0, 0, 0, 0], [0, 0, 4, 0, 0], [0, 0, 0, 0, 4]], F)


def _run(n, **kw):
  return plan_ref.sweeps(NEXT, REWARD, DONE, DISCOUNT, GAMMA, n, **kw)


def _same(a, b):
  a, b = np.asarray(a, F), np.asarray(b, F)
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_the_frame_discount_is_the_listed_one_or_the_default():
  listed = [1.0, 0.25, 0.0] + [0.5] * 13
  got = plan_ref.frame_discount([0, 0, 1, 2, 2], [0, 1, 0, 0, 1], listed)
  assert _same(got, [1.0, 0.0, 0.25, 0.0, 0.0])
  assert _same(DISCOUNT, 1.0 - DONE.astype(F))


def test_uniform_policy_by_hand():
  # sweep 1: q = r.  state 0: (2*1 + 2*0 - 2*1 + 2*0) / 8 = 0; state 1: (2 + 0 + 2 - 2) / 8
  # sweep 2, state 0: q = [1 + .5 * .25, 0, -1, .5 * .25, 0] -> (2.25 + 0 - 2 + .25) / 8
  #          state 1: q = [1 (done), 0, 1.125, -1, .125] -> (2 + 0 + 2.25 - 2) / 8
  # sweep 3, state 0: q = [1.140625, 0, -.96875, .140625, .03125] -> .625 / 8
  #          state 1: q = [1, .03125, 1.140625, -1, .140625] -> 2.34375 / 8
  want = [[0, 0.25, 0], [0.0625, 0.28125, 0], [0.078125, 0.29296875, 0]]
  for n in (1, 2, 3):
    out = _run(n, policy=FOUR_MOVES)
    assert _same(out['values'], want[n - 1]), n
    assert out['bad_rows'] == 0 and 'greedy' not in out
  assert _same(out['q'][0], [1.140625, 0, -0.96875, 0.140625, 0.03125])
  assert _same(out['q'][1], [1, 0.03125, 1.140625, -1, 0.140625])
  assert _same(out['q'][2], [0, 0, 0, 0, 1.03125])
  assert _same(out['residual'], [0.25, 0.0625, 0.015625])
  assert all(_same(out['history'][k + 1], want[k]) for k in range(3))


def test_one_hot_policy_by_hand():
  # state 0 takes a0 (to 1, reward 1), state 1 a2 (stays, 1), state 2 a4 (to 0, 1): 1, 1.5, 1.75
  for n, v in ((1, 1.0), (2, 1.5), (3, 1.75)):
    out = _run(n, policy=ONE_HOT)
    assert _same(out['values'], [v] * 3), n
  assert _same(out['residual'], [1, 0.5, 0.25])


def test_greedy_by_hand_and_the_tie_goes_to_the_lowest_action():
  out = _run(1)
  # state 1: q0 = 1 (done) and q2 = 1 tie -> action 0
  assert _same(out['q'][1], [1, 0, 1, -1, 0]) and out['greedy'].tolist() == [0, 0, 4]
  assert out['greedy'].dtype == np.int8 and _same(out['values'], [1, 1, 1])
  out = _run(2)
  assert _same(out['q'][1], [1, 0.5, 1.5, -0.5, 0.5]) and out['greedy'].tolist() == [0, 2, 4]
  assert _same(out['values'], [1.5] * 3)
  out = _run(3)
  assert _same(out['values'], [1.75] * 3) and _same(out['q'][0], [1.75, 0.75, -0.25, 0.75, 0.75])
  assert _same(out['residual'], [1, 0.5, 0.25])


def test_values_is_the_reduction_of_the_returned_q_and_sweeps_continue():
  whole = _run(5, policy=FOUR_MOVES)
  first = _run(2, policy=FOUR_MOVES)
  rest = _run(3, policy=FOUR_MOVES, values=first['values'])
  assert _same(rest['values'], whole['values']) and _same(rest['q'], whole['q'])
  assert _same(np.concatenate([first['residual'], rest['residual']]), whole['residual'])
  assert _same(plan_ref.reduce_policy(whole['q'], FOUR_MOVES)[0], whole['values'])
  g = _run(4)
  assert _same(plan_ref.reduce_greedy(g['q'])[0], g['values'])


@pytest.mark.parametrize('row', [[1, -1, 1, 1, 1], [1, NAN, 1, 1, 1], [0, 0, 0, 0, 0],
                                 [3e38, 3e38, 0, 0, 0], [1, 1, 1, 1, -0.5]])
def test_a_bad_row_takes_action_4_and_is_counted(row):
  policy = FOUR_MOVES.copy()
  policy[1] = row
  out = _run(3, policy=policy)
  assert out['bad_rows'] == 1
  assert _same(out['values'][1], out['q'][1, 4])
  good = _run(3, policy=FOUR_MOVES)
  assert not _same(out['values'], good['values'])
  # -0.0 is not negative: the sampler's test is w >= 0
  policy[1] = [2, 2, 2, 2, -0.0]
  assert _run(3, policy=policy)['bad_rows'] == 0


def test_a_nan_reward_counts_as_zero_also_in_an_override():
  zero = np.where(np.isnan(REWARD), F(0), REWARD)
  a, b = _run(3, policy=FOUR_MOVES), plan_ref.sweeps(NEXT, zero, DONE, DISCOUNT, GAMMA, 3, policy=FOUR_MOVES)
  assert _same(a['values'], b['values']) and _same(a['q'], b['q'])
  over = np.full((3, 5), NAN, F)
  out = _run(3, reward_override=over)
  assert _same(out['values'], [0, 0, 0]) and _same(out['q'], np.zeros((3, 5)))
  over[2, 4] = 2
  assert _same(_run(1, reward_override=over)['values'], [0, 0, 2])


def test_the_residual_is_the_largest_bit_pattern():
  assert _same(plan_ref.residual_of([1, -3, 2], [1, 1, 2.5]), 4.0)
  assert _same(plan_ref.residual_of([0.0], [-0.0]), 0.0)
  assert np.isnan(plan_ref.residual_of([1, NAN, 9], [0, 0, 0]))
  assert np.isnan(plan_ref.residual_of([np.inf, 1], [np.inf, 0]))          # inf - inf
  assert plan_ref.residual_of([np.inf, 1], [0, 0]) == np.inf
  assert plan_ref.residual_of([1, 2], [1, 2]).dtype == F


def test_done_cuts_the_carry_and_discounts_scale_it():
  v = np.array([8, 16, 32], F)
  q = plan_ref.backup(NEXT, REWARD, DONE, DISCOUNT, 0.5, v)
  assert q[1, 0] == 1 and q[0, 0] == 1 + 0.5 * 16 and q[0, 3] == 0.5 * 16
  disc = DISCOUNT.copy()
  disc[0, 0] = 0.25
  assert plan_ref.backup(NEXT, REWARD, DONE, disc, 0.5, v)[0, 0] == 1 + 0.125 * 16


# ---------------------------------------------------------------- the plan's arithmetic

LDS_MAX = 144 * 1024
HEADER = 128


def _plan(S, policy, override, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_sweeps_plan(S, policy, override, lds_max, path, out)
  return code, list(out)


def _lds_bytes(S, policy):
  """The header's account of path 1: a header, the entries, two value vectors and - for a policy -
  the weights and their totals, each part rounded up to 16 bytes."""
  up = lambda x: (x + 15) // 16 * 16
  return HEADER + up(40 * S) + 2 * up(4 * S) + ((up(20 * S) + up(4 * S)) if policy else 0)


def _largest(policy):
  S = 1
  while _lds_bytes(S + 1, policy) <= LDS_MAX:
    S += 1
  return S


def test_exports_and_op_name():
  from campx_amd import _hip
  assert 'campx_wide_sweeps_plan' in _hip.EXPORTS and 'campx_wide_sweeps_launch' in _hip.EXPORTS
  assert 'wide_sweeps' in _hip.OP_NAMES
  assert _hip.config_get('wide_lds_max') == LDS_MAX


@pytest.mark.parametrize('policy', [0, 1])
@pytest.mark.parametrize('override', [0, 1])
def test_the_largest_table_that_fits_and_the_next(policy, override):
  S = _largest(policy)
  assert S == (2045 if policy else 3068)        # 72 and 48 bytes per state, less the roundings
  code, p = _plan(S, policy, override)
  assert code == 0 and p == [1, _lds_bytes(S, policy), 1024, 1]
  code, p = _plan(S + 1, policy, override)
  assert code == 0 and p == [2, 0, 256, (S + 1 + 255) // 256]
  # forced either way
  assert _plan(S, policy, override, path=2)[1] == [2, 0, 256, (S + 255) // 256]
  assert _plan(S, policy, override, path=1)[1][0] == 1
  assert _plan(S + 1, policy, override, path=1)[0] != 0


def test_threads_cover_small_tables_in_whole_waves():
  for S, threads in ((1, 64), (8, 64), (64, 64), (65, 128), (1000, 1024), (1024, 1024), (1025, 1024)):
    code, p = _plan(S, 1, 0)
    assert code == 0 and p[0] == 1 and p[2] == threads and p[1] == _lds_bytes(S, 1), S
    assert p[1] % 16 == 0


def test_wide_lds_max_zero_forces_global_and_path_1_is_refused_then():
  for policy in (0, 1):
    assert _plan(8, policy, 0, lds_max=0) == (0, [2, 0, 256, 1])
    assert _plan(8, policy, 0, lds_max=0, path=1)[0] != 0
    assert _plan(8, policy, 0, lds_max=_lds_bytes(8, policy))[1][0] == 1
    assert _plan(8, policy, 0, lds_max=_lds_bytes(8, policy) - 1)[1][0] == 2


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  for args in ((0, 0, 0), (-1, 0, 0), ((1 << 24) + 1, 0, 0), (8, 2, 0), (8, 0, 2), (8, -1, 0)):
    assert _plan(*args)[0] != 0, args
  assert _plan(8, 0, 0, lds_max=-1)[0] != 0
  assert _plan(8, 0, 0, path=3)[0] != 0 and _plan(8, 0, 0, path=-1)[0] != 0
  assert _hip.lib.campx_wide_sweeps_plan(8, 0, 0, LDS_MAX, 0, None) != 0
  assert _plan(1 << 24, 1, 1) == (0, [2, 0, 256, (1 << 24) // 256])


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_sweeps_launch
  fake = vp(0x1000)
  # no spec, no tables, no values, no residual
  assert f(None, fake, None, None, 0.5, fake, fake, fake, None, None, fake, None, None, 1, 0, None) != 0
