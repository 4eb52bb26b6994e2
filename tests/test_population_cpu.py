"""`campx_wide_population_plan()` - pure host arithmetic - against a brute-force count of the
members every workgroup touches, the launch's refusals that are decided before a device is
touched, and the population walk of tests/population_reference.py against
`policy_reference.PolicyWalker` and a table worked by hand.  No kernel is launched here."""

import ctypes

import numpy as np
import pytest

import policy_reference as ref
import population_reference as pop_ref

F = np.float32
LDS_MAX = 144 * 1024
THREADS = 256
OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h
BATCHES = (1, 64, 255, 256, 260, 512, 771, 65536)


def _plan(S, perf, B, P, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_population_plan(S, perf, B, P, lds_max, path, out)
  return code, list(out)


def _brute_members_per_block(B, P):
  """The definition: over every workgroup of 256 consecutive environments, the number of
  distinct members e // n among them."""
  member = np.arange(B, dtype=np.int64) // (B // P)
  starts = np.arange(0, B, THREADS)
  ends = np.minimum(starts + THREADS, B) - 1
  return int((member[ends] - member[starts] + 1).max())      # (members are contiguous)


def _lds_bytes(S, perf, members):
  """The header's account of path 1: the entries, the states' cells and - hidden performance -
  its bytes, each part rounded up to 16, plus five float thresholds per state and staged member."""
  up = lambda x: (x + 15) // 16 * 16
  return up(40 * S) + 16 * S + (up(5 * S) if perf else 0) + members * S * 20


def _divisors(B):
  return sorted({P for P in range(1, min(B, 1024) + 1) if B % P == 0} | {B})


def test_exports_op_name_and_schema():
  import torch
  from campx_amd import _hip
  assert 'campx_wide_policy_population_launch' in _hip.EXPORTS
  assert 'campx_wide_population_plan' in _hip.EXPORTS
  assert 'wide_policy_population' in _hip.OP_NAMES
  assert _hip.config_get('wide_lds_max') == LDS_MAX
  s = str(torch.ops.campx.wide_policy_population.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(c!)? ret', 'Tensor policy', 'int seed',
               'int first_frame', 'Tensor(d!)? reward', 'Tensor(e!)? discount', 'Tensor(f!)? step_done',
               'Tensor(g!)? perf', 'Tensor(h!) trace', 'Tensor(i!) actions_out',
               'Tensor(j!)? states_out', 'Tensor(k!)? bad_count', 'Tensor(l!)? bad_flag',
               'bool reset_first', 'int path=0'):
    assert part in s, s
  # wide_policy_update's schema and one more argument
  sibling = str(torch.ops.campx.wide_policy_update.default._schema)
  assert s.replace('wide_policy_population', 'wide_policy_update').replace(', int path=0', '') == sibling


@pytest.mark.parametrize('B', BATCHES)
def test_members_per_block_against_a_brute_force_count(B):
  for P in _divisors(B):
    want = _brute_members_per_block(B, P)
    for S, perf in ((8, 1), (159, 0)):
      code, p = _plan(S, perf, B, P)
      assert code == 0, (B, P, S)
      assert p[3] == want and p[2] == THREADS, (B, P, p, want)
      need = _lds_bytes(S, perf, want)
      assert p[:2] == ([1, need] if need <= LDS_MAX else [2, 0]), (B, P, S, p, need)
      # both sides of the bound, and the forced paths
      assert _plan(S, perf, B, P, lds_max=need)[1][:2] == [1, need]
      assert _plan(S, perf, B, P, lds_max=need - 1) == (0, [2, 0, THREADS, want])
      assert _plan(S, perf, B, P, lds_max=need, path=2) == (0, [2, 0, THREADS, want])
      assert _plan(S, perf, B, P, lds_max=need, path=1) == (0, [1, need, THREADS, want])
      assert _plan(S, perf, B, P, lds_max=need - 1, path=1)[0] == EINVAL


def test_the_extremes_the_header_names():
  # aligned blocks, n a multiple of 256: one member; n = 1: 256 members - 41 KB of thresholds for
  # the boat race's 8 states, the global path for the maze's 159
  assert _plan(8, 1, 65536, 256)[1][3] == 1 and _plan(8, 1, 65536, 16)[1][3] == 1
  code, p = _plan(8, 1, 65536, 65536)
  assert code == 0 and p == [1, _lds_bytes(8, 1, 256), THREADS, 256] and 256 * 8 * 20 == 40960
  assert _plan(159, 0, 65536, 65536) == (0, [2, 0, THREADS, 256])
  assert _plan(159, 0, 65536, 65536, path=1)[0] == EINVAL
  # P = 1 takes what wide_policy_update_kernel takes (its table bytes and one set of thresholds)
  assert _plan(159, 0, 65536, 1)[1] == [1, _lds_bytes(159, 0, 1), THREADS, 1]
  # n >= 256 that is no multiple of 256: a boundary lies inside a workgroup
  assert _plan(8, 0, 771, 3)[1][3] == 2 and _plan(8, 0, 514, 2)[1][3] == 2
  assert _plan(8, 0, 257, 1)[1][3] == 1


@pytest.mark.parametrize('perf', [0, 1])
@pytest.mark.parametrize('members,B,P', [(1, 512, 2), (256, 512, 512)])
def test_the_largest_table_that_fits_and_the_next(members, B, P, perf):
  assert _brute_members_per_block(B, P) == members
  S = 1
  while _lds_bytes(S + 1, perf, members) <= LDS_MAX:
    S += 1
  code, p = _plan(S, perf, B, P)
  assert code == 0 and p == [1, _lds_bytes(S, perf, members), THREADS, members]
  assert _plan(S + 1, perf, B, P) == (0, [2, 0, THREADS, members])
  assert _plan(S + 1, perf, B, P, path=1)[0] == EINVAL and _plan(S, perf, B, P, path=1)[0] == 0
  assert _plan(S, perf, B, P, path=2) == (0, [2, 0, THREADS, members])


def test_wide_lds_max_zero_forces_global_and_path_1_is_refused_then():
  for B, P in ((512, 2), (64, 64)):
    assert _plan(8, 1, B, P, lds_max=0)[1][:2] == [2, 0]
    assert _plan(8, 1, B, P, lds_max=0, path=1)[0] == EINVAL


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  assert _plan(8, 0, 512, 2)[0] == 0
  for S, perf, B, P in ((0, 0, 512, 2), (-1, 0, 512, 2), ((1 << 24) + 1, 0, 512, 2), (8, 2, 512, 2),
                        (8, -1, 512, 2), (8, 0, 0, 1), (8, 0, -4, 2), (8, 0, 1 << 32, 2),
                        (8, 0, 512, 0), (8, 0, 512, -1), (8, 0, 512, 3), (8, 0, 512, 1024),
                        (1 << 20, 0, 1 << 11, 1 << 11), (1 << 24, 0, 128, 128)):
    assert _plan(S, perf, B, P)[0] == EINVAL, (S, perf, B, P)
  assert _plan((1 << 20) - 1, 0, 1 << 11, 1 << 11)[0] == 0          # P * S = 2^31 - 2^11
  assert _plan(8, 0, (1 << 32) - 1, 1)[0] == 0
  assert _plan(8, 0, 512, 2, lds_max=-1)[0] == EINVAL
  assert _plan(8, 0, 512, 2, path=3)[0] == EINVAL and _plan(8, 0, 512, 2, path=-1)[0] == EINVAL
  assert _hip.lib.campx_wide_population_plan(8, 0, 512, 2, LDS_MAX, 0, None) == EINVAL


def _valid_spec(n_states):
  """A CampxWideSpec whose plain fields pass the launch's validation (a 4x4 board, one layer, one
  thing); it points at no table - the calls below are refused before one is looked at."""
  from campx_amd import gamespec
  spec = gamespec.CampxWideSpec()
  spec.magic, spec.version = gamespec.SPEC_MAGIC, gamespec.SPEC_VERSION
  spec.rows, spec.cols, spec.n_layers, spec.n_dyn = 4, 4, 1, 1
  spec.n_states = n_states
  return spec


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made."""
  from campx_amd import _hip, gamespec
  vp = ctypes.c_void_p
  f = _hip.lib.campx_wide_policy_population_launch
  fake = 0x1000
  fake_spec = ctypes.cast(fake, ctypes.POINTER(gamespec.CampxWideSpec))      # (never read)
  state = _hip.CampxState(pos=fake, done=fake, ret=None, pair_table=None)
  out = _hip.CampxOutputs(trace=fake)

  def call(spec=fake_spec, tables=vp(fake), st=state, policy=vp(fake), first=0, o=out, actions=vp(fake),
           states=vp(fake), B=512, T=4, members=3, path=0):
    return f(spec, tables, st, policy, 1, first, o, actions, states, B, T, 0, members, path, None)

  # 512 environments do not split into 3 blocks: refused before the spec is read
  assert call() == EINVAL
  assert call(members=0) == EINVAL and call(members=-2) == EINVAL and call(members=1024) == EINVAL
  assert call(spec=None, members=2) == EINVAL and call(tables=None, members=2) == EINVAL
  assert call(policy=None, members=2) == EINVAL and call(actions=None, members=2) == EINVAL
  assert call(st=_hip.CampxState(pos=None, done=fake), members=2) == EINVAL
  assert call(st=_hip.CampxState(pos=fake, done=None), members=2) == EINVAL
  assert call(o=_hip.CampxOutputs(trace=None), members=2) == EINVAL
  assert call(B=0, members=1) == EINVAL and call(T=0, members=2) == EINVAL
  assert call(first=-1, members=2) == EINVAL and call(B=1 << 32, members=2) == EINVAL
  assert call(policy=vp(fake + 2), members=2) == EINVAL and call(states=vp(fake + 2), members=2) == EINVAL
  assert call(o=_hip.CampxOutputs(trace=fake, scalar_pitch=256), members=2) == EINVAL      # pitch < B
  # A spec that passes validation, so that the launch reaches the plan and refuses by ITS verdict.
  # That it does pass: an all-zero spec is refused as a spec, this one is not.
  assert call(spec=ctypes.byref(gamespec.CampxWideSpec()), members=2) == ESPEC
  spec = _valid_spec(1 << 20)
  by = ctypes.byref(spec)
  assert call(spec=by, B=1 << 11, members=1 << 11) == EINVAL          # P * n_states = 2^31
  assert call(spec=by, B=1 << 11, members=1 << 11, path=2) == EINVAL
  assert call(spec=by, members=2, path=3) == EINVAL and call(spec=by, members=2, path=-1) == EINVAL
  # the control: only the plan knows that 2^20 states do not fit the LDS of a workgroup
  assert _plan(1 << 20, 0, 512, 2, path=1)[0] == EINVAL and _plan(1 << 20, 0, 512, 2, path=2)[0] == 0
  assert call(spec=by, members=2, path=1) == EINVAL
  # out.perf for a game without hidden performance
  assert call(spec=by, members=2, o=_hip.CampxOutputs(trace=fake, perf=fake)) == EINVAL


# ---------------------------------------------------------------- the reference itself

class _Table(object):
  """Three states.  (next, reward, done) per action:
       state 0   a0 (1, 1)   a1 (2, 0)   a2 (0, -1)   a3 (1, None)   a4 (0, 0)
       state 1   a0 (2, 1, DONE)   a1 (0, 0)   a2 (1, 1)   a3 (2, -1)   a4 (1, 0)
       state 2   a0 .. a3 (2, 0)   a4 (0, 1)"""
  n_states = 3
  st_next = np.array([[1, 2, 0, 1, 0], [2, 0, 1, 2, 1], [2, 2, 2, 2, 0]], np.int32)
  st_reward = np.array([[1, 0, -1, np.nan, 0], [1, 0, 1, -1, 0], [0, 0, 0, 0, 1]], F)
  st_done = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.uint8)
  st_discount = (1.0 - st_done).astype(F)
  st_perf = np.array([[0, 1, 0, 0, 0], [0, 0, -1, 0, 0], [0, 0, 0, 0, 2]], np.int8)
  st_reached = np.ones((3, 5), bool)


def _one_hot(actions):
  w = np.zeros((len(actions), 5), F)
  w[np.arange(len(actions)), actions] = 2.5
  return w


def _same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  if a.dtype.kind == 'f':
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
  return a.dtype == b.dtype and np.array_equal(a, b)


def test_members_own_equal_contiguous_blocks():
  assert pop_ref.members(6, 3).tolist() == [0, 0, 1, 1, 2, 2]
  assert pop_ref.members(4, 4).tolist() == [0, 1, 2, 3] and pop_ref.members(3, 1).tolist() == [0, 0, 0]
  with pytest.raises(AssertionError):
    pop_ref.members(5, 2)


def test_two_deterministic_members_by_hand():
  """Member 0: state 0 takes a0 (to 1, reward 1), state 1 a0 (to 2, reward 1, DONE), then row 0
  again.  Member 1: state 0 takes a1 (to 2, 0), state 2 a4 (to 0, reward 1), and round.  One-hot
  rows do not look at the random word."""
  policies = np.stack([_one_hot([0, 0, 4]), _one_hot([1, 4, 4])])
  walker = pop_ref.PopulationWalker(_Table, 4)
  out = walker.rollout(policies, 5, seed=7, reset_first=True)
  assert out['states'].dtype == np.int32 and out['actions'].dtype == np.int8
  # flat rows: member 1's are offset by n_states = 3
  assert out['states'].T.tolist() == [[0, 1, 0, 1, 0]] * 2 + [[3, 5, 3, 5, 3]] * 2
  assert out['actions'].T.tolist() == [[0] * 5] * 2 + [[1, 4, 1, 4, 1]] * 2
  assert out['done'].T.tolist() == [[0, 1, 0, 1, 0]] * 2 + [[0] * 5] * 2
  assert out['reward'].T.tolist() == [[1, 1, 1, 1, 1]] * 2 + [[0, 1, 0, 1, 0]] * 2
  assert out['discount'].T.tolist() == [[1, 0, 1, 0, 1]] * 2 + [[1] * 5] * 2
  assert out['perf'].T.tolist() == [[0] * 5] * 2 + [[1, 2, 1, 2, 1]] * 2
  assert walker.state.tolist() == [1, 1, 2, 2] and walker.over.tolist() == [False] * 4
  assert walker.ret.tolist() == [1, 1, 2, 2]           # member 0: the third episode's first reward
  assert out['bad'] == 0 and walker.frame == 5
  # a bad row in member 1 only: its environments take action 4 in state 0 and stay there
  policies[1, 0] = [1, -1, 1, 1, 1]
  out = pop_ref.PopulationWalker(_Table, 4).rollout(policies, 3, reset_first=True)
  assert out['bad'] == 6 and out['bad_by_member'].tolist() == [0, 6]
  assert out['actions'].T.tolist() == [[0, 0, 0]] * 2 + [[4, 4, 4]] * 2
  assert out['states'].T.tolist() == [[0, 1, 0]] * 2 + [[3, 3, 3]] * 2


@pytest.mark.parametrize('B,P', [(6, 1), (6, 3), (6, 6), (255, 3)])
def test_copies_of_one_policy_walk_what_the_policy_walker_walks(B, P):
  rng = np.random.RandomState(B + P)
  w = rng.uniform(0.05, 1.0, size=(3, 5)).astype(F)
  w[2, [1, 3]] = 0.0
  one, many = ref.PolicyWalker(_Table, B), pop_ref.PopulationWalker(_Table, B)
  offsets = pop_ref.members(B, P).astype(np.int32) * 3
  for T, kw in ((19, dict(reset_first=True)), (13, {}), (5, dict(first_frame=(1 << 40) + 6))):
    want = one.rollout(w, T, seed=0xfeedfacecafebeef, **kw)
    got = many.rollout(np.stack([w] * P), T, seed=0xfeedfacecafebeef, **kw)
    for k in ('actions', 'reward', 'discount', 'done', 'perf'):
      assert _same(got[k], want[k]), k
    assert _same(got['states'], want['states'] + offsets[None, :])
    assert got['bad'] == want['bad'] == 0
    assert np.array_equal(one.state, many.state) and np.array_equal(one.over, many.over)
    assert _same(one.ret, many.ret) and one.frame == many.frame
  assert len(np.unique(got['actions'])) > 1


def test_members_sample_their_own_rows():
  """Two different members from the same start: each block equals a walk of its own policy over
  the whole batch, cut to the block's environments (the counter is the absolute environment)."""
  B, P, T = 8, 2, 16
  rng = np.random.RandomState(3)
  policies = rng.uniform(0.05, 1.0, size=(P, 3, 5)).astype(F)
  got = pop_ref.PopulationWalker(_Table, B).rollout(policies, T, seed=11, reset_first=True)
  for m in range(P):
    want = ref.PolicyWalker(_Table, B).rollout(policies[m], T, seed=11, reset_first=True)
    cols = slice(m * 4, (m + 1) * 4)
    assert _same(got['actions'][:, cols], want['actions'][:, cols])
    assert _same(got['states'][:, cols], want['states'][:, cols] + np.int32(3 * m))
  assert not _same(got['actions'][:, :4], got['actions'][:, 4:])
