"""`campx_wide_population_solve_plan()` - pure host arithmetic - for the four forms of a population
of rewards and gammas (policy or greedy reduction by shared or per-member rewards), at the sizes
where the plan changes, and what `campx_wide_population_solve_launch()` refuses before it touches
a device (made-up pointers that no host code reads).  No kernel is launched here."""

import ctypes

import pytest

import wide_table_reference as ref

LDS_MAX = 144 * 1024
HEADER = 128
THREADS = 1024                 # of the LDS workgroup, at most
PACK = 256                     # pairs a workgroup is packed up to
MAX_GRID = 1 << 20
LIMIT = (1 << 31) - 1          # P * S * 5
FAKE = 0x1000
FORMS = [(1, 0), (1, 1), (0, 0), (0, 1)]     # (policy, per-member rewards)
BYTES_PER_STATE = {(1, 0): 72, (1, 1): 92, (0, 0): 48, (0, 1): 68}   # of one member, entries included


def _plan(S, P, policy, rewards, lds_max=LDS_MAX, n_cus=256, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_population_solve_plan(S, P, policy, rewards, lds_max, n_cus, path, out)
  return code, list(out)


def _up(x):
  return (x + 15) // 16 * 16


def _lds_bytes(S, G, policy, rewards):
  """The header's account of path 1: a header, the entries once (40 bytes a state), two residual
  slots and a gamma per member, and flat over the G * S pairs two value vectors (8 bytes a pair),
  for a policy the weights and the totals (24), with rewards per member those (20) - each part
  rounded up to 16 bytes."""
  n = HEADER + _up(40 * S) + _up(8 * G) + _up(4 * G) + 2 * _up(4 * G * S)
  if policy:
    n += _up(20 * G * S) + _up(4 * G * S)
  if rewards:
    n += _up(20 * G * S)
  return n


def _ceil(a, b):
  return (a + b - 1) // b


def _want(S, P, policy, rewards, lds_max=LDS_MAX, n_cus=256):
  """The rule, restated: G = min(what fits, floor(256 / S), ceil(P / n_cus)), never below 1."""
  if _lds_bytes(S, 1, policy, rewards) > lds_max:
    return [2, 0, 256, min(_ceil(S, 256) * P, MAX_GRID), 1]
  G = min(max(1, PACK // S), _ceil(P, n_cus))
  while _lds_bytes(S, G, policy, rewards) > lds_max:
    G -= 1
  return [1, _lds_bytes(S, G, policy, rewards), min(THREADS, _ceil(G * S, 64) * 64),
          min(_ceil(P, G), MAX_GRID), G]


def _largest(policy, rewards, lds_max=LDS_MAX):
  """The largest S whose one member the plan function puts in LDS, by bisection over it."""
  lo, hi = 1, 1 << 14
  assert _plan(lo, 1, policy, rewards, lds_max)[1][0] == 1 and _plan(hi, 1, policy, rewards, lds_max)[1][0] == 2
  while lo < hi:
    mid = (lo + hi + 1) // 2
    lo, hi = (mid, hi) if _plan(mid, 1, policy, rewards, lds_max)[1][0] == 1 else (lo, mid - 1)
  return lo


def test_exports_op_name_and_surface():
  from campx_amd import _hip, wide
  assert 'campx_wide_population_solve_plan' in _hip.EXPORTS
  assert 'campx_wide_population_solve_launch' in _hip.EXPORTS
  assert 'wide_population_solve' in _hip.OP_NAMES
  assert 'value_iteration_population' in wide.STATE_TABLE_ONLY
  assert _hip.config_get('wide_lds_max') == LDS_MAX


def test_the_policy_form_with_shared_rewards_is_the_population_plan():
  from campx_amd import _hip
  for S in (1, 8, 159, 2045, 2046):
    for P in (1, 17, 257, 65536):
      old = (ctypes.c_int64 * 5)()
      assert _hip.lib.campx_wide_population_sweeps_plan(S, P, 0, LDS_MAX, 256, 0, old) == 0
      assert _plan(S, P, 1, 0) == (0, list(old)), (S, P)


@pytest.mark.parametrize('policy,rewards', FORMS)
def test_lds_bytes_by_hand(policy, rewards):
  # S = 8, G = 1: 128 + 320 + 16 + 16 + 2 * 32, then 160 + 32 for a policy, 160 for rewards
  want = 544 + (192 if policy else 0) + (160 if rewards else 0)
  assert _lds_bytes(8, 1, policy, rewards) == want
  assert _plan(8, 1, policy, rewards) == (0, [1, want, 64, 1, 1])
  # per (member, state) beyond the shared entries: 8, +24 for a policy, +20 for rewards
  per_pair = 8 + (24 if policy else 0) + (20 if rewards else 0)
  assert BYTES_PER_STATE[(policy, rewards)] == 40 + per_pair
  # (the slots and gammas of two members round up to 32 bytes, of four to 48)
  assert _lds_bytes(64, 4, policy, rewards) - _lds_bytes(64, 2, policy, rewards) == 2 * 64 * per_pair + 16
  code, p = _plan(8, 65536, policy, rewards)
  assert code == 0 and p[4] == 32 and p[1] == _lds_bytes(8, 32, policy, rewards) and p[1] % 16 == 0


@pytest.mark.parametrize('policy,rewards', FORMS)
@pytest.mark.parametrize('n_cus', [1, 8, 256])
def test_the_plan_is_the_rule_at_every_size(policy, rewards, n_cus):
  S_max = _largest(policy, rewards)
  for S in (1, 5, 8, 37, 159, 257, 1024, 1025, S_max, S_max + 1):
    for P in (1, 16, 255, 256, 257, 2051, 65536):
      code, p = _plan(S, P, policy, rewards, n_cus=n_cus)
      assert code == 0 and p == _want(S, P, policy, rewards, n_cus=n_cus), (S, P, n_cus, p)


@pytest.mark.parametrize('policy,rewards', FORMS)
def test_members_per_workgroup_by_the_three_rules(policy, rewards):
  # (b) floor(256 / S) against (c) ceil(65536 / 256) = 256
  for S, G in ((1, 256), (8, 32), (159, 1), (128, 2), (129, 1), (1025, 1)):
    code, p = _plan(S, 65536, policy, rewards)
    assert code == 0 and p[0] == 1 and p[4] == G and p[3] == _ceil(65536, G), (S, p)
  # (c) a small population spreads first
  for P, G in ((1, 1), (16, 1), (256, 1), (257, 2), (2051, 9), (65536, 32)):
    assert _plan(8, P, policy, rewards)[1][3:] == [_ceil(P, G), G], P
  for P, G in ((1, 1), (16, 16), (255, 32)):
    assert _plan(8, P, policy, rewards, n_cus=1)[1][4] == G, P
  # (a) a lowered wide_lds_max bounds the members with THIS form's bytes
  for G in (1, 2, 3, 17, 31):
    lds = _lds_bytes(8, G, policy, rewards)
    code, p = _plan(8, 65536, policy, rewards, lds_max=lds, n_cus=1)
    assert code == 0 and p == [1, lds, min(1024, _ceil(8 * G, 64) * 64), _ceil(65536, G), G], G
    if G > 1:
      assert _plan(8, 65536, policy, rewards, lds_max=lds - 1, n_cus=1)[1][4] == G - 1
  one = _lds_bytes(8, 1, policy, rewards)
  assert _plan(8, 65536, policy, rewards, lds_max=one - 1) == (0, [2, 0, 256, 65536, 1])
  assert _plan(8, 65536, policy, rewards, lds_max=one - 1, path=1)[0] != 0


@pytest.mark.parametrize('policy,rewards', FORMS)
def test_the_largest_table_whose_one_member_fits_and_the_next(policy, rewards):
  S = _largest(policy, rewards)
  per = BYTES_PER_STATE[(policy, rewards)]
  # 128 + 32 bytes beside the states' own, and the roundings of up to six parts
  assert (LDS_MAX - 160 - 6 * 15) // per <= S <= (LDS_MAX - 160) // per
  assert _lds_bytes(S, 1, policy, rewards) <= LDS_MAX < _lds_bytes(S + 1, 1, policy, rewards)
  assert _plan(S, 300, policy, rewards) == (0, [1, _lds_bytes(S, 1, policy, rewards), 1024, 300, 1])
  blocks = _ceil(S + 1, 256)
  assert _plan(S + 1, 300, policy, rewards) == (0, [2, 0, 256, blocks * 300, 1])
  # forced either way: path 1 on the table that does not fit is refused
  assert _plan(S, 300, policy, rewards, path=2) == (0, [2, 0, 256, _ceil(S, 256) * 300, 1])
  assert _plan(S, 300, policy, rewards, path=1)[1][0] == 1
  assert _plan(S + 1, 300, policy, rewards, path=1)[0] != 0


def test_the_largest_tables_differ_per_form():
  largest = {form: _largest(*form) for form in FORMS}
  assert largest[(1, 0)] == 2045                      # evaluate_population()'s own
  assert largest[(0, 0)] > largest[(0, 1)] > largest[(1, 0)] > largest[(1, 1)]
  assert largest == {(1, 0): 2045, (1, 1): 1600, (0, 0): 3068, (0, 1): 2165}


@pytest.mark.parametrize('policy,rewards', FORMS)
def test_plan_refuses_bad_arguments_and_the_element_bound(policy, rewards):
  from campx_amd import _hip
  assert _hip.lib.campx_wide_population_solve_plan(8, 16, policy, rewards, LDS_MAX, 256, 0, None) != 0
  for S, P in ((0, 1), (-1, 1), ((1 << 24) + 1, 1), (8, 0), (8, -1)):
    assert _plan(S, P, policy, rewards)[0] != 0, (S, P)
  assert _plan(8, 16, 2, rewards)[0] != 0 and _plan(8, 16, -1, rewards)[0] != 0
  assert _plan(8, 16, policy, 2)[0] != 0 and _plan(8, 16, policy, -1)[0] != 0
  assert _plan(8, 16, policy, rewards, n_cus=0)[0] != 0 and _plan(8, 16, policy, rewards, lds_max=-1)[0] != 0
  assert _plan(8, 16, policy, rewards, path=3)[0] != 0 and _plan(8, 16, policy, rewards, path=-1)[0] != 0
  for S in (1, 8, 159, 1 << 24):
    most = LIMIT // (S * 5)
    assert most * S * 5 <= LIMIT < (most + 1) * S * 5
    assert _plan(S, most, policy, rewards)[0] == 0 and _plan(S, most, policy, rewards, path=2)[0] == 0, S
    assert _plan(S, most + 1, policy, rewards)[0] != 0 and _plan(S, most + 1, policy, rewards, path=2)[0] != 0, S
  assert _plan(8, 1 << 62, policy, rewards)[0] != 0


@pytest.fixture(scope='module')
def spec():
  from campx_amd import _hip, tabulate
  spec, arrays = tabulate.to_wide_spec(ref.make_table(4001, 4, 4, 2, 1, 3))
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0 and spec.n_states == 3
  return spec, arrays


def _launch(spec, **kw):
  """The launch with every argument valid unless named; v_in and v_out one array, the rest apart."""
  from campx_amd import _hip
  size = 1 << 20
  args = dict(tables=FAKE, policies=None, rewards=FAKE + size, members=4, reward=None, gamma=0.5,
              gammas=None, v_in=FAKE + 2 * size, v_out=FAKE + 2 * size, scratch=FAKE + 3 * size, q=None,
              greedy=FAKE + 6 * size, residual=FAKE + 4 * size, bad_rows=None, bad_flag=None, n_sweeps=3,
              path=2)
  args.update(kw)
  vp = lambda x: None if x is None else ctypes.c_void_p(x)
  by = ctypes.byref(spec) if spec is not None else None
  return _hip.lib.campx_wide_population_solve_launch(
      by, vp(args['tables']), vp(args['policies']), vp(args['rewards']), args['members'], vp(args['reward']),
      args['gamma'], vp(args['gammas']), vp(args['v_in']), vp(args['v_out']), vp(args['scratch']),
      vp(args['q']), vp(args['greedy']), vp(args['residual']), vp(args['bad_rows']), vp(args['bad_flag']),
      args['n_sweeps'], args['path'], None)


POLICY = dict(policies=FAKE + (7 << 20), greedy=None)      # the policy form of the same call

REFUSED = [
    ('null tables', dict(tables=None)),
    ('null v_in', dict(v_in=None)),
    ('null v_out', dict(v_out=None)),
    ('null residual', dict(residual=None)),
    ('null scratch on path 2', dict(scratch=None)),
    ('policy form null v_in', dict(POLICY, v_in=None)),
    ('policy form null scratch on path 2', dict(POLICY, scratch=None)),
    ('greedy beside policies', dict(policies=FAKE + (7 << 20))),
    ('rewards beside the shared override', dict(reward=FAKE + (5 << 20))),
    ('no member', dict(members=0)),
    ('members below zero', dict(members=-4)),
    ('too many elements', dict(members=LIMIT // 15 + 1)),
    ('no sweep', dict(n_sweeps=0)),
    ('a sweep too many', dict(n_sweeps=(1 << 20) + 1)),
    ('gamma nan', dict(gamma=float('nan'))),
    ('gamma inf', dict(gamma=float('inf'))),
    ('odd tables', dict(tables=FAKE + 4)),
    ('odd policies', dict(POLICY, policies=FAKE + (7 << 20) + 2)),
    ('odd rewards', dict(rewards=FAKE + (1 << 20) + 2)),
    ('odd rewards policy form', dict(POLICY, rewards=FAKE + (1 << 20) + 1)),
    ('odd gammas', dict(gammas=FAKE + (5 << 20) + 1)),
    ('odd shared reward', dict(rewards=None, reward=FAKE + (5 << 20) + 2)),
    ('odd q', dict(q=FAKE + (5 << 20) + 3)),
    ('odd residual', dict(residual=FAKE + (4 << 20) + 2)),
    ('odd bad_rows', dict(POLICY, bad_rows=FAKE + (5 << 20) + 2)),
    ('odd v_in', dict(v_in=FAKE + (5 << 20) + 2)),
    ('v_out into v_in', dict(v_out=FAKE + (2 << 20) + 4)),              # 4 members x 3 states x 4 bytes
    ('v_out just inside v_in', dict(v_out=FAKE + (2 << 20) + 44)),
    ('scratch is v_out', dict(scratch=FAKE + (2 << 20))),
    ('scratch into v_in', dict(v_in=FAKE + (5 << 20), scratch=FAKE + (5 << 20) + 44)),
    ('scratch into v_out', dict(v_in=FAKE + (5 << 20), scratch=FAKE + (2 << 20) - 44)),
    ('policy form scratch into v_out', dict(POLICY, v_in=FAKE + (5 << 20), scratch=FAKE + (2 << 20) - 44)),
    ('path 3', dict(path=3)),
    ('path -1', dict(path=-1)),
]


@pytest.mark.parametrize('case', REFUSED, ids=[c[0].replace(' ', '-') for c in REFUSED])
def test_launch_refuses_before_it_touches_a_device(spec, case):
  """Every refusal is decided by host arithmetic, in front of the first HIP call."""
  assert _launch(spec[0], **case[1]) != 0


def test_launch_refuses_no_spec_and_a_path_1_that_cannot_fit(spec):
  from campx_amd import _hip
  assert _launch(None) != 0
  with _hip.config(wide_lds_max=0):
    assert _launch(spec[0], path=1) != 0
    assert _launch(spec[0], path=0, scratch=None) != 0         # (path 0 is the global path then)
  # one member of three states with its rewards takes 128 + 128 + 16 + 16 + 2 * 16 + 64 bytes; the
  # same member without them 64 fewer: between the two, path 1 is refused for the rewards alone
  with _hip.config(wide_lds_max=383):
    assert _launch(spec[0], path=1) != 0
    assert _launch(spec[0], path=1, rewards=None, tables=None) != 0    # (only the NULL stops this one)
