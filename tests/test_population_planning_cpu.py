"""`campx_wide_population_sweeps_plan()` - pure host arithmetic - at the sizes where the plan of
`evaluate_population()` changes, and what `campx_wide_population_sweeps_launch()` refuses before it
touches a device (made-up pointers that no host code reads).  No kernel is launched here."""

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


def _plan(S, P, override=0, lds_max=LDS_MAX, n_cus=256, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_population_sweeps_plan(S, P, override, lds_max, n_cus, path, out)
  return code, list(out)


def _up(x):
  return (x + 15) // 16 * 16


def _lds_bytes(S, G):
  """The header's account of path 1: a header, the entries once, two residual slots and a gamma per
  member, and per member two value vectors, the weights and the totals - flat over the G * S
  pairs, each part rounded up to 16 bytes."""
  return (HEADER + _up(40 * S) + _up(8 * G) + _up(4 * G) + 2 * _up(4 * G * S) + _up(20 * G * S)
          + _up(4 * G * S))


def _ceil(a, b):
  return (a + b - 1) // b


def _want(S, P, lds_max=LDS_MAX, n_cus=256):
  """The rule, restated: G = min(what fits, floor(256 / S), ceil(P / n_cus)), never below 1."""
  if _lds_bytes(S, 1) > lds_max:
    return [2, 0, 256, min(_ceil(S, 256) * P, MAX_GRID), 1]
  G = min(max(1, PACK // S), _ceil(P, n_cus))
  while _lds_bytes(S, G) > lds_max:
    G -= 1
  return [1, _lds_bytes(S, G), min(THREADS, _ceil(G * S, 64) * 64), min(_ceil(P, G), MAX_GRID), G]


def _largest():
  S = 1
  while _lds_bytes(S + 1, 1) <= LDS_MAX:
    S += 1
  return S


def test_exports_and_op_name():
  from campx_amd import _hip, wide
  assert 'campx_wide_population_sweeps_plan' in _hip.EXPORTS
  assert 'campx_wide_population_sweeps_launch' in _hip.EXPORTS
  assert 'wide_population_sweeps' in _hip.OP_NAMES
  assert _hip.config_get('wide_lds_max') == LDS_MAX
  assert 'evaluate_population' in wide.STATE_TABLE_ONLY
  assert 'population_sweep_buffers' in wide.STATE_TABLE_ONLY


def test_members_per_workgroup_by_hand():
  # a large population on the whole chip: (b) floor(256 / S) against (c) ceil(65536 / 256) = 256
  for S, G in ((1, 256), (8, 32), (159, 1), (128, 2), (129, 1), (1024, 1), (1025, 1)):
    code, p = _plan(S, 65536)
    assert code == 0 and p[0] == 1 and p[4] == G, (S, p)
    assert p[3] == _ceil(65536, G) and p[1] == _lds_bytes(S, G) and p[1] % 16 == 0
  # on one compute unit (c) never binds: (b) alone
  for S, G in ((1, 256), (8, 32), (159, 1), (1024, 1), (1025, 1)):
    assert _plan(S, 65536, n_cus=1)[1][4] == G, S
  # a small population spreads first: one member per workgroup up to one workgroup per CU
  for P, G in ((1, 1), (16, 1), (255, 1), (256, 1), (257, 2), (65536, 32)):
    code, p = _plan(8, P)
    assert code == 0 and p[4] == G and p[3] == _ceil(P, G), (P, p)
  for P, G in ((1, 1), (16, 16), (255, 32), (256, 32), (257, 32)):
    assert _plan(8, P, n_cus=1)[1][4] == G, P
  # threads: whole waves over the G * S pairs, 1 024 at most
  assert _plan(8, 16)[1][2] == 64 and _plan(8, 16, n_cus=1)[1][2] == 128
  assert _plan(159, 65536)[1][2] == 192 and _plan(37, 65536)[1][2:] == [256, 10923, 6]
  assert _plan(8, 65536)[1][2] == 256 and _plan(1, 65536)[1][2] == 256
  assert _plan(5, 17, n_cus=1)[1][2] == 128 and _plan(1025, 3)[1][2] == 1024


@pytest.mark.parametrize('n_cus', [1, 256])
@pytest.mark.parametrize('P', [1, 16, 255, 256, 257, 65536])
def test_the_plan_is_the_rule_at_every_size(P, n_cus):
  S_max = _largest()
  for S in (1, 8, 159, 1024, 1025, S_max, S_max + 1):
    for override in (0, 1):
      code, p = _plan(S, P, override, n_cus=n_cus)
      assert code == 0 and p == _want(S, P, n_cus=n_cus), (S, P, n_cus, p)


def test_the_largest_table_that_fits_and_the_next():
  S = _largest()
  assert S == 2045 and _lds_bytes(S, 1) == LDS_MAX          # 72 bytes per state, and the roundings
  assert _plan(S, 300) == (0, [1, LDS_MAX, 1024, 300, 1])
  assert _plan(S + 1, 300) == (0, [2, 0, 256, _ceil(S + 1, 256) * 300, 1])
  # forced either way
  assert _plan(S, 300, path=2) == (0, [2, 0, 256, 8 * 300, 1])
  assert _plan(S, 300, path=1)[1][0] == 1
  assert _plan(S + 1, 300, path=1)[0] != 0
  assert _plan(8, 65536, path=2) == (0, [2, 0, 256, 65536, 1])   # past grid.y's 65 535: along x
  assert _plan(257, 3, path=2)[1][3] == 6


def test_a_lowered_wide_lds_max_bounds_the_members():
  # S = 8, P = 65536, one CU: (b) says 32; LDS says less
  for G in (1, 2, 3, 17, 31):
    lds = _lds_bytes(8, G)
    code, p = _plan(8, 65536, lds_max=lds, n_cus=1)
    assert code == 0 and p == [1, lds, min(1024, _ceil(8 * G, 64) * 64), _ceil(65536, G), G], G
    if G > 1:
      assert _plan(8, 65536, lds_max=lds - 1, n_cus=1)[1][4] == G - 1
  one = _lds_bytes(8, 1)
  assert _plan(8, 65536, lds_max=one - 1) == (0, [2, 0, 256, 65536, 1])
  assert _plan(8, 65536, lds_max=one - 1, path=1)[0] != 0
  assert _plan(8, 65536, lds_max=0) == (0, [2, 0, 256, 65536, 1])
  assert _plan(8, 65536, lds_max=0, path=1)[0] != 0


def test_the_grid_stops_at_two_to_the_twenty():
  P = (1 << 20) + 3
  assert _plan(1, P, path=2)[1][3] == MAX_GRID
  assert _plan(1, P, lds_max=_lds_bytes(1, 1))[1][3:] == [MAX_GRID, 1]
  assert _plan(1, P)[1][3:] == [_ceil(P, 256), 256]


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  assert _hip.lib.campx_wide_population_sweeps_plan(8, 16, 0, LDS_MAX, 256, 0, None) != 0
  for S, P in ((0, 1), (-1, 1), ((1 << 24) + 1, 1), (8, 0), (8, -1)):
    assert _plan(S, P)[0] != 0, (S, P)
  assert _plan(8, 16, override=2)[0] != 0 and _plan(8, 16, override=-1)[0] != 0
  assert _plan(8, 16, n_cus=0)[0] != 0 and _plan(8, 16, lds_max=-1)[0] != 0
  assert _plan(8, 16, path=3)[0] != 0 and _plan(8, 16, path=-1)[0] != 0


def test_the_limit_on_the_elements_of_the_policies():
  for S in (1, 8, 159, 1 << 24):
    most = LIMIT // (S * 5)
    assert most * S * 5 <= LIMIT < (most + 1) * S * 5
    assert _plan(S, most)[0] == 0 and _plan(S, most, path=2)[0] == 0, S
    assert _plan(S, most + 1)[0] != 0 and _plan(S, most + 1, path=2)[0] != 0, S
  assert _plan(8, 1 << 62)[0] != 0


@pytest.fixture(scope='module')
def spec():
  from campx_amd import _hip, tabulate
  spec, arrays = tabulate.to_wide_spec(ref.make_table(4001, 4, 4, 2, 1, 3))
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0 and spec.n_states == 3
  return spec, arrays


def _launch(spec, **kw):
  """The launch with every argument valid unless named; v_in and v_out one array, the rest apart."""
  from campx_amd import _hip
  P, S = kw.get('members', 4), 3
  size = 1 << 20
  args = dict(tables=FAKE, policies=FAKE + size, members=P, reward=None, gamma=0.5, gammas=None,
              v_in=FAKE + 2 * size, v_out=FAKE + 2 * size, scratch=FAKE + 3 * size, q=None,
              residual=FAKE + 4 * size, bad_rows=None, bad_flag=None, n_sweeps=3, path=2)
  args.update(kw)
  vp = lambda x: None if x is None else ctypes.c_void_p(x)
  by = ctypes.byref(spec) if spec is not None else None
  return _hip.lib.campx_wide_population_sweeps_launch(
      by, vp(args['tables']), vp(args['policies']), args['members'], vp(args['reward']), args['gamma'],
      vp(args['gammas']), vp(args['v_in']), vp(args['v_out']), vp(args['scratch']), vp(args['q']),
      vp(args['residual']), vp(args['bad_rows']), vp(args['bad_flag']), args['n_sweeps'], args['path'], None)


REFUSED = [
    ('null tables', dict(tables=None)),
    ('null policies', dict(policies=None)),
    ('null v_in', dict(v_in=None)),
    ('null v_out', dict(v_out=None)),
    ('null residual', dict(residual=None)),
    ('null scratch on path 2', dict(scratch=None)),
    ('no member', dict(members=0)),
    ('members below zero', dict(members=-4)),
    ('too many elements', dict(members=LIMIT // 15 + 1)),
    ('no sweep', dict(n_sweeps=0)),
    ('a sweep too many', dict(n_sweeps=(1 << 20) + 1)),
    ('gamma nan', dict(gamma=float('nan'))),
    ('gamma inf', dict(gamma=float('inf'))),
    ('odd tables', dict(tables=FAKE + 4)),
    ('odd policies', dict(policies=FAKE + (1 << 20) + 2)),
    ('odd gammas', dict(gammas=FAKE + (5 << 20) + 1)),
    ('odd reward', dict(reward=FAKE + (5 << 20) + 2)),
    ('odd q', dict(q=FAKE + (5 << 20) + 3)),
    ('odd residual', dict(residual=FAKE + (4 << 20) + 2)),
    ('odd bad_rows', dict(bad_rows=FAKE + (5 << 20) + 2)),
    ('v_out into v_in', dict(v_out=FAKE + (2 << 20) + 4)),              # 4 members x 3 states x 4 bytes
    ('v_out just inside v_in', dict(v_out=FAKE + (2 << 20) + 44)),
    ('scratch is v_out', dict(scratch=FAKE + (2 << 20))),
    ('scratch into v_in', dict(v_in=FAKE + (5 << 20), scratch=FAKE + (5 << 20) + 44)),
    ('scratch into v_out', dict(v_in=FAKE + (5 << 20), scratch=FAKE + (2 << 20) - 44)),
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
