"""The population form of the visitation rule without a GPU: its numpy restatement
(tests/visitation_population_reference.py) against the single-policy one member by member,
`campx_wide_visit_population_plan()` - pure host arithmetic - against the rule restated here, and
what `campx_wide_visit_population_launch()` refuses before it touches a device (made-up pointers
that no host code reads).  No kernel is launched here."""

import ctypes
import functools

import numpy as np
import pytest

import visitation_population_reference as pop_ref
import visitation_reference as visit_ref
import wide_table_reference as ref

UNIT = 1 << 38
LDS_MAX = 144 * 1024
HEADER = 64                    # of the single call's plan: the first member's two slots of finished[t]
MEMBER_HEADER = 16             # the two slots of each further member
THREADS = 1024                 # of the LDS workgroup, at most
PER_LANE = 3                   # states a lane of it owns, at most
PACK = 256                     # pairs a workgroup is packed up to
MAX_GRID = 1 << 20
LIMIT = (1 << 31) - 1          # P * S * 5
FAKE = 0x100000


# ---------------------------------------------------------------- the reference

@functools.lru_cache(maxsize=None)
def _table(S):
  return ref.make_table(9100 + S, 4, 4, 2, 1, S)


def _policies(P, S, seed, bad=()):
  rng = np.random.RandomState(seed)
  w = rng.uniform(0.25, 2.0, size=(P, S, 5)).astype(np.float32)
  w[rng.rand(P, S, 5) < 0.2] = 0
  w[:, np.arange(S), rng.randint(0, 5, size=S)] = 1.25              # (no row is all zero)
  for k, (m, s) in enumerate(bad):
    w[m, s, k % 5] = (-1.0, np.nan, np.inf)[k % 3]
  return w


def _starts(P, S, kind, seed):
  rng = np.random.RandomState(seed)
  if kind == 'none':
    return None
  shape = (S,) if kind.startswith('shared') else (P, S)
  p = rng.rand(*shape) * (rng.rand(*shape) < 0.6)
  p[..., rng.randint(S)] += 1.0
  p /= p.sum(axis=-1, keepdims=True)
  if kind.endswith('float'):
    return p.astype(np.float32)
  d = np.floor(p * (UNIT // 2)).astype(np.int64)
  if kind == 'member':
    d[P // 2] = 0                                                    # a member with no mass at all
  return d


@pytest.mark.parametrize('S', [1, 8, 37])
@pytest.mark.parametrize('P', [1, 3])
def test_the_population_reference_is_the_single_reference_member_by_member(S, P):
  g = _table(S)
  bad = [(P - 1, 0), (0, S - 1), (P // 2, S // 2)]
  for seed, restart, kind, spoiled in ((1, True, 'none', ()), (2, False, 'shared', bad), (3, True, 'member', bad),
                                       (4, False, 'member float', ()), (5, True, 'shared float', bad[:1])):
    w = _policies(P, S, seed + 10 * S, spoiled)
    start = _starts(P, S, kind, seed)
    for frames in (1, 6):
      got = pop_ref.visitation(g.st_next, g.st_done, w, frames, start=start, restart=restart)
      n_bad = 0
      for m in range(P):
        own = None if start is None else (start if start.ndim == 1 else start[m])
        if own is not None and own.dtype != np.int64:
          own = visit_ref.quantise(own)
        one = visit_ref.visitation(g.st_next, g.st_done, w[m], frames, start=own, restart=restart)
        what = (S, P, m, frames, restart, kind)
        assert np.array_equal(got['visits'][m], one['visits']), what
        assert np.array_equal(got['finished'][:, m], one['finished']), what
        assert np.array_equal(got['final'][m], one['final']), what
        assert np.array_equal(got['per_frame'][:, m], one['per_frame']), what
        assert np.array_equal(got['counts'][m], one['counts']), what
        n_bad += one['bad_rows']
      assert got['bad_rows'] == n_bad == len({(m, s) for m, s in spoiled})
      assert got['visits'].dtype == got['finished'].dtype == got['final'].dtype == np.int64
      assert got['counts'].dtype == np.int32 and got['finished'].shape == (frames, P)
      assert got['per_frame'].shape == (frames + 1, P, S)
      if restart:
        assert np.array_equal(got['final'].sum(axis=1), got['per_frame'][0].sum(axis=1))


# ---------------------------------------------------------------- the plan's arithmetic

def _plan(S, P, lds_max=LDS_MAX, n_cus=256, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_visit_population_plan(S, P, lds_max, n_cus, path, out)
  return code, list(out)


def _single_plan(S, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_visit_plan(S, lds_max, path, out)
  return code, list(out)


def _up(x):
  return (x + 15) // 16 * 16


def _ceil(a, b):
  return (a + b - 1) // b


def _lds_bytes(S, G):
  """The header's account of path 1: the single call's header and 16 bytes for each member after
  the first, the entries' second words once (20 bytes a state), and per member N (16 bytes a
  state) and two mass vectors (8 each), flat over the G * S pairs, each part rounded up to 16."""
  return HEADER + MEMBER_HEADER * (G - 1) + _up(20 * S) + _up(16 * G * S) + 2 * _up(8 * G * S)


def _want(S, P, lds_max=LDS_MAX, n_cus=256, path=0):
  """The rule, restated: path 1 whenever one member fits; G = min(what fits, floor(256 / S),
  ceil(P / n_cus)), never below 1."""
  fits = _lds_bytes(S, 1) <= lds_max and S <= THREADS * PER_LANE
  if path == 2 or (path == 0 and not fits):
    return [2, 0, 256, min(_ceil(S, 256) * P, MAX_GRID), 1]
  assert fits
  G = min(max(1, PACK // S), _ceil(P, n_cus))
  while _lds_bytes(S, G) > lds_max:
    G -= 1
  return [1, _lds_bytes(S, G), min(THREADS, _ceil(G * S, 64) * 64), min(_ceil(P, G), MAX_GRID), G]


def _largest():
  S = 1
  while _lds_bytes(S + 1, 1) <= LDS_MAX:
    S += 1
  return S


def test_exports_op_name_and_the_tier_s_own_names():
  from campx_amd import _hip, wide
  assert 'campx_wide_visit_population_plan' in _hip.EXPORTS
  assert 'campx_wide_visit_population_launch' in _hip.EXPORTS
  assert 'wide_visit_population' in _hip.OP_NAMES
  assert _hip.config_get('wide_lds_max') == LDS_MAX
  assert 'visit_population' in wide.STATE_TABLE_ONLY
  assert 'visit_population_buffers' in wide.STATE_TABLE_ONLY


@pytest.mark.parametrize('n_cus', [1, 256])
@pytest.mark.parametrize('P', [1, 16, 255, 256, 257, 65536])
def test_the_plan_is_the_rule_at_every_size(P, n_cus):
  S_max = _largest()
  for S in (1, 8, 37, 159, 256, 257, 1024, 1025, S_max, S_max + 1):
    for path in (0, 2) + ((1,) if S <= S_max else ()):
      code, p = _plan(S, P, n_cus=n_cus, path=path)
      assert code == 0 and p == _want(S, P, n_cus=n_cus, path=path), (S, P, n_cus, path, p)
      assert p[1] % 16 == 0
    if S > S_max:
      assert _plan(S, P, n_cus=n_cus, path=1)[0] != 0


def test_members_per_workgroup_by_hand():
  for S, G in ((1, 256), (8, 32), (37, 6), (128, 2), (129, 1), (159, 1), (1025, 1)):
    code, p = _plan(S, 65536)
    assert code == 0 and p[0] == 1 and p[4] == G and p[3] == _ceil(65536, G), (S, p)
  # a small population spreads first: one member per workgroup up to one workgroup per CU
  for P, G in ((1, 1), (16, 1), (256, 1), (257, 2), (8200, 32), (65536, 32)):
    assert _plan(8, P)[1][3:] == [_ceil(P, G), G], P
  assert _plan(8, 16, n_cus=1)[1][2:] == [128, 1, 16]
  # with G > 1 the pairs have a lane each, in whole waves, 256 at most
  assert _plan(37, 65536)[1][2] == 256 and _plan(8, 257)[1][2] == 64 and _plan(1, 65536)[1][2] == 256
  # with G = 1 up to 1 024 lanes own up to three states each
  assert _plan(1025, 3)[1][2] == 1024 and _plan(159, 3)[1][2] == 192


def test_at_one_member_per_workgroup_the_account_is_the_single_call_s():
  S_max = _largest()
  assert S_max == 2834
  for S in (1, 8, 37, 159, 256, 257, 1024, 1025, S_max):
    code, single = _single_plan(S)
    assert code == 0 and single[0] == 1
    for P in (1, 200):
      code, p = _plan(S, P)
      assert code == 0 and p[4] == 1 and p[:3] == single[:3], (S, P, p, single)
  # the largest table that fits is the same one, whatever the ceiling
  for lds_max in (LDS_MAX, 64 * 1024, 4096, 200, 1 << 20):
    for S in range(1, 4000, 7):
      assert (_plan(S, 3, lds_max=lds_max)[1][0] == 1) == (_single_plan(S, lds_max=lds_max)[1][0] == 1), \
          (S, lds_max)
  assert _plan(S_max + 1, 3) == (0, [2, 0, 256, _ceil(S_max + 1, 256) * 3, 1])
  assert _plan(THREADS * PER_LANE, 3, lds_max=1 << 20)[1][0] == 1
  assert _plan(THREADS * PER_LANE + 1, 3, lds_max=1 << 20)[1][0] == 2
  assert _plan(THREADS * PER_LANE + 1, 3, lds_max=1 << 20, path=1)[0] != 0


def test_the_single_plan_is_the_first_four_words_of_one_member_s_at_every_input():
  """campx_wide_visit_plan(S, lds_max, path) against campx_wide_visit_population_plan(S, 1, lds_max,
  n_cus, path): the same return code and the same first four words for every input, refused ones
  included - the words are pre-filled, so that one a call leaves untouched shows as the canary."""
  from campx_amd import _hip
  single_fn, members_fn = _hip.lib.campx_wide_visit_plan, _hip.lib.campx_wide_visit_population_plan
  canary = -0x5a5a5a5a5a5a5a5b
  most = 1 << 24                                 # CAMPX_WIDE_MAX_STATES

  def largest(lds_max):
    S = 1
    while _lds_bytes(S + 1, 1) <= lds_max:
      S += 1
    return S

  sizes = set(range(1, 4097)) | {0, -1}
  for centre in (largest(64 * 1024), largest(LDS_MAX), most):
    sizes |= set(range(centre - 2, centre + 3))
  assert largest(LDS_MAX) == 2834 and max(sizes) == most + 2
  one, five = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 5)()
  calls = refused = 0
  for S in sorted(sizes):
    for lds_max in (-1, 0, _lds_bytes(1, 1), 64 * 1024, LDS_MAX):
      for path in (-1, 0, 1, 2, 3):
        one[:] = [canary] * 4
        code = single_fn(S, lds_max, path, one)
        words = list(one)
        assert (code == 0) == (canary not in words), (S, lds_max, path, code, words)
        for n_cus in (1, 256):
          five[:] = [canary] * 5
          got = members_fn(S, 1, lds_max, n_cus, path, five)
          assert got == code and list(five)[:4] == words, (S, lds_max, path, n_cus, code, got, words, list(five))
          assert five[4] == (1 if code == 0 else canary), (S, lds_max, path, n_cus, list(five))
        calls += 1
        refused += code != 0
  assert calls == len(sizes) * 25 and 0 < refused < calls
  # fewer than one compute unit is the population's alone to refuse
  five[:] = [canary] * 5
  assert members_fn(8, 1, LDS_MAX, 0, 0, five) != 0 and list(five) == [canary] * 5
  assert single_fn(8, LDS_MAX, 0, one) == 0


def test_a_lowered_wide_lds_max_bounds_the_members():
  # S = 8, P = 65536, one CU: (b) says 32; LDS says less
  for G in (1, 2, 3, 17, 31):
    lds = _lds_bytes(8, G)
    code, p = _plan(8, 65536, lds_max=lds, n_cus=1)
    assert code == 0 and p == [1, lds, _ceil(8 * G, 64) * 64, _ceil(65536, G), G], G
    if G > 1:
      assert _plan(8, 65536, lds_max=lds - 1, n_cus=1)[1][4] == G - 1
  one = _lds_bytes(8, 1)
  assert _plan(8, 65536, lds_max=one - 1) == (0, [2, 0, 256, 65536, 1])
  assert _plan(8, 65536, lds_max=one - 1, path=1)[0] != 0
  assert _plan(8, 65536, lds_max=0, path=1)[0] != 0


def test_the_grid_stops_at_two_to_the_twenty():
  P = (1 << 20) + 3
  assert _plan(1, P, path=2)[1][3] == MAX_GRID
  assert _plan(1, P, lds_max=_lds_bytes(1, 1))[1][3:] == [MAX_GRID, 1]
  assert _plan(1, P)[1][3:] == [_ceil(P, 256), 256]
  assert _plan(257, 3, path=2)[1][3] == 6


def test_plan_refuses_bad_arguments_and_too_many_elements():
  from campx_amd import _hip
  assert _hip.lib.campx_wide_visit_population_plan(8, 16, LDS_MAX, 256, 0, None) != 0
  for S, P in ((0, 1), (-1, 1), ((1 << 24) + 1, 1), (8, 0), (8, -1), (8, 1 << 62)):
    assert _plan(S, P)[0] != 0, (S, P)
  assert _plan(8, 16, n_cus=0)[0] != 0 and _plan(8, 16, lds_max=-1)[0] != 0
  assert _plan(8, 16, path=3)[0] != 0 and _plan(8, 16, path=-1)[0] != 0
  for S in (1, 8, 159, 1 << 24):
    most = LIMIT // (S * 5)
    assert _plan(S, most)[0] == 0 and _plan(S, most, path=2)[0] == 0, S
    assert _plan(S, most + 1)[0] != 0 and _plan(S, most + 1, path=2)[0] != 0, S


# ---------------------------------------------------------------- the launch's validator

@pytest.fixture(scope='module')
def spec():
  from campx_amd import _hip, tabulate
  spec, arrays = tabulate.to_wide_spec(ref.make_table(4001, 4, 4, 2, 1, 3))
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0 and spec.n_states == 3
  return spec, arrays


ORDER = ('tables', 'policies', 'members', 'start', 'per_member', 'restart', 'frames', 'visits', 'finished',
         'final', 'per_frame', 'counts', 'scratch', 'bad_rows', 'bad_flag', 'path')
POINTERS = ('tables', 'policies', 'start', 'visits', 'finished', 'final', 'per_frame', 'counts', 'scratch',
            'bad_rows', 'bad_flag')
M = 1 << 20                    # the made-up arrays are 1 MiB apart
BYTES = 4 * 3 * 8              # of final: 4 members x 3 states x 8 bytes


def _launch(spec, **kw):
  """The launch with every argument valid unless named: 4 members of 3 states, a start per member
  that is not `final`, path 2."""
  from campx_amd import _hip
  args = dict(tables=FAKE, policies=FAKE + M, members=4, start=FAKE + 2 * M, per_member=1, restart=1,
              frames=7, visits=FAKE + 3 * M, finished=FAKE + 4 * M, final=FAKE + 5 * M,
              per_frame=FAKE + 6 * M, counts=FAKE + 7 * M, scratch=FAKE + 8 * M, bad_rows=FAKE + 9 * M,
              bad_flag=FAKE + 10 * M, path=2)
  args.update(kw)
  vp = lambda x: None if x is None else ctypes.c_void_p(x)
  values = [vp(args[k]) if k in POINTERS else args[k] for k in ORDER]
  by = ctypes.byref(spec) if spec is not None else None
  return _hip.lib.campx_wide_visit_population_launch(by, *values, None)


REFUSED = [
    ('null tables', dict(tables=None)),
    ('null policies', dict(policies=None)),
    ('null visits', dict(visits=None)),
    ('null finished', dict(finished=None)),
    ('null final', dict(final=None)),
    ('null counts', dict(counts=None)),
    ('null scratch on path 2', dict(scratch=None)),
    ('no member', dict(members=0)),
    ('members below zero', dict(members=-4)),
    ('too many elements', dict(members=LIMIT // 15 + 1)),
    ('no frame', dict(frames=0)),
    ('frames below zero', dict(frames=-1)),
    ('a frame too many', dict(frames=(1 << 20) + 1)),
    ('restart 2', dict(restart=2)),
    ('restart -1', dict(restart=-1)),
    ('per_member 2', dict(per_member=2)),
    ('per_member -1', dict(per_member=-1)),
    ('path 3', dict(path=3)),
    ('path -1', dict(path=-1)),
    ('odd tables', dict(tables=FAKE + 4)),
    ('odd start', dict(start=FAKE + 2 * M + 4)),
    ('odd visits', dict(visits=FAKE + 3 * M + 4)),
    ('odd finished', dict(finished=FAKE + 4 * M + 4)),
    ('odd final', dict(final=FAKE + 5 * M + 4)),
    ('odd per_frame', dict(per_frame=FAKE + 6 * M + 4)),
    ('odd scratch', dict(scratch=FAKE + 8 * M + 4)),
    ('odd policies', dict(policies=FAKE + M + 2)),
    ('odd counts', dict(counts=FAKE + 7 * M + 2)),
    ('odd bad_rows', dict(bad_rows=FAKE + 9 * M + 2)),
    ('odd bad_flag', dict(bad_flag=FAKE + 10 * M + 2)),
    ('final one element into the start', dict(final=FAKE + 2 * M + 8)),
    ('final just inside the start', dict(final=FAKE + 2 * M - (BYTES - 8))),
    ('a shared start that is final', dict(per_member=0, start=FAKE + 5 * M)),
    ('a shared start inside final', dict(per_member=0, start=FAKE + 5 * M + BYTES - 8)),
    ('a shared start whose end is in final', dict(per_member=0, start=FAKE + 5 * M - 16)),
    ('scratch is final', dict(scratch=FAKE + 5 * M)),
    ('scratch just inside final', dict(scratch=FAKE + 5 * M + BYTES - 8)),
    ('scratch is the start', dict(scratch=FAKE + 2 * M)),
    ('scratch is the start and final', dict(scratch=FAKE + 2 * M, final=FAKE + 2 * M)),
    ('a shared start inside scratch', dict(per_member=0, start=FAKE + 8 * M + BYTES - 8)),
]


@pytest.mark.parametrize('case', REFUSED, ids=[c[0].replace(' ', '-') for c in REFUSED])
def test_launch_refuses_before_it_touches_a_device(spec, case):
  """Every refusal is decided by host arithmetic, in front of the first HIP call: each is the
  argument error itself, CAMPX_EINVAL."""
  from campx_amd import _hip
  einval = _hip.lib.campx_wide_visit_population_plan(0, 0, 0, 0, 0, None)
  assert einval != 0 and _launch(spec[0], **case[1]) == einval


def test_launch_refuses_no_spec_a_broken_one_and_a_path_1_that_cannot_fit(spec):
  from campx_amd import _hip
  assert _launch(None) != 0
  broken = type(spec[0]).from_buffer_copy(bytes(ctypes.sizeof(spec[0])))
  assert _launch(broken) != 0
  with _hip.config(wide_lds_max=0):
    assert _launch(spec[0], path=1) != 0
    assert _launch(spec[0], path=0, scratch=None) != 0         # (path 0 is the global path then)
