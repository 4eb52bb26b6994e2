"""The visitation rule's numpy restatement (tests/visitation_reference.py) against the sampler it
describes (tests/policy_reference.py), against planning (tests/planning_reference.py) and against
itself, and `campx_wide_visit_plan()` / the validator of `campx_wide_visit_launch()`, pure host
code.  No kernel is launched here."""

import ctypes
import functools

import numpy as np
import pytest

import planning_reference as plan_ref
import policy_reference as policy_ref
import visitation_reference as visit_ref
import wide_table_reference as ref

F = np.float32
UNIT = 1 << 38
WORDS = 1 << 24
SUB = 2.0 ** -140                 # a float32 subnormal (on the GPU: tests/test_float_edges.py)

ROWS = {
    'random': [0.731, 1.914, 0.502, 1.333, 0.871],
    'random_uneven': [3.0e-3, 17.25, 1.0e-6, 0.4375, 2.0],
    'one_hot': [0, 0, 1, 0, 0],
    'zero_last_weight': [1.5, 0.25, 0, 2.0, 0],
    'subnormal': [SUB, 3 * SUB, 0, 2 * SUB, SUB],
    'bad_negative': [1, 1, -0.5, 1, 1],
    'bad_infinite_total': [3e38, 3e38, 1, 0, 0],
}


@functools.lru_cache(maxsize=None)
def _table(S=8, seed=3):
  return ref.make_table(seed, 4, 4, 2, 1, S)


def _policy(S, seed, zeros=True):
  rng = np.random.RandomState(seed)
  w = rng.uniform(0.25, 2.0, size=(S, 5)).astype(F)
  if zeros:
    w[rng.rand(S, 5) < 0.2] = 0
    w[np.arange(S), rng.randint(0, 5, size=S)] = 1.25          # (no row is all zero)
  return w


# ---------------------------------------------------------------- the counts

@pytest.mark.parametrize('name', sorted(ROWS))
def test_bisection_counts_equal_a_brute_force_count_of_the_sampler(name):
  row = np.array(ROWS[name], F)
  words = np.arange(WORDS, dtype=np.uint32) << np.uint32(8)         # every 24-bit value u, once
  actions, bad = policy_ref.sample(words, row)
  brute = np.bincount(actions, minlength=5).astype(np.int64)
  N, is_bad = visit_ref.cumulative_counts(row[None, :])
  counts = visit_ref.counts_of(N)
  assert counts.dtype == np.int32 and counts.shape == (1, 5)
  assert np.array_equal(counts[0], brute), (name, counts[0], brute)
  assert int(counts.sum()) == WORDS and N[0, 4] == WORDS
  assert bool(is_bad[0]) == bool(bad.all()) == name.startswith('bad')
  if name.startswith('bad'):
    assert N[0].tolist() == [0, 0, 0, 0, WORDS] and brute.tolist() == [0, 0, 0, 0, WORDS]
  if name == 'one_hot':
    assert counts[0].tolist() == [0, 0, WORDS, 0, 0]
  if name == 'zero_last_weight':
    assert counts[0, 2] == 0 and counts[0, 4] == 0


def test_counts_are_not_the_rounded_weights():
  """The sampler's f32 product decides, not w / sum(w): the two differ by a few words."""
  w = np.array([ROWS['random']], F)
  counts = visit_ref.counts_of(visit_ref.cumulative_counts(w)[0])[0]
  ideal = w[0].astype(np.float64) / w[0].astype(np.float64).sum() * WORDS
  assert np.abs(counts - ideal).max() < 8
  assert int(counts.sum()) == WORDS


# ---------------------------------------------------------------- the split

def test_split_is_exact_non_negative_and_conserves_mass():
  rng = np.random.RandomState(5)
  special = [0, 1, 2, WORDS - 1, WORDS, WORDS + 1, UNIT - 1, UNIT, UNIT + 1, (1 << 62) - 1]
  masses = special + [int(x) for x in rng.randint(0, 1 << 62, size=200, dtype=np.int64)] + \
      [int(x) for x in rng.randint(0, 1 << 40, size=200, dtype=np.int64)]
  rows = np.array([ROWS[k] for k in sorted(ROWS)] + list(_policy(9, 1)), F)
  N, _ = visit_ref.cumulative_counts(rows)
  for i, m in enumerate(masses):
    n = N[i % len(N)]
    x = visit_ref.split(np.array([m], np.int64), n[None, :])[0]
    assert x.dtype == np.int64 and (x >= 0).all(), (m, x)
    assert int(x.sum()) == m, (m, x)
    y = [(m * int(k)) >> 24 for k in n]                    # Python integers do not overflow
    assert [int(v) for v in np.cumsum(x)] == y, (m, n)
    assert y[4] == m


# ---------------------------------------------------------------- frames

def test_mass_is_conserved_to_the_unit():
  g = _table()
  w = _policy(8, 2)
  out = visit_ref.visitation(g.st_next, g.st_done, w, 20, restart=True)
  assert out['per_frame'].shape == (21, 8) and (out['per_frame'] >= 0).all()
  assert (out['per_frame'].sum(axis=1) == UNIT).all()
  assert out['finished'].sum() > 0                                 # (episodes do end on this table)
  assert (out['visits'].sum() == 20 * UNIT) and np.array_equal(out['final'], out['per_frame'][-1])
  # every frame's visits are the frame's mass
  assert np.array_equal(out['visits'].sum(axis=1), out['per_frame'][:-1].sum(axis=0))
  gone = visit_ref.visitation(g.st_next, g.st_done, w, 20, restart=False)
  left = UNIT - gone['per_frame'].sum(axis=1)
  assert np.array_equal(left[1:], np.cumsum(gone['finished'])) and left[0] == 0
  assert 0 < gone['final'].sum() < UNIT
  assert np.array_equal(gone['counts'], out['counts'])


def test_n_frames_then_m_more_equal_n_plus_m():
  g = _table()
  w = _policy(8, 4)
  for restart in (True, False):
    whole = visit_ref.visitation(g.st_next, g.st_done, w, 12, restart=restart)
    first = visit_ref.visitation(g.st_next, g.st_done, w, 5, restart=restart)
    rest = visit_ref.visitation(g.st_next, g.st_done, w, 7, start=first['final'], restart=restart)
    assert np.array_equal(rest['final'], whole['final'])
    assert np.array_equal(first['visits'] + rest['visits'], whole['visits'])
    assert np.array_equal(np.concatenate([first['finished'], rest['finished']]), whole['finished'])
    assert np.array_equal(np.concatenate([first['per_frame'], rest['per_frame'][1:]]), whole['per_frame'])


def test_bad_rows_send_all_their_mass_to_action_4():
  g = _table()
  w = _policy(8, 6)
  w[0] = ROWS['bad_negative']
  w[3] = ROWS['bad_infinite_total']
  out = visit_ref.visitation(g.st_next, g.st_done, w, 6)
  assert out['bad_rows'] == 2
  assert not out['visits'][[0, 3], :4].any() and out['visits'][0, 4] >= UNIT
  assert out['counts'][0].tolist() == [0, 0, 0, 0, WORDS]


def test_a_float_start_is_quantised_to_exactly_one_environment():
  p = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
  d = visit_ref.quantise(p)
  assert d.dtype == np.int64 and int(d.sum()) == UNIT and (d >= 0).all()
  floor = np.floor(p * float(UNIT)).astype(np.int64)
  assert np.array_equal(np.delete(d, 2), np.delete(floor, 2)) and 0 <= d[2] - floor[2] < 5
  assert visit_ref.quantise(np.array([0, 1.0, 0])).tolist() == [0, UNIT, 0]


def test_the_sampler_s_counts_lie_within_six_deviations_of_the_expectation():
  B, T = 65536, 20
  g = _table()
  w = _policy(8, 7)
  walk = policy_ref.PolicyWalker(g, B).rollout(w, T, seed=11, reset_first=True)
  seen = np.zeros((8, 5), np.int64)
  np.add.at(seen, (walk['states'].astype(np.int64), walk['actions'].astype(np.int64)), 1)
  out = visit_ref.visitation(g.st_next, g.st_done, w, T, restart=True)
  E = B * out['visits'].astype(np.float64) / UNIT
  assert abs(E.sum() - B * T) < 1e-6 and seen.sum() == B * T
  # a cell's count is a sum over B independent environments of a per-environment count in 0 .. T,
  # whose variance is at most T times its mean: sigma^2 <= T * E
  dev = np.abs(seen - E)
  hit = E > 0
  worst = float((dev[hit] / np.sqrt(T * E[hit])).max())
  print('largest deviation / sqrt(T * E): %.3f' % worst)
  assert (dev[hit] <= 6.0 * np.sqrt(T * E[hit])).all(), worst
  assert not seen[~hit].any()
  assert hit.sum() >= 20 and (~hit).any()              # (the zero weights are cells of E = 0)


def test_visits_times_reward_is_the_value_planning_computes():
  """Duality: with restart=False, sum(visits * r) / 2^38 over T frames IS v_T[0], the expected
  undiscounted reward of T frames from the reset state."""
  T, S = 20, 8
  g = _table()
  assert not g.st_dcode.any()                                     # a plain table
  w = _policy(S, 8)
  out = visit_ref.visitation(g.st_next, g.st_done, w, T, restart=False)
  r = np.where(np.isnan(g.st_reward), 0.0, g.st_reward.astype(np.float64))
  got = float((out['visits'].astype(np.float64) * r).sum() / UNIT)
  # float64 dense evaluation under the exact probabilities
  p = out['counts'].astype(np.float64) / WORDS
  alive = (g.st_done == 0).astype(np.float64)
  v = np.zeros(S)
  for _ in range(T):
    v = (p * (r + alive * v[g.st_next.astype(np.int64)])).sum(axis=1)
  # Each of the T * S * 5 shares x_a is within one unit (2^-38) of m * p_a - two floors of the
  # same kind are subtracted - and a unit of mass is paid max|r| where it lands; that is the
  # allowance.  (float64 itself: about T * 2^-52 * T * max|r|, six orders below it.)
  bound = T * S * 5 * 2.0 ** -38 * float(np.abs(r).max())
  print('duality: visits %.9f dense %.9f difference %.3e bound %.3e' % (got, v[0], abs(got - v[0]), bound))
  assert np.abs(r).max() > 0 and abs(got - v[0]) <= bound
  # and the float32 planner, given the counts as weights (2^24 and below: exact in float32):
  # a sweep is 5 products, 4 sums, one division and per entry one sum, each within 2^-24 of a
  # value that is at most T * max|r|; the errors of T sweeps add up (an average does not grow them)
  planned = plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, 1.0, T,
                            policy=out['counts'].astype(F))
  assert planned['bad_rows'] == 0
  f32_bound = T * 11 * 2.0 ** -24 * T * float(np.abs(r).max())
  print('planner: %.6f difference %.3e bound %.3e' % (planned['values'][0], abs(planned['values'][0] - v[0]),
                                                      f32_bound))
  assert abs(float(planned['values'][0]) - v[0]) <= f32_bound


# ---------------------------------------------------------------- the plan's arithmetic

LDS_MAX = 144 * 1024
HEADER = 64
PER_LANE = 3


def _plan(S, lds_max=LDS_MAX, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_visit_plan(S, lds_max, path, out)
  return code, list(out)


def _lds_bytes(S):
  """The header's account of path 1: a header, the entries' words, N and two mass vectors, each
  part rounded up to 16 bytes."""
  up = lambda x: (x + 15) // 16 * 16
  return HEADER + up(20 * S) + up(16 * S) + 2 * up(8 * S)


def _largest():
  S = 1
  while _lds_bytes(S + 1) <= LDS_MAX:
    S += 1
  return S


def test_exports_and_op_name():
  from campx_amd import _hip
  assert 'campx_wide_visit_plan' in _hip.EXPORTS and 'campx_wide_visit_launch' in _hip.EXPORTS
  assert 'wide_visit' in _hip.OP_NAMES
  assert _hip.config_get('wide_lds_max') == LDS_MAX


def test_the_largest_table_that_fits_and_the_next():
  S = _largest()
  assert S == 2834                                   # 52 bytes per state, less the roundings
  assert _plan(S) == (0, [1, _lds_bytes(S), 1024, 1])
  assert _plan(S + 1) == (0, [2, 0, 256, (S + 1 + 255) // 256])
  assert _plan(S, path=2) == (0, [2, 0, 256, (S + 255) // 256])
  assert _plan(S, path=1)[1][0] == 1
  assert _plan(S + 1, path=1)[0] != 0
  # with LDS to spare the registers bound it: a lane owns three states at most
  roomy = 1 << 20
  assert _plan(1024 * PER_LANE, lds_max=roomy)[1][0] == 1
  assert _plan(1024 * PER_LANE + 1, lds_max=roomy)[1][0] == 2
  assert _plan(1024 * PER_LANE + 1, lds_max=roomy, path=1)[0] != 0


def test_threads_cover_small_tables_in_whole_waves():
  for S, threads in ((1, 64), (8, 64), (64, 64), (65, 128), (1000, 1024), (1024, 1024), (1025, 1024)):
    code, p = _plan(S)
    assert code == 0 and p == [1, _lds_bytes(S), threads, 1], S
    assert p[1] % 16 == 0


def test_wide_lds_max_zero_forces_global_and_path_1_is_refused_then():
  assert _plan(8, lds_max=0) == (0, [2, 0, 256, 1])
  assert _plan(8, lds_max=0, path=1)[0] != 0
  assert _plan(8, lds_max=_lds_bytes(8))[1][0] == 1
  assert _plan(8, lds_max=_lds_bytes(8) - 1)[1][0] == 2


def test_plan_refuses_bad_arguments():
  from campx_amd import _hip
  for S in (0, -1, (1 << 24) + 1):
    assert _plan(S)[0] != 0, S
  assert _plan(8, lds_max=-1)[0] != 0
  assert _plan(8, path=3)[0] != 0 and _plan(8, path=-1)[0] != 0
  assert _hip.lib.campx_wide_visit_plan(8, LDS_MAX, 0, None) != 0
  assert _plan(1 << 24) == (0, [2, 0, 256, (1 << 24) // 256])


# ---------------------------------------------------------------- the launch's validator

def _spec(S=8):
  from campx_amd import tabulate
  spec, arrays = tabulate.to_wide_spec(_table(S))
  return spec, arrays


def test_launch_validates_before_it_touches_a_device():
  """Every refusal below is decided by host arithmetic: no HIP call is made (none of the addresses
  is memory at all)."""
  from campx_amd import _hip
  spec, keep = _spec()
  S = int(spec.n_states)
  f = _hip.lib.campx_wide_visit_launch
  vp = ctypes.c_void_p
  A = 0x10000                                     # fake addresses, 64 KiB apart, 16-byte aligned
  good = dict(spec=ctypes.byref(spec), tables=vp(A), policy=vp(2 * A), start=vp(3 * A), restart=1,
              frames=7, visits=vp(4 * A), finished=vp(5 * A), final=vp(6 * A), per_frame=vp(7 * A),
              counts=vp(8 * A), scratch=vp(9 * A), bad_rows=vp(10 * A), bad_flag=vp(11 * A), path=2,
              stream=None)
  order = ('spec', 'tables', 'policy', 'start', 'restart', 'frames', 'visits', 'finished', 'final',
           'per_frame', 'counts', 'scratch', 'bad_rows', 'bad_flag', 'path', 'stream')

  def call(**change):
    args = dict(good, **change)
    return f(*[args[k] for k in order])

  refused = []
  # NULL where it is not allowed
  for name in ('spec', 'tables', 'policy', 'visits', 'finished', 'final', 'counts'):
    refused.append(({name: None}, call(**{name: None})))
  refused.append(({'scratch': None, 'path': 2}, call(scratch=None, path=2)))
  # misaligned pointers: 8 bytes for the int64 arrays and the tables, 4 for the others
  for name, base in (('tables', A), ('start', 3 * A), ('visits', 4 * A), ('finished', 5 * A),
                     ('final', 6 * A), ('per_frame', 7 * A), ('scratch', 9 * A)):
    refused.append(({name: '+4'}, call(**{name: vp(base + 4)})))
  for name, base in (('policy', 2 * A), ('counts', 8 * A), ('bad_rows', 10 * A), ('bad_flag', 11 * A)):
    refused.append(({name: '+2'}, call(**{name: vp(base + 2)})))
  # frames, restart, path
  for frames in (0, -1, (1 << 20) + 1):
    refused.append(({'frames': frames}, call(frames=frames)))
  for restart in (2, -1):
    refused.append(({'restart': restart}, call(restart=restart)))
  for path in (3, -1):
    refused.append(({'path': path}, call(path=path)))
  # final overlapping start without being equal to it; scratch overlapping either
  refused.append(('final = start + 8', call(final=vp(3 * A + 8))))
  refused.append(('final = start - 8 * (S - 1)', call(final=vp(3 * A - 8 * (S - 1)))))
  refused.append(('scratch = final', call(scratch=vp(6 * A))))
  refused.append(('scratch = final + 8', call(scratch=vp(6 * A + 8))))
  refused.append(('scratch = start', call(scratch=vp(3 * A))))
  refused.append(('scratch = start = final', call(scratch=vp(3 * A), final=vp(3 * A))))
  # path 1 for a table that does not fit (the plain fields are all a launch reads of a spec)
  spec.n_states = 2835
  refused.append(('path 1, 2 835 states', call(path=1)))
  spec.n_states = S
  einval = _hip.lib.campx_wide_visit_plan(0, 0, 0, None)
  assert einval != 0
  for what, code in refused:
    assert code == einval, (what, code)
  # a spec that is not one
  broken = type(spec).from_buffer_copy(bytes(ctypes.sizeof(spec)))
  assert call(spec=ctypes.byref(broken)) != 0
  del keep
