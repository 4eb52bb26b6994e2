"""`WideGame.visit_population()` on the GPU (csrc/k_visit.hip, `campx::wide_visit_population`)
against tests/visitation_population_reference.py - a numpy restatement of the population rule in
include/campx_hip.h - bit for bit: every comparison is `array_equal` of 'visits', 'finished',
'final', 'per_frame' and 'counts'; and member by member against `state_visitation()` on the same
game.

Tables: the boat race's own (8 states) and synthetic ones of 1, 37, 257 and 1 025 states (two
states a lane), of the plan's largest table in LDS and of the next.  The populations are chosen so
that the LDS path packs G = 1, 2 and 32 members of 8 states and 6 of 37 into a workgroup, each of
the packed ones with a short last workgroup; every case ASSERTS the G the plan gives, read back
from the plan call with the device's own number of compute units.  A population of ONE runs the
kernels compiled without members - `state_visitation()`'s - through this call's entry point: at
every one of the sizes it is held, path by path, against the reference and against
`state_visitation()` on the same path.  The reference does not depend
on the path: it is computed once per (table, P, frames, restart, start) and every path is held
against it.
"""

import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import visitation_population_reference as pop_ref
from test_visitation import big_table

pytestmark = pytest.mark.gpu

LDS_MAX = 144 * 1024
UNIT = 1 << 38
FRAMES = (1, 2, 7)                   # odd and even: either buffer of path 2 is read first
KINDS = ('none', 'shared', 'shared float', 'member')
KEYS = ('visits', 'finished', 'final', 'per_frame', 'counts')
NO_ROWS = KEYS[:3] + KEYS[4:]


def _cus():
  return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _plan(S, P, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_visit_population_plan(S, P, LDS_MAX, _cus(), path, out)
  return code, list(out)


@functools.lru_cache(maxsize=None)
def _largest():
  lo, hi = 1, 1 << 14
  while lo < hi:                               # the largest S the plan puts in LDS
    mid = (lo + hi + 1) // 2
    lo, hi = (mid, hi) if _plan(mid, 1)[1][0] == 1 else (lo, mid - 1)
  return lo


def _states(name):
  return {'fits': _largest(), 'next': _largest() + 1}.get(name) or int(name)


@functools.lru_cache(maxsize=None)
def _game(name):
  """-> (the tier's game, next_state, done); 'boat': the boat race's own table."""
  if name == 'boat':
    from campx_amd.games import boat_race
    game = boat_race.build(batch=8, device='cuda')
    game.use_state_table()
    game.its_showtime()
    traced = game.fused.traced
    assert game.fused.n_states == 8
    return game.fused, traced.st_next, traced.st_done
  from campx_amd import wide
  g = big_table(_states(name), 0.25, 9000 + _states(name))
  f = wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), 1, 'cuda', g)
  assert f.n_states == g.n_states
  return f, g.st_next, g.st_done


def _weights(P, S, seed, bad=()):
  rng = np.random.RandomState(seed)
  w = rng.uniform(0.25, 2.0, size=(P, S, 5)).astype(np.float32)
  w[rng.rand(P, S, 5) < 0.2] = 0
  w[:, np.arange(S), rng.randint(0, 5, size=S)] = 1.25              # (no row is all zero)
  for k, (m, s) in enumerate(bad):
    w[m, s, k % 5] = (-1.0, np.nan, np.inf)[k % 3]
  return w


def _start(P, S, kind, seed):
  """The `start` argument as numpy, or None.  'member': int64 per member, some members' total 0."""
  if kind == 'none':
    return None
  rng = np.random.RandomState(seed)
  shape = (S,) if kind.startswith('shared') else (P, S)
  p = rng.rand(*shape) * (rng.rand(*shape) < 0.6)
  p[..., rng.randint(S)] += 1.0
  p /= p.sum(axis=-1, keepdims=True)
  if kind.endswith('float'):
    return p.astype(np.float32)
  d = np.floor(p * (UNIT // 2)).astype(np.int64)                    # int64: half an environment
  if kind == 'member':
    d[sorted({0, P // 2, P - 1})[:P - 1]] = 0                       # (never every member)
  return d


def _paths(S):
  return ([1] if _plan(S, 1, path=1)[0] == 0 else []) + [2, 0]


def _eq(res, want, what, keys=KEYS):
  for k in keys:
    got = res[k].cpu().numpy()
    assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.dtype, got.shape)
    assert np.array_equal(got, want[k]), (what, k, int((got != want[k]).sum()))


def _members_to_check(P, G):
  """The first and last member of the first workgroup and of the last, and one in between."""
  last_group = (P - 1) // G * G
  return sorted({0, min(G, P) - 1, P // 2, last_group, P - 1, min(1, P - 1), max(P - 2, 0)})


def _cases():
  """(table, P, the G the LDS path must plan - None where a member does not fit).  8 200 members
  of 8 states on 256 compute units are 32 to a workgroup with 8 left over; on another chip the
  same shape is derived from its own count."""
  cus = _cus()
  return [('boat', 1, 1), ('boat', min(cus, 5), 1), ('boat', cus + 1, 2), ('boat', 32 * cus + 8, 32),
          ('1', 3, 1), ('1', 3 * cus + 2, 4), ('37', 5 * cus + 1, 6), ('257', 5, 1), ('1025', 5, 1), ('fits', 5, 1),
          ('next', 5, None),
          ('37', 1, 1), ('257', 1, 1), ('1025', 1, 1), ('fits', 1, 1), ('next', 1, None)]


CASE_IDS = ['boat-1', 'boat-few', 'boat-G2', 'boat-G32', 'one-state', 'one-state-G4', '37-G6', '257', '1025', 'fits', 'next',
            '37-solo', '257-solo', '1025-solo', 'fits-solo', 'next-solo']
SOLO_KEYS = KEYS + ('probs',)


@pytest.mark.parametrize('case', range(len(CASE_IDS)), ids=CASE_IDS)
def test_every_path_equals_the_reference_and_every_member_the_single_call(case):
  name, P, G = _cases()[case]
  f, nxt, done = _game(name)
  S = f.n_states
  code, plan = _plan(S, P)
  assert code == 0
  if G is None:
    assert plan[0] == 2 and _paths(S) == [2, 0]
  else:
    assert plan[0] == 1 and plan[4] == G and _paths(S) == [1, 2, 0], plan
    assert plan[3] == (P + G - 1) // G
    if G > 1:
      assert P % G != 0 and G * S <= 256                           # a short last workgroup
    if name == '37':
      assert G * S % 64 != 0 and S < 64                            # members share a wave, the last wave is part idle
    if name == '1025':
      assert plan[2] == 1024                                       # two states a lane
    if name == 'fits':
      assert S == 2834 and plan[2] == 1024                         # three states a lane
  w = _weights(P, S, 100 + case)
  policies = torch.from_numpy(w).cuda()
  members = _members_to_check(P, G or 1)
  assert len(members) >= min(P, 5)
  cumulative = pop_ref.cumulative_counts(w.reshape(P * S, 5))      # the bisection, once per case
  for frames in FRAMES:
    for restart in (True, False):
      for kind in KINDS:
        given = _start(P, S, kind, 7 * frames + case)
        want = pop_ref.visitation(nxt, done, w, frames, start=given, restart=restart, cumulative=cumulative)
        assert want['bad_rows'] == 0
        arg = None if given is None else torch.from_numpy(given).cuda()
        what = (name, P, frames, restart, kind)
        for path in _paths(S):
          res = f.visit_population(policies, frames, start=arg, restart=restart, want_frames=True, path=path)
          _eq(res, want, what + (path,))
          assert res['unit'] == UNIT and res['probs'].dtype == torch.float64
          assert np.array_equal(res['probs'].cpu().numpy(), want['counts'] / float(1 << 24))
          if path == 2:                          # and without per_frame: other buffers, same bits
            bare = f.visit_population(policies, frames, start=arg, restart=restart, path=path)
            assert 'per_frame' not in bare
            _eq(bare, want, what + (path, 'no per_frame'), NO_ROWS)
          if P == 1:                             # the same instances from the other entry point, path by path
            own = None if arg is None else arg.reshape(-1)[:S].reshape(S)
            one = f.state_visitation(policies[0], frames, start=own, restart=restart, want_frames=True, path=path)
            for k in SOLO_KEYS:
              got = res[k][:, 0] if k in ('finished', 'per_frame') else res[k][0]
              assert got.dtype == one[k].dtype and torch.equal(got, one[k]), what + (path, k)
        if restart:                              # the invariant: the total stays put
          assert np.array_equal(want['final'].sum(axis=1), want['per_frame'][0].sum(axis=1))
          assert torch.equal(res['final'].sum(1), res['per_frame'][0].sum(1))
        for m in members:                        # (res: what path 0 gave)
          own = None if arg is None else (arg if arg.dim() == 1 else arg[m])
          one = f.state_visitation(policies[m], frames, start=own, restart=restart, want_frames=True)
          assert torch.equal(res['visits'][m], one['visits']), what + (m,)
          assert torch.equal(res['finished'][:, m], one['finished']), what + (m,)
          assert torch.equal(res['final'][m], one['final']), what + (m,)
          assert torch.equal(res['per_frame'][:, m], one['per_frame']), what + (m,)
          assert torch.equal(res['counts'][m], one['counts']) and torch.equal(res['probs'][m], one['probs'])
  f.check_actions()


def test_through_the_engine_and_into_reused_buffers():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.use_state_table()
  game.its_showtime()
  traced = game.fused.traced
  w = _weights(3, 8, 22)
  policies = torch.from_numpy(w).cuda()
  want = pop_ref.visitation(traced.st_next, traced.st_done, w, 7)
  _eq(game.visit_population(policies, 7, want_frames=True), want, 'engine')
  out = game.visit_population_buffers(3, 7, want_frames=True)
  assert sorted(out) == ['counts', 'final', 'finished', 'per_frame', 'probs', 'scratch', 'visits']
  for t in out.values():
    t.fill_(-7)
  res = game.visit_population(policies, 7, want_frames=True, out=out)
  assert all(res[k] is out[k] for k in KEYS + ('probs',))
  _eq(out, want, 'engine out=')
  assert 'per_frame' not in game.visit_population_buffers(3, 7)


@pytest.mark.parametrize('name,P', [('boat', 70), ('37', 13), ('next', 4), ('boat', 1), ('1025', 1), ('next', 1)])
def test_continuation_in_place_with_reused_buffers(name, P):
  f, nxt, done = _game(name)
  S = f.n_states
  w = _weights(P, S, 41)
  policies = torch.from_numpy(w).cuda()
  given = _start(P, S, 'member', 43)
  for restart in (True, False):
    for n, m in ((5, 7), (4, 2)):                # odd and even: either buffer of path 2 is read first
      whole = pop_ref.visitation(nxt, done, w, n + m, start=given, restart=restart)
      for path in _paths(S)[:2]:
        first = f.visit_population_buffers(P, n, want_frames=True)
        for t in first.values():
          t.fill_(-7)
        a = f.visit_population(policies, n, start=torch.from_numpy(given).cuda(), restart=restart,
                               want_frames=True, out=first, path=path)
        assert a['final'] is first['final']
        _eq(a, pop_ref.visitation(nxt, done, w, n, start=given, restart=restart), (name, path, 'first'))
        # m more frames from 'final' IN PLACE, every other buffer of another size
        rest = dict(f.visit_population_buffers(P, m, want_frames=True), final=first['final'])
        b = f.visit_population(policies, m, start=first['final'], restart=restart, want_frames=True,
                               out=rest, path=path)
        assert b['final'] is first['final']
        what = (name, path, restart, n, m)
        assert np.array_equal(b['final'].cpu().numpy(), whole['final']), what
        assert np.array_equal((a['visits'] + b['visits']).cpu().numpy(), whole['visits']), what
        assert np.array_equal(torch.cat([a['finished'], b['finished']]).cpu().numpy(), whole['finished']), what
        assert np.array_equal(b['per_frame'].cpu().numpy(), whole['per_frame'][n:]), what
        # and from a copy of it: the start given is left as it is
        keep = torch.from_numpy(whole['per_frame'][n]).cuda()
        c = f.visit_population(policies, m, start=keep, restart=restart, path=path)
        assert np.array_equal(keep.cpu().numpy(), whole['per_frame'][n])
        assert torch.equal(c['final'], b['final']) and torch.equal(c['visits'], b['visits'])
  f.check_actions()


@pytest.mark.parametrize('name,P', [('boat', 70), ('next', 4)])
def test_bad_rows_give_the_reference_s_bits_and_raise_lazily_with_their_count(name, P):
  f, nxt, done = _game(name)
  S = f.n_states
  bad = [(0, 0), (P - 1, S - 1), (P // 2, 0), (P // 2, S // 2), (1, S - 1)]      # in some members, state 0's row too
  w = _weights(P, S, 51, bad)
  want = pop_ref.visitation(nxt, done, w, 7)
  assert want['bad_rows'] == len(set(bad)) == 5
  policies = torch.from_numpy(w).cuda()
  message = '^5 rows of the policies given to visit_population\\(\\) are bad'
  for path in _paths(S)[:2]:
    out = f.visit_population_buffers(P, 7, want_frames=True)
    # the call does not wait for the count: it raises only if the flag is already up when it looks
    try:
      f.visit_population(policies, 7, want_frames=True, out=out, path=path)
      torch.cuda.synchronize()
      assert int(f._bad_visit_rows) == 0 and int(f._bad_visit_member_rows) == 5   # state_visitation()'s own stays 0
      with pytest.raises(ValueError, match=message) as caught:
        f.check_actions()
      text = str(caught.value)
    except ValueError as e:
      text = str(e)
    assert text.startswith('5 rows of the policies given to visit_population() are bad')
    assert 'state_visitation' not in text and text.count('rows of') == 1
    _eq(out, want, (name, path, 'bad rows'))
    f.check_actions()
    f.validate_actions = 'sync'
    try:
      with pytest.raises(ValueError, match=message):
        f.visit_population(policies, 7, path=path)
    finally:
      f.validate_actions = True
    f.check_actions()
  # the single call counts into its own counter and says so
  with pytest.raises(ValueError, match='rows of the policy given to state_visitation'):
    f.state_visitation(policies[0], 3)
    f.check_actions()
  f.check_actions()


@pytest.mark.parametrize('name', ['boat', 'next'])
def test_bad_rows_of_one_member_land_on_the_counter_of_the_function_called(name):
  """P = 1 runs one set of kernels from both entry points; whose counter and message a bad row
  lands on is the caller's, both ways, each with the exact count."""
  f, nxt, done = _game(name)
  S = f.n_states
  bad = [(0, 0), (0, S - 1), (0, S // 2)]
  w = _weights(1, S, 57, bad)
  want = pop_ref.visitation(nxt, done, w, 5)
  assert want['bad_rows'] == 3
  policies = torch.from_numpy(w).cuda()
  f.check_actions()
  f.validate_actions = 'sync'                    # the call itself raises, with the count
  try:
    for path in _paths(S)[:2]:
      res = f.visit_population_buffers(1, 5, want_frames=True)
      with pytest.raises(ValueError) as caught:
        f.visit_population(policies, 5, want_frames=True, out=res, path=path)
      text = str(caught.value)
      assert text.startswith('3 rows of the policies given to visit_population() are bad')
      assert 'state_visitation' not in text and text.count('rows of') == 1
      assert int(f._bad_visit_rows) == 0 and int(f._bad_visit_member_rows) == 0
      _eq(res, want, (name, path, 'bad rows of one member'))
      f.check_actions()                          # nothing is left counted
      one = f.visitation_buffers(5, want_frames=True)
      with pytest.raises(ValueError) as caught:
        f.state_visitation(policies[0], 5, want_frames=True, out=one, path=path)
      text = str(caught.value)
      assert text.startswith('3 rows of the policy given to state_visitation() are bad')
      assert 'visit_population' not in text and text.count('rows of') == 1
      assert int(f._bad_visit_rows) == 0 and int(f._bad_visit_member_rows) == 0
      assert torch.equal(one['visits'], res['visits'][0]) and torch.equal(one['final'], res['final'][0])
      f.check_actions()
    # not validated: neither counter moves
    f.validate_actions = False
    f.visit_population(policies, 5)
    f.state_visitation(policies[0], 5)
    torch.cuda.synchronize()
    assert int(f._bad_visit_rows) == 0 and int(f._bad_visit_member_rows) == 0
  finally:
    f.validate_actions = True
  f.check_actions()


def test_a_shared_start_that_is_final_is_refused_for_one_member_too():
  """A [S] start is SHARED, whatever P is: at P = 1 it still must not be 'final' - only a
  [1, S] start continues in place - and the refusal comes before any launch, from the method and
  from the C entry."""
  from campx_amd import _hip
  f, nxt, done = _game('37')
  S = f.n_states
  w = _weights(1, S, 81)
  policies = torch.from_numpy(w).cuda()
  given = _start(1, S, 'member', 82)
  out = f.visit_population_buffers(1, 3)
  launched = []
  real = _hip.ops.wide_visit_population
  try:
    _hip.ops.wide_visit_population = lambda *a: launched.append(a) or real(*a)
    for path in (1, 2, 0):
      out['final'].copy_(torch.from_numpy(given))
      with pytest.raises(ValueError, match='start must not overlap out'):
        f.visit_population(policies, 3, start=out['final'][0], out=out, path=path)
      assert not launched
  finally:
    del _hip.ops.wide_visit_population
  spec = (ctypes.c_char * f._spec_host.numel()).from_buffer(f._spec_host.numpy())
  vp = ctypes.c_void_p
  launch = _hip.lib.campx_wide_visit_population_launch
  for t in out.values():
    t.fill_(-3)
  for path in (1, 2, 0):
    for per_member, refused in ((0, True), (1, False)):
      out['final'].copy_(torch.from_numpy(given))
      code = launch(ctypes.cast(spec, launch.argtypes[0]), vp(f._tables.data_ptr()), vp(policies.data_ptr()), 1,
                    vp(out['final'].data_ptr()), per_member, 1, 3, vp(out['visits'].data_ptr()),
                    vp(out['finished'].data_ptr()), vp(out['final'].data_ptr()), None,
                    vp(out['counts'].data_ptr()), vp(out['scratch'].data_ptr()), None, None, path,
                    vp(torch.cuda.current_stream().cuda_stream))
      torch.cuda.synchronize()
      if refused:
        assert code != 0
        assert bool((out['visits'] == -3).all()) and bool((out['counts'] == -3).all())   # nothing ran
        assert np.array_equal(out['final'].cpu().numpy(), given)
      else:                                      # the same pointers as a start per member: in place
        assert code == 0
        _eq(out, pop_ref.visitation(nxt, done, w, 3, start=given), ('in place', path), NO_ROWS)
        out['visits'].fill_(-3)
        out['counts'].fill_(-3)


def test_path_1_on_a_table_that_does_not_fit_raises():
  f, _, _ = _game('next')
  policies = torch.from_numpy(_weights(2, f.n_states, 1)).cuda()
  with pytest.raises(ValueError, match='path=1'):
    f.visit_population(policies, 3, path=1)
  f.visit_population(policies, 3, path=2)
  f.check_actions()


def test_a_game_that_is_not_on_the_tier_refuses_by_name():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.its_showtime()
  with pytest.raises(NotImplementedError, match=r'^visit_population\(\) is .*state-table tier only'):
    game.visit_population(torch.ones(2, 8, 5, device='cuda'), 3)
  with pytest.raises(NotImplementedError, match=r'^visit_population_buffers\(\) is .*state-table tier only'):
    game.visit_population_buffers(2, 3)
  with pytest.raises(RuntimeError, match='its_showtime'):
    boat_race.build(batch=8, device='cuda').visit_population(torch.ones(2, 8, 5, device='cuda'), 3)


def test_argument_errors_raise_before_any_launch():
  f, _, _ = _game('37')
  S, P = f.n_states, 4
  policies = torch.from_numpy(_weights(P, S, 61)).cuda()
  out = f.visit_population_buffers(P, 3, want_frames=True)
  for t in out.values():
    t.fill_(7)
  launched = []
  from campx_amd import _hip
  real = _hip.ops.wide_visit_population

  class Spy(object):
    def __call__(self, *a):
      launched.append(a)
      return real(*a)

  ones = torch.ones(P, S, device='cuda')
  units = ones.long()
  spare = torch.zeros(2 * P * S, dtype=torch.int64, device='cuda')
  visit = f.visit_population
  bad_calls = [
      lambda: visit(policies.double(), 3, out=out),
      lambda: visit(policies[:, :-1], 3, out=out),
      lambda: visit(policies[0], 3, out=out),
      lambda: visit(policies.cpu(), 3, out=out),
      lambda: visit(policies.transpose(0, 1).contiguous().transpose(0, 1), 3, out=out),   # not contiguous
      lambda: visit(policies, 0, out=out),
      lambda: visit(policies, 3.0, out=out),
      lambda: visit(policies, (1 << 20) + 1),
      lambda: visit(policies, 3, path=3, out=out),
      lambda: visit(policies, 3, start=units[:, :-1], out=out),
      lambda: visit(policies, 3, start=units[:-1], out=out),                              # [P - 1, S]
      lambda: visit(policies, 3, start=units.cpu(), out=out),
      lambda: visit(policies, 3, start=units.int(), out=out),
      lambda: visit(policies, 3, start=-units, out=out),
      lambda: visit(policies, 3, start=units.t().contiguous().t(), out=out),              # not contiguous
      lambda: visit(policies, 3, start=torch.cat([units[:-1], units[:1] * (UNIT // S + 1)]), out=out),   # one member's total
      lambda: visit(policies, 3, start=units[0] * (UNIT // S + 1), out=out),              # the shared total
      lambda: visit(policies, 3, start=ones, out=out),                                    # rows sum to S
      lambda: visit(policies, 3, start=ones[0] * float('nan'), out=out),
      lambda: visit(policies, 3, start=torch.cat([ones[:-1] / S, ones[:1]]), out=out),    # one row sums to S
      lambda: visit(policies, 3, start=out['scratch'], out=out, path=2),
      lambda: visit(policies, 3, start=out['scratch'][0], out=out, path=2),
      lambda: visit(policies, 3, start=out['final'][0], out=out),                         # a shared start in 'final'
      lambda: visit(policies, 3, start=spare[1:P * S + 1].view(P, S),                     # overlapping, not equal
                    out=dict(out, final=spare[:P * S].view(P, S))),
      lambda: visit(policies, 3, out={'visits': out['visits']}),
      lambda: visit(policies, 4, out=out),                                                # finished of 3
      lambda: visit(policies, 3, out=dict(out, counts=out['counts'].long())),
      lambda: visit(policies, 3, out=dict(out, finished=out['finished'].t())),            # [P, frames]
      lambda: visit(policies, 3, want_frames=True, out=f.visit_population_buffers(P, 3)),
      lambda: visit(policies[:3], 3, out=out),                                            # buffers of 4 members
      lambda: visit(policies, 3, out=[out]),
      lambda: f.visit_population_buffers(0, 3),
      lambda: f.visit_population_buffers(P, 0),
  ]
  try:
    _hip.ops.wide_visit_population = Spy()
    for k, call in enumerate(bad_calls):
      with pytest.raises(ValueError):
        call()
      assert not launched, k
  finally:
    del _hip.ops.wide_visit_population
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in out.values())                       # nothing was written
  visit(policies, 3, want_frames=True, out=out)                                # and the dict was fine
  f.check_actions()


def test_the_two_element_limits_raise_before_anything_is_allocated():
  f, _, _ = _game('37')
  S = f.n_states
  too_many = ((1 << 31) - 1) // (S * 5) + 1
  with pytest.raises(ValueError, match=r'visit_population\(\): P \* n_states \* 5 = {} x 37 x 5 must be at most '
                                       r'2\^31 - 1'.format(too_many)):
    f.visit_population_buffers(too_many, 3)
  with pytest.raises(ValueError, match=r'\(frames \+ 1\) \* P \* n_states = .* must be at most 2\^31 - 1 with '
                                       r'want_frames; split'):
    f.visit_population_buffers(100, 1 << 20, want_frames=True)
  policies = torch.from_numpy(_weights(100, S, 3)).cuda()
  with pytest.raises(ValueError, match='want_frames; split'):
    f.visit_population(policies, 1 << 20, want_frames=True)
  frames = ((1 << 31) - 1) // (100 * S) - 1                                    # the most that is allowed
  assert (frames + 1) * 100 * S <= (1 << 31) - 1 < (frames + 2) * 100 * S
  f._check_frame_elements(100, frames)
  with pytest.raises(ValueError, match='want_frames; split'):
    f._check_frame_elements(100, frames + 1)


def test_the_c_entry_through_ctypes_with_a_shared_start_and_no_per_frame():
  from campx_amd import _hip
  f, nxt, done = _game('37')
  S, P = f.n_states, 9
  w = _weights(P, S, 71)
  given = _start(P, S, 'shared', 72)
  want = pop_ref.visitation(nxt, done, w, 7, start=given, restart=False)
  policies = torch.from_numpy(w).cuda()
  start = torch.from_numpy(given).cuda()
  out = f.visit_population_buffers(P, 7)
  spec = (ctypes.c_char * f._spec_host.numel()).from_buffer(f._spec_host.numpy())
  vp = ctypes.c_void_p
  stream = torch.cuda.current_stream().cuda_stream
  launch = _hip.lib.campx_wide_visit_population_launch
  for path in (2, 0):
    for t in out.values():
      t.fill_(-3)
    code = launch(ctypes.cast(spec, launch.argtypes[0]), vp(f._tables.data_ptr()), vp(policies.data_ptr()), P,
                  vp(start.data_ptr()), 0, 0, 7, vp(out['visits'].data_ptr()), vp(out['finished'].data_ptr()),
                  vp(out['final'].data_ptr()), None, vp(out['counts'].data_ptr()),
                  vp(out['scratch'].data_ptr()), None, None, path, vp(stream))
    assert code == 0
    torch.cuda.synchronize()
    _eq(out, want, ('ctypes', path), NO_ROWS)
    assert np.array_equal(start.cpu().numpy(), given)                          # the start is left as it is
    if path == 2:
      assert not out['scratch'].any()                                          # left all zero
