"""`WideGame.evaluate_population()` on the GPU (csrc/k_plan.hip, `campx::wide_population_sweeps`)
against tests/planning_reference.py run member by member, bit for bit: every comparison is
`array_equal` on the int32 views of the float arrays, with no tolerance.

Tables come from `wide_table_reference.make_table()` through the production constructor, as in
tests/test_planning.py.  Sizes: one state; a wave that straddles members (S = 5, 37 with two or more
members to a workgroup); a member that straddles waves (257, and every S above 64); one state per
thread of the LDS workgroup and two (1 023, 1 025); the largest table whose ONE member fits LDS
and the next.  P = 1, 2, 3, 17, 64, 257: on a chip of 256 compute units the plan gives a workgroup
one member up to P = 256 and two at 257, whose last workgroup is then half full; the test of a
packed workgroup further down takes P = 2 051 for nine members to a workgroup.  The numpy loop over the members
dominates the run time, so the grid of (S, P, sweeps) is trimmed by hand: every S, every P, every
sweep count, the large P with the small S or the few sweeps.
"""

import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import planning_reference as plan_ref
import wide_table_reference as ref

pytestmark = pytest.mark.gpu

LDS_MAX = 144 * 1024
KINDS = ['random', 'zeros', 'onehot', 'bad']
GAMMAS = [1.0, 0.99, 0.5]


def _plan(S, P, path=0, lds_max=LDS_MAX, n_cus=256):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_population_sweeps_plan(S, P, 0, lds_max, n_cus, path, out)
  return code, list(out)


def _largest():
  lo, hi = 1, 1 << 14
  while lo < hi:                               # the largest S whose one member the plan puts in LDS
    mid = (lo + hi + 1) // 2
    lo, hi = (mid, hi) if _plan(mid, 1)[1][0] == 1 else (lo, mid - 1)
  return lo


LARGEST = _largest()

# (S, P, sweeps)
GRID = [(1, 257, 64), (1, 3, 7), (2, 64, 7), (2, 1, 1), (5, 17, 64), (5, 257, 2), (37, 3, 64),
        (37, 257, 7), (37, 17, 1), (255, 2, 7), (255, 64, 2), (256, 17, 2), (256, 1, 64),
        (257, 3, 64), (257, 257, 1), (1023, 64, 1), (1023, 2, 64), (1025, 17, 7), (1025, 3, 2),
        (LARGEST, 1, 7), (LARGEST, 17, 1), (LARGEST, 3, 2), (LARGEST + 1, 2, 64),
        (LARGEST + 1, 3, 7), (LARGEST + 1, 17, 1)]


def _fits(S):
  return _plan(S, 1, path=1)[0] == 0


def _paths(S):
  return ([1] if _fits(S) else []) + [2, 0]


@functools.lru_cache(maxsize=None)
def _table(S, dcodes=False, perf=False):
  return ref.make_table(7000 + S, 4, 4, 2, 1, S, dcodes=dcodes and S >= 4, perf=perf)


def _game(g, batch=1):
  from campx_amd import wide
  f = wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), batch, 'cuda', g)
  assert f.n_states == g.n_states
  return f


def _policy(S, kind, seed):
  """-> (weights float32 [S, 5], number of bad rows): tests/test_planning.py's kinds."""
  rng = np.random.RandomState(seed)
  w = rng.uniform(0.5, 2.0, size=(S, 5)).astype(np.float32)
  w.reshape(-1)[rng.randint(0, S * 5, size=max(1, S // 8))] = np.float32(2.0 ** -20)
  bad = 0
  if kind == 'zeros':
    w[rng.rand(S, 5) < 0.4] = 0
    w[np.arange(S), rng.randint(0, 5, size=S)] = 1.5        # (no row is all zero)
  elif kind == 'onehot':
    w[:] = 0
    w[np.arange(S), rng.randint(0, 5, size=S)] = 1
  elif kind == 'bad':
    rows = rng.choice(S, size=min(S, 3), replace=False)
    for i, row in enumerate(rows):
      if i == 0:
        w[row, rng.randint(5)] = -1.0
      elif i == 1:
        w[row, rng.randint(5)] = np.nan
      else:
        w[row] = 0
    bad = len(rows)
  return w, bad


def _population(S, P, seed, kinds=KINDS):
  """-> (weights [P, S, 5], bad rows in all): the kinds rotated, a seed per member."""
  made = [_policy(S, kinds[(seed + m) % len(kinds)], 1000 * seed + m) for m in range(P)]
  return np.stack([w for w, _ in made]), sum(b for _, b in made)


def _bits(x):
  x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
  return x.view(np.int32) if x.dtype == np.float32 else x


def _eq(got, want, what):
  got, want = _bits(got), _bits(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
  assert np.array_equal(got, want), (what, int((got != want).sum()))


def _reference(g, ws, gammas, n, values=None, members=None, **kw):
  """The reference, member by member -> values [P, S], q [P, S, 5], residual [n, P], bad rows."""
  members = range(len(ws)) if members is None else members
  gammas = np.broadcast_to(np.asarray(gammas, np.float32), (len(ws),))
  each = [plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, gammas[m], n, policy=ws[m],
                          values=None if values is None else values[m], **kw) for m in members]
  return dict(values=np.stack([e['values'] for e in each]), q=np.stack([e['q'] for e in each]),
              residual=np.stack([e['residual'] for e in each], axis=1),
              bad_rows=sum(e['bad_rows'] for e in each))


def _check(res, want, what, q=True):
  _eq(res['values'], want['values'], (what, 'values'))
  _eq(res['residual'], want['residual'], (what, 'residual'))
  if q:
    _eq(res['q'], want['q'], (what, 'q'))


def test_the_plan_is_the_one_the_sizes_were_chosen_for():
  from campx_amd import _hip
  assert LARGEST == 2045 and _hip.config_get('wide_lds_max') == LDS_MAX
  assert torch.cuda.get_device_properties(0).multi_processor_count == 256, 'the sizes below assume 256 compute units'
  # members to a workgroup at the grid's P: one up to P = 256, two at 257 - 129 workgroups, the last half full
  assert [_plan(5, P)[1][4] for P in (1, 2, 3, 17, 64, 257)] == [1, 1, 1, 1, 1, 2]
  assert _plan(5, 257)[1][3] == 129 and _plan(37, 257)[1][2] == 128 and _plan(257, 257)[1][2:] == [320, 257, 1]
  assert _plan(1025, 17)[1][2:] == [1024, 17, 1]              # two states to a thread
  assert _plan(5, 2051)[1][3:] == [228, 9] and 2051 % 9 == 8


@pytest.mark.parametrize('S,P,n', GRID, ids=lambda x: str(x))
def test_both_paths_equal_the_reference_member_by_member(S, P, n):
  i = GRID.index((S, P, n))
  dcodes = i % 2 == 1
  g = _table(S, dcodes=dcodes)
  f = _game(g)
  f.validate_actions = 'sync'
  ws, n_bad = _population(S, P, i)
  gamma = GAMMAS[i % 3]
  policies = torch.from_numpy(ws).cuda()
  want = _reference(g, ws, gamma, n)
  assert want['bad_rows'] == n_bad and (P < 4 or n_bad > 0)
  for path in _paths(S):
    out = f.population_sweep_buffers(P, n, want_q=True)
    for t in out.values():
      t.fill_(-7)
    if n_bad:
      with pytest.raises(ValueError, match='^{} rows of the policies given to evaluate_population'.format(n_bad)):
        f.evaluate_population(policies, gamma, n, want_q=True, out=out, path=path)
      res = out
    else:
      res = f.evaluate_population(policies, gamma, n, want_q=True, out=out, path=path)
      assert res['sweeps'] == n and res['values'] is out['values']
    _check(res, want, (S, P, n, gamma, dcodes, path))
  f.check_actions()                              # nothing is left counted


@pytest.mark.parametrize('S', [5, 37])
def test_a_packed_workgroup_nine_members_the_last_short(S):
  """P = 2 051 on 256 compute units: nine members to a workgroup, waves that hold parts of two or
  more members, a last workgroup of eight.  The global path - a workgroup per member, checked
  above - is the whole population's reference; numpy's a sample of members, the ends of
  workgroups among them."""
  P, n = 2051, 7
  g = _table(S, dcodes=True)
  f = _game(g)
  f.validate_actions = False
  ws, _ = _population(S, P, 3)
  gammas = np.linspace(0.3, 1.0, P).astype(np.float32)
  start = np.random.RandomState(S).uniform(-2, 2, size=(P, S)).astype(np.float32)
  args = (torch.from_numpy(ws).cuda(), torch.from_numpy(gammas).cuda(), n)
  a = f.evaluate_population(*args, values=torch.from_numpy(start).cuda(), want_q=True, path=1)
  b = f.evaluate_population(*args, values=torch.from_numpy(start).cuda(), want_q=True, path=2)
  for k in ('values', 'q', 'residual'):
    _eq(a[k], b[k], (S, k))
  sample = [0, 1, 8, 9, 10, 17, 18, 1000, 1025, 2042, 2043, 2049, 2050]
  want = _reference(g, ws, gammas, n, values=start, members=sample)
  _check({k: a[k][:, sample] if k == 'residual' else a[k][sample] for k in ('values', 'q', 'residual')},
         want, (S, 'sample'))


def test_more_workgroups_than_a_grid_holds():
  """Past 2^20 workgroups a workgroup takes several groups in turn: P = 2^20 + 3 members of one
  state - on the global path, and on the LDS path with wide_lds_max lowered to one member."""
  from campx_amd import _hip
  P, S, n = (1 << 20) + 3, 1, 2
  g = _table(S)
  f = _game(g)
  f.validate_actions = False
  rng = np.random.RandomState(5)
  ws = rng.uniform(0.5, 2.0, size=(P, S, 5)).astype(np.float32)
  gammas = rng.uniform(0.1, 1.0, size=P).astype(np.float32)
  args = (torch.from_numpy(ws).cuda(), torch.from_numpy(gammas).cuda(), n)
  packed = f.evaluate_population(*args, path=1)
  assert _plan(S, P)[1][3:] == [4097, 256]
  wide = f.evaluate_population(*args, path=2)
  one = _plan(S, 1)[1][1]
  assert _plan(S, P, lds_max=one)[1] == [1, one, 64, 1 << 20, 1]
  with _hip.config(wide_lds_max=one):
    single = f.evaluate_population(*args, path=1)
  for k in ('values', 'residual'):
    assert torch.equal(packed[k].view(torch.int32), wide[k].view(torch.int32)), k
    assert torch.equal(packed[k].view(torch.int32), single[k].view(torch.int32)), k
  sample = [0, 1, 1023, 1024, (1 << 20) - 1, 1 << 20, P - 1]
  want = _reference(g, ws, gammas, n, members=sample)
  _eq(packed['values'][sample], want['values'], 'values')
  _eq(packed['residual'][:, sample], want['residual'], 'residual')


ONE_MEMBER = ((37, 7), (257, 7), (1025, 2), (1025, 3))   # less than a wave; a second workgroup of one
                                                         # live lane on path 2; two states to a thread


def _one_member(S, seed=4):
  g = _table(S, dcodes=True)
  w, _ = _policy(S, 'zeros', seed)
  rng = np.random.RandomState(S)
  over = rng.uniform(-1, 1, size=(S, 5)).astype(np.float32)
  start = rng.uniform(-2, 2, size=S).astype(np.float32)
  return g, _game(g), w, over, start


def _eq_member(res, alone, what):
  n, S = alone['residual'].shape[0], alone['values'].shape[0]
  assert tuple(res['values'].shape) == (1, S) and tuple(res['residual'].shape) == (n, 1)
  _eq(res['values'][0], alone['values'], (what, 'values'))
  _eq(res['q'][0], alone['q'], (what, 'q'))
  _eq(res['residual'][:, 0], alone['residual'], (what, 'residual'))


def test_one_member_is_evaluate_policy():
  """P = 1 without a gamma of its own runs evaluate_policy()'s kernels: every path of either call
  against every path of the other and against the reference - from zeros with the table's rewards,
  from given values with a reward override, and with `values is out['values']` (an odd count: on
  path 2 the start is copied into the scratch array first)."""
  for S, n in ONE_MEMBER:
    g, f, w, over, start = _one_member(S)
    policy = torch.from_numpy(w).cuda()
    alone = f.evaluate_policy(policy, 0.99, n)
    for path in (1, 2):
      res = f.evaluate_population(policy[None], 0.99, n, want_q=True, path=path)
      _eq_member(res, alone, (S, path))
    kw = dict(reward=torch.from_numpy(over).cuda())
    values = torch.from_numpy(start).cuda()
    want = plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, np.float32(0.99), n, policy=w,
                           values=start, reward_override=over)
    for solo_path in (1, 2, 0):
      alone = f.evaluate_policy(policy, 0.99, n, values=values, path=solo_path, **kw)
      for k in ('values', 'q', 'residual'):
        _eq(alone[k], want[k], (S, solo_path, k, 'evaluate_policy() against the reference'))
      for path in (1, 2, 0):
        res = f.evaluate_population(policy[None], 0.99, n, values=values[None], want_q=True, path=path, **kw)
        _eq_member(res, alone, (S, solo_path, path, 'override, start'))
    _eq(values, start, 'the values given are left as they are')
    for path in (1, 2):
      out = f.population_sweep_buffers(1, n, want_q=True)
      out['values'].copy_(values[None])
      res = f.evaluate_population(policy[None], 0.99, n, values=out['values'], want_q=True, out=out, path=path, **kw)
      assert res['values'] is out['values']
      _eq_member(res, want, (S, path, 'values is out[values]'))
      solo = f.sweep_buffers(n, greedy=False)
      solo['values'].copy_(values)
      alone = f.evaluate_policy(policy, 0.99, n, values=solo['values'], out=solo, path=path, **kw)
      _eq_member(res, alone, (S, path, 'both aliased'))


def test_one_member_with_a_gamma_of_its_own():
  """P = 1 with `gamma` as a float32 [1] tensor: the same bits as evaluate_policy() with that number
  on both paths; the tensor is not read on the host, so a NaN in it is not refused and the result is
  the reference's (NaN in the same places - the payload of a generated NaN is defined by no rule -
  and the same bits everywhere else)."""
  import float_edges as fe
  for S, n in ONE_MEMBER:
    g, f, w, over, start = _one_member(S)
    policy = torch.from_numpy(w).cuda()
    values = torch.from_numpy(start).cuda()
    for gamma in (np.float32(0.99), np.float32(0.3)):
      gammas = torch.from_numpy(np.array([gamma])).cuda()
      alone = f.evaluate_policy(policy, float(gamma), n, values=values)
      for path in (1, 2):
        res = f.evaluate_population(policy[None], gammas, n, values=values[None], want_q=True, path=path)
        _eq_member(res, alone, (S, float(gamma), path))
    nan = torch.full((1,), float('nan'), device='cuda')
    want = plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, np.float32(np.nan), n, policy=w,
                           values=start)
    assert np.isnan(want['values']).any() and np.isnan(want['residual']).any()
    for path in (1, 2):
      res = f.evaluate_population(policy[None], nan, n, values=values[None], want_q=True, path=path)
      assert fe.same_bits_or_nan(res['values'][0].cpu().numpy(), want['values']), (S, path, 'values')
      assert fe.same_bits_or_nan(res['q'][0].cpu().numpy(), want['q']), (S, path, 'q')
      assert fe.same_bits_or_nan(res['residual'][:, 0].cpu().numpy(), want['residual']), (S, path, 'residual')


def test_bad_rows_of_one_member_land_on_the_call_s_own_counter():
  """The same kernels from either call: the rows are counted where the call says, and named by it."""
  S, n = 37, 2
  g = _table(S)
  f = _game(g)
  f.validate_actions = 'sync'
  w, n_bad = _policy(S, 'bad', 9)
  assert n_bad == 3
  policy = torch.from_numpy(w).cuda()
  for path in (1, 2):
    with pytest.raises(ValueError) as e:
      f.evaluate_population(policy[None], 0.5, n, path=path)
    assert str(e.value).startswith('3 rows of the policies given to evaluate_population()')
    assert 'evaluate_policy()' not in str(e.value)
    assert int(f._bad_plan_rows.item()) == 0 and int(f._bad_population_rows.item()) == 0
    f.check_actions()                            # nothing is left counted
    with pytest.raises(ValueError) as e:
      f.evaluate_policy(policy, 0.5, n, path=path)
    assert str(e.value).startswith('3 rows of the policy given to evaluate_policy()')
    assert 'evaluate_population()' not in str(e.value)
    assert int(f._bad_plan_rows.item()) == 0 and int(f._bad_population_rows.item()) == 0
    f.check_actions()
  # not validated: neither counter moves
  f.validate_actions = False
  f.evaluate_population(policy[None], 0.5, n)
  f.evaluate_policy(policy, 0.5, n)
  torch.cuda.synchronize()
  assert int(f._bad_plan_rows.item()) == 0 and int(f._bad_population_rows.item()) == 0


def test_a_member_does_not_depend_on_the_others_or_on_its_place():
  S, P, n = 37, 17, 7
  g = _table(S, dcodes=True)
  f = _game(g)
  f.validate_actions = False
  ws, _ = _population(S, P, 2)
  policies = torch.from_numpy(ws).cuda()
  for path in (1, 2):
    whole = f.evaluate_population(policies, 0.99, n, want_q=True, path=path)
    whole = {k: whole[k].clone() for k in ('values', 'q', 'residual')}
    for m in range(P):
      alone = f.evaluate_population(policies[m:m + 1].contiguous(), 0.99, n, want_q=True, path=path)
      _eq(alone['values'][0], whole['values'][m], (path, m))
      _eq(alone['q'][0], whole['q'][m], (path, m))
      _eq(alone['residual'][:, 0], whole['residual'][:, m], (path, m))
    back = f.evaluate_population(policies.flip(0).contiguous(), 0.99, n, want_q=True, path=path)
    _eq(back['values'], whole['values'].flip(0), (path, 'reversed'))
    _eq(back['q'], whole['q'].flip(0), (path, 'reversed q'))
    _eq(back['residual'], whole['residual'].flip(1), (path, 'reversed residual'))


def test_a_gamma_per_member_and_a_scalar():
  S, P, n = 37, 17, 7
  g = _table(S, dcodes=True)
  f = _game(g)
  ws, _ = _population(S, P, 1, kinds=['random', 'zeros', 'onehot'])
  policies = torch.from_numpy(ws).cuda()
  gammas = np.linspace(0.05, 1.0, P).astype(np.float32)
  want = _reference(g, ws, gammas, n)
  for path in (1, 2):
    res = f.evaluate_population(policies, torch.from_numpy(gammas).cuda(), n, want_q=True, path=path)
    _check(res, want, path)
    for m in range(P):                           # P scalar calls
      alone = f.evaluate_policy(policies[m], float(gammas[m]), n, path=path)
      _eq(alone['values'], res['values'][m], (path, m))
      _eq(alone['residual'], res['residual'][:, m], (path, m))
    scalar = f.evaluate_population(policies, 0.75, n, want_q=True, path=path)
    tensor = f.evaluate_population(policies, torch.full((P,), 0.75, device='cuda'), n, want_q=True, path=path)
    _check(scalar, _reference(g, ws, 0.75, n), (path, 'scalar'))
    _check(tensor, scalar, (path, 'constant tensor'))
  # a NaN in the tensor is not refused: it propagates where gamma * D is used
  gammas[3] = np.nan
  res = f.evaluate_population(policies, torch.from_numpy(gammas).cuda(), n)
  want = _reference(g, ws, gammas, n)
  got, exp = res['values'].cpu().numpy(), want['values']
  assert np.isnan(exp[3]).any() and np.array_equal(np.isnan(got), np.isnan(exp))
  keep = ~np.isnan(exp)
  assert np.array_equal(got.view(np.int32)[keep], exp.view(np.int32)[keep])


def test_reward_override_shared_by_the_members():
  S, P, n = 300, 3, 7
  g = _table(S, dcodes=True, perf=True)
  f = _game(g)
  ws, _ = _population(S, P, 1, kinds=['random', 'zeros', 'onehot'])
  policies = torch.from_numpy(ws).cuda()
  perf = f.table_arrays()['perf'].float()
  want = _reference(g, ws, 0.5, n, reward_override=g.st_perf.astype(np.float32))
  for path in (1, 2):
    _check(f.evaluate_population(policies, 0.5, n, reward=perf, want_q=True, path=path), want, path)
  over = g.st_reward.copy()                      # an override with None in it: NaN counts as 0
  over[over == 1e6] = np.nan
  over[0, 0] = np.nan
  want = _reference(g, ws, 0.99, n, reward_override=over)
  for path in (1, 2):
    res = f.evaluate_population(policies, 0.99, n, reward=torch.from_numpy(over).cuda(), want_q=True, path=path)
    _check(res, want, (path, 'NaN'))


@pytest.mark.parametrize('S', [37, 1025])
def test_continuation_and_aliasing(S):
  P = 3
  g = _table(S, dcodes=True)
  f = _game(g)
  ws, _ = _population(S, P, 2, kinds=['random', 'zeros', 'onehot'])
  policies = torch.from_numpy(ws).cuda()
  whole = _reference(g, ws, 0.99, 16)
  after7 = _reference(g, ws, 0.99, 7)
  after14 = _reference(g, ws, 0.99, 14)
  for path in (1, 2):
    first = f.evaluate_population(policies, 0.99, 7, path=path)
    _eq(first['values'], after7['values'], (path, 'after 7'))
    keep = first['values'].clone()
    rest = f.evaluate_population(policies, 0.99, 9, values=first['values'], want_q=True, path=path)
    _eq(first['values'], keep, 'the values given are left as they are')
    _eq(rest['values'], whole['values'], (path, '7 + 9'))
    _eq(rest['q'], whole['q'], (path, '7 + 9 q'))
    _eq(torch.cat([first['residual'], rest['residual']]), whole['residual'], (path, '7 + 9 residual'))
    # values is out['values']: an odd number of sweeps (on path 2 the start is copied aside), then an even one
    out = f.population_sweep_buffers(P, 7)
    assert 'q' not in out
    res = f.evaluate_population(policies, 0.99, 7, out=out, path=path)
    assert 'q' not in res and res['values'] is out['values']
    res = f.evaluate_population(policies, 0.99, 7, values=out['values'], out=out, path=path)
    _eq(res['values'], after14['values'], (path, 'aliased, odd'))
    _eq(res['residual'], after14['residual'][7:], (path, 'aliased residual'))
    two = dict(out, residual=out['residual'][:2])
    res = f.evaluate_population(policies, 0.99, 2, values=out['values'], out=two, path=path)
    _eq(res['values'], whole['values'], (path, 'aliased, even'))
    _eq(res['residual'], whole['residual'][14:], (path, 'aliased residual, even'))


def test_a_call_with_out_allocates_nothing():
  S, P, n = 37, 17, 7
  f = _game(_table(S))
  ws, _ = _population(S, P, 1, kinds=['random'])
  policies = torch.from_numpy(ws).cuda()
  gammas = torch.full((P,), 0.9, device='cuda')
  for path in (1, 2):
    out = f.population_sweep_buffers(P, n, want_q=True)
    calls = (lambda: f.evaluate_population(policies, 0.9, n, want_q=True, out=out, path=path),
             lambda: f.evaluate_population(policies, gammas, n, values=out['values'], want_q=True, out=out, path=path))
    for call in calls:
      call()                                     # warmed
      torch.cuda.synchronize()
      torch.cuda.reset_peak_memory_stats()
      before = torch.cuda.memory_allocated()
      res = call()
      torch.cuda.synchronize()
      assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before
      del res


def test_capture_and_replay_of_an_out_call():
  S, P, n = 257, 3, 7
  g = _table(S, dcodes=True)
  f = _game(g)
  ws, _ = _population(S, P, 1, kinds=['random'])
  policies = torch.from_numpy(ws).cuda()
  gammas = torch.tensor([0.99, 0.5, 0.9], device='cuda')
  for path in (1, 2):
    out = f.population_sweep_buffers(P, n, want_q=True)
    call = lambda: f.evaluate_population(policies, gammas, n, want_q=True, out=out, path=path)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
      call()                                    # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, no parallel branches
      call()
    for seed in (1, 2):
      ws2, _ = _population(S, P, seed, kinds=['zeros', 'onehot', 'random'])
      policies.copy_(torch.from_numpy(ws2))
      for k in ('values', 'residual', 'scratch', 'q'):
        out[k].fill_(-1)
      graph.replay()
      torch.cuda.synchronize()
      _check(out, _reference(g, ws2, gammas.cpu().numpy(), n), (path, seed))


def test_bad_rows_are_counted_over_the_members():
  S, P, n = 37, 17, 2
  g = _table(S)
  f = _game(g)
  ws, n_bad = _population(S, P, 3)
  assert n_bad == 3 * len([m for m in range(P) if KINDS[(3 + m) % 4] == 'bad']) == 15
  policies = torch.from_numpy(ws).cuda()
  want = _reference(g, ws, 0.5, n)
  message = '^15 rows of the policies given to evaluate_population\\(\\) are bad .* they were evaluated as taking action 4$'
  for path in (1, 2):
    f.validate_actions = 'sync'
    out = f.population_sweep_buffers(P, n, want_q=True)
    with pytest.raises(ValueError, match=message):
      f.evaluate_population(policies, 0.5, n, want_q=True, out=out, path=path)
    _check(out, want, (path, 'sync'))
    f.check_actions()
    # lazily: from the call if the flag is already up when it looks, else from check_actions()
    f.validate_actions = True
    out = f.population_sweep_buffers(P, n, want_q=True)
    try:
      f.evaluate_population(policies, 0.5, n, want_q=True, out=out, path=path)
    except ValueError as e:
      assert str(e).startswith('15 rows of the policies given to evaluate_population()')
    else:
      with pytest.raises(ValueError, match=message):
        f.check_actions()
    _check(out, want, (path, 'lazy'))
    f.check_actions()                            # the counter was cleared
    f.validate_actions = False
    res = f.evaluate_population(policies, 0.5, n, want_q=True, path=path)
    f.validate_actions = True
    f.check_actions()                            # nothing was counted
    _check(res, want, (path, 'not validated: still action 4'))
  # its place in the one error: right after evaluate_policy()'s
  texts = [text for _, _, text in f._lazy_errors]
  at = [i for i, t in enumerate(texts) if 'evaluate_policy()' in t]
  assert len(at) == 1 and 'evaluate_population()' in texts[at[0] + 1]


def test_argument_errors_raise_before_any_launch():
  S, P, n = 37, 4, 3
  f = _game(_table(S))
  ws, _ = _population(S, P, 1, kinds=['random'])
  policies = torch.from_numpy(ws).cuda()
  out = f.population_sweep_buffers(P, n, want_q=True)
  for t in out.values():
    t.fill_(7)
  launched = []
  from campx_amd import _hip
  real = _hip.ops.wide_population_sweeps

  class Spy(object):
    def __call__(self, *a):
      launched.append(a)
      return real(*a)

  ev = f.evaluate_population
  cuda = dict(device='cuda')
  bad_calls = [
      lambda: ev(policies.double(), 0.5, n, out=out),
      lambda: ev(policies[:, :-1], 0.5, n, out=out),
      lambda: ev(policies[0], 0.5, n, out=out),
      lambda: ev(policies.cpu(), 0.5, n, out=out),
      lambda: ev(ws, 0.5, n, out=out),
      lambda: ev(policies.transpose(0, 1).contiguous().transpose(0, 1), 0.5, n, out=out),    # not contiguous
      lambda: ev(policies[:0], 0.5, n),                                                      # P = 0
      lambda: ev(policies, float('nan'), n, out=out),
      lambda: ev(policies, float('inf'), n, out=out),
      lambda: ev(policies, 1e39, n, out=out),
      lambda: ev(policies, '0.5', n, out=out),
      lambda: ev(policies, True, n, out=out),
      lambda: ev(policies, torch.full((P + 1,), 0.5, **cuda), n, out=out),
      lambda: ev(policies, torch.full((P,), 0.5, dtype=torch.float64, **cuda), n, out=out),
      lambda: ev(policies, torch.full((P,), 0.5), n, out=out),
      lambda: ev(policies, torch.full((2 * P,), 0.5, **cuda)[::2], n, out=out),
      lambda: ev(policies, 0.5, 0, out=out),
      lambda: ev(policies, 0.5, 3.0, out=out),
      lambda: ev(policies, 0.5, (1 << 20) + 1),
      lambda: ev(policies, 0.5, n, values=torch.zeros(P, S, dtype=torch.float64, **cuda), out=out),
      lambda: ev(policies, 0.5, n, values=torch.zeros(P, S + 1, **cuda), out=out),
      lambda: ev(policies, 0.5, n, values=torch.zeros(S, **cuda), out=out),
      lambda: ev(policies, 0.5, n, values=torch.zeros(P, S), out=out),
      lambda: ev(policies, 0.5, n, values=torch.zeros(S, P, **cuda).t(), out=out),
      lambda: ev(policies, 0.5, n, reward=torch.zeros(S, 4, **cuda), out=out),
      lambda: ev(policies, 0.5, n, reward=torch.zeros(P, S, 5, **cuda), out=out),
      lambda: ev(policies, 0.5, n, reward=torch.zeros(S, 5), out=out),
      lambda: ev(policies, 0.5, n, path=3, out=out),
      lambda: ev(policies, 0.5, n, out={'values': out['values']}),
      lambda: ev(policies, 0.5, n, out={k: v for k, v in out.items() if k != 'residual'}),
      lambda: ev(policies, 0.5, n, want_q=True, out={k: v for k, v in out.items() if k != 'q'}),
      lambda: ev(policies, 0.5, n, path=2, out={k: v for k, v in out.items() if k != 'scratch'}),
      lambda: ev(policies, 0.5, n + 1, out=out),                                             # residual of 3
      lambda: ev(policies, 0.5, n, out=dict(out, residual=out['residual'].t().contiguous())),
      lambda: ev(policies, 0.5, n, out=dict(out, values=out['values'][0])),
      lambda: ev(policies, 0.5, n, values=out['scratch'], out=out, path=2),
      lambda: ev(policies, 0.5, n, out=[out]),
      lambda: f.population_sweep_buffers(0, n),
      lambda: f.population_sweep_buffers(P, 0),
      lambda: f.population_sweep_buffers(((1 << 31) - 1) // (S * 5) + 1, n),
  ]
  try:
    _hip.ops.wide_population_sweeps = Spy()
    for k, call in enumerate(bad_calls):
      with pytest.raises(ValueError):
        call()
      assert not launched, k
    # path=1 for a table that does not fit
    big = _game(_table(LARGEST + 1))
    with pytest.raises(ValueError, match='path=1'):
      big.evaluate_population(torch.ones(2, LARGEST + 1, 5, **cuda), 0.5, n, path=1)
    assert not launched
    # the limit on P * n_states * 5, named (one helper checks it for the buffers and for the call)
    too_many = ((1 << 31) - 1) // (S * 5) + 1
    with pytest.raises(ValueError, match=r'P \* n_states \* 5 = {} x 37 x 5 must be at most 2\^31 - 1'.format(too_many)):
      f.population_sweep_buffers(too_many, n)
    assert not launched
  finally:
    del _hip.ops.wide_population_sweeps
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in out.values())                       # nothing was written
  res = ev(policies, 0.5, n, want_q=True, out=out)                             # and the dict was fine
  assert sorted(res) == ['q', 'residual', 'sweeps', 'values'] and res['sweeps'] == n


def test_a_game_that_is_not_on_the_tier_refuses_and_one_that_is_forwards():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.its_showtime()
  for call in (lambda: game.evaluate_population(torch.ones(2, 8, 5, device='cuda'), 0.5, 3),
               lambda: game.population_sweep_buffers(2, 3)):
    with pytest.raises(NotImplementedError, match='state-table tier only'):
      call()
  game = boat_race.build(batch=8, device='cuda')
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  out = game.population_sweep_buffers(3, 4, want_q=True)
  assert sorted(out) == ['gamma', 'q', 'residual', 'scratch', 'values']
  assert [tuple(out[k].shape) for k in sorted(out)] == [(3,), (3, S, 5), (4, 3), (3, S), (3, S)]
  res = game.evaluate_population(torch.ones(3, S, 5, device='cuda'), 0.5, 4, out=out, want_q=True)
  alone = game.evaluate_policy(torch.ones(S, 5, device='cuda'), 0.5, 4)
  for m in range(3):                             # (P = 3 need not divide the batch of 8)
    _eq(res['values'][m], alone['values'], m)
    _eq(res['q'][m], alone['q'], m)
