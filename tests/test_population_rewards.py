"""`WideGame.value_iteration_population()` and `evaluate_population(rewards=...)` on the GPU
(csrc/k_plan.hip, `campx::wide_population_solve`) against tests/planning_reference.py run member
by member with `reward_override=rewards[m]`, bit for bit: every comparison is `array_equal` on the
int32 views of the float arrays, with no tolerance.

Tables come from `wide_table_reference.make_table()` through the production constructor, as in
tests/test_population_planning.py.  Sizes: one state; a wave that straddles members (S = 5, 37 with
two or more members to a workgroup); a member that straddles waves (257); more pairs than threads
(1 025); the largest table whose ONE member fits LDS for the form - it differs per form - and the
next.  P = 1, 2, 3, 17, 257: on a chip of 256 compute units a workgroup takes one member up to
P = 256 and two at 257, the last workgroup half full; P = 2 051 gives nine members to a workgroup and
a last one of eight.  Rewards are random with NaNs (None) sprinkled in; member 0 holds the table's
own.  The numpy loop over the members dominates the run time, so the grid of (S, P, sweeps) is
trimmed by hand: every S, every P, every sweep count, the large P with the small S or few sweeps.
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
KEYS = ('values', 'q', 'greedy', 'residual')


def _plan(S, P, policy, rewards, path=0, lds_max=LDS_MAX, n_cus=256):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_population_solve_plan(S, P, policy, rewards, lds_max, n_cus, path, out)
  return code, list(out)


def _largest(policy, rewards):
  lo, hi = 1, 1 << 14
  while lo < hi:                               # the largest S whose one member the plan puts in LDS
    mid = (lo + hi + 1) // 2
    lo, hi = (mid, hi) if _plan(mid, 1, policy, rewards)[1][0] == 1 else (lo, mid - 1)
  return lo


LG, LP, LS = _largest(0, 1), _largest(1, 1), _largest(0, 0)    # greedy / policy with rewards; greedy shared


def _grid(L):
  """(S, P, sweeps) for a form whose largest table that fits is L."""
  return [(1, 257, 7), (1, 3, 64), (5, 17, 64), (5, 257, 2), (37, 3, 64), (37, 257, 7), (37, 17, 1),
          (257, 3, 64), (257, 257, 1), (257, 2, 2), (1025, 17, 7), (1025, 1, 2), (L, 1, 7), (L, 3, 2),
          (L + 1, 2, 7), (L + 1, 17, 1)]


def _paths(S, policy, rewards):
  return ([1] if _plan(S, 1, policy, rewards, path=1)[0] == 0 else []) + [2, 0]


@functools.lru_cache(maxsize=None)
def _table(S, dcodes=False, perf=False):
  return ref.make_table(7000 + S, 4, 4, 2, 1, S, dcodes=dcodes and S >= 4, perf=perf)


def _game(g, batch=1):
  from campx_amd import wide
  f = wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), batch, 'cuda', g)
  assert f.n_states == g.n_states
  return f


def _rewards(g, P, seed):
  """float32 [P, S, 5]: random, one in sixteen NaN (None: counts as 0); member 0 the table's own."""
  rng = np.random.RandomState(seed)
  S = g.n_states
  r = rng.uniform(-1, 1, size=(P, S, 5)).astype(np.float32)
  r[rng.random_sample((P, S, 5)) < 1.0 / 16] = np.nan
  r[0] = np.asarray(g.st_reward, np.float32)
  return r


def _weights(S, P, seed):
  """float32 [P, S, 5] good rows: random weights, some tiny, two in five members with zeros."""
  rng = np.random.RandomState(seed)
  w = rng.uniform(0.5, 2.0, size=(P, S, 5)).astype(np.float32)
  w.reshape(-1)[rng.randint(0, P * S * 5, size=max(1, P * S // 8))] = np.float32(2.0 ** -20)
  zero = rng.random_sample((P, S, 5)) < 0.4
  zero[np.arange(P) % 5 > 1] = False
  w[zero] = 0
  w[:, np.arange(S), rng.randint(0, 5, size=S)] = 1.5          # (no row is all zero)
  return w


def _bits(x):
  x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
  return x.view(np.int32) if x.dtype == np.float32 else x


def _eq(got, want, what):
  got, want = _bits(got), _bits(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
  assert np.array_equal(got, want), (what, int((got != want).sum()))


def _reference(g, rewards, gammas, n, ws=None, values=None, members=None):
  """The reference, member by member -> values [P, S], q [P, S, 5], residual [n, P], bad rows and -
  greedy reduction, `ws` None - greedy [P, S].  `rewards` None: the table's own for every member."""
  P = len(rewards if rewards is not None else ws if ws is not None else gammas)
  members = range(P) if members is None else members
  gammas = np.broadcast_to(np.asarray(gammas, np.float32), (P,))
  each = [plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, gammas[m], n,
                          policy=None if ws is None else ws[m],
                          values=None if values is None else values[m],
                          reward_override=None if rewards is None else rewards[m]) for m in members]
  out = dict(values=np.stack([e['values'] for e in each]), q=np.stack([e['q'] for e in each]),
             residual=np.stack([e['residual'] for e in each], axis=1),
             bad_rows=sum(e['bad_rows'] for e in each))
  if ws is None:
    out['greedy'] = np.stack([e['greedy'] for e in each])
  return out


def _check(res, want, what, keys=KEYS):
  for k in keys:
    if k in want:
      _eq(res[k], want[k], (what, k))


def _cuda(x):
  return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_the_plan_is_the_one_the_sizes_were_chosen_for():
  from campx_amd import _hip
  assert (LG, LP, LS) == (2165, 1600, 3068) and _hip.config_get('wide_lds_max') == LDS_MAX
  assert torch.cuda.get_device_properties(0).multi_processor_count == 256, 'the sizes below assume 256 compute units'
  for policy, rewards in ((0, 1), (1, 1), (0, 0)):
    assert [_plan(5, P, policy, rewards)[1][4] for P in (1, 2, 3, 17, 257)] == [1, 1, 1, 1, 2]
    assert _plan(5, 257, policy, rewards)[1][3] == 129 and _plan(257, 257, policy, rewards)[1][2:] == [320, 257, 1]
    assert _plan(1025, 17, policy, rewards)[1][2:] == [1024, 17, 1]          # two states to a thread
    assert _plan(5, 2051, policy, rewards)[1][3:] == [228, 9] and 2051 % 9 == 8
    assert _plan(37, 2051, policy, rewards)[1][2:] == [256, 342, 6] and 2051 % 6 == 5


GRID_VI = _grid(LG)


@pytest.mark.parametrize('S,P,n', GRID_VI, ids=lambda x: str(x))
def test_value_iteration_under_a_reward_per_member_equals_the_reference(S, P, n):
  i = GRID_VI.index((S, P, n))
  g = _table(S, dcodes=i % 2 == 1)
  f = _game(g)
  rewards = _rewards(g, P, 100 + i)
  gammas = np.linspace(0.3, 1.0, P).astype(np.float32) if i % 2 else np.float32([1.0, 0.99, 0.5][i % 3])
  start = None if i % 3 == 0 else np.random.RandomState(i).uniform(-2, 2, size=(P, S)).astype(np.float32)
  want = _reference(g, rewards, gammas, n, values=start)
  gamma = _cuda(gammas) if i % 2 else float(gammas)
  for path in _paths(S, 0, 1):
    out = f.population_sweep_buffers(P, n, want_q=True, greedy=True)
    for t in out.values():
      t.fill_(-7)
    res = f.value_iteration_population(gamma, n, rewards=_cuda(rewards), want_q=True, out=out, path=path,
                                       values=None if start is None else _cuda(start))
    assert res['sweeps'] == n and res['values'] is out['values'] and res['greedy'] is out['greedy']
    assert res['greedy'].dtype == torch.int8 and tuple(res['greedy'].shape) == (P, S)
    _check(res, want, (S, P, n, path))


GRID_EV = _grid(LP)


@pytest.mark.parametrize('S,P,n', GRID_EV, ids=lambda x: str(x))
def test_evaluation_under_a_reward_per_member_equals_the_reference(S, P, n):
  i = GRID_EV.index((S, P, n))
  g = _table(S, dcodes=i % 2 == 0)
  f = _game(g)
  rewards, ws = _rewards(g, P, 200 + i), _weights(S, P, 300 + i)
  gammas = np.linspace(0.2, 1.0, P).astype(np.float32) if i % 2 == 0 else np.float32([1.0, 0.99, 0.5][i % 3])
  start = None if i % 3 == 1 else np.random.RandomState(i).uniform(-2, 2, size=(P, S)).astype(np.float32)
  want = _reference(g, rewards, gammas, n, ws=ws, values=start)
  assert want['bad_rows'] == 0
  gamma = _cuda(gammas) if i % 2 == 0 else float(gammas)
  for path in _paths(S, 1, 1):
    out = f.population_sweep_buffers(P, n, want_q=True)
    for t in out.values():
      t.fill_(-7)
    res = f.evaluate_population(_cuda(ws), gamma, n, rewards=_cuda(rewards), want_q=True, out=out, path=path,
                                values=None if start is None else _cuda(start))
    assert res['sweeps'] == n and res['values'] is out['values'] and 'greedy' not in res
    _check(res, want, (S, P, n, path))
  f.check_actions()                              # nothing is left counted


GRID_GAMMAS = [(5, 17, 7), (37, 257, 2), (257, 3, 64), (1025, 2, 1), (LS, 3, 2), (LS + 1, 2, 7)]


@pytest.mark.parametrize('S,P,n', GRID_GAMMAS, ids=lambda x: str(x))
def test_value_iteration_under_a_gamma_per_member_and_the_table_s_rewards(S, P, n):
  g = _table(S, dcodes=True)
  f = _game(g)
  gammas = np.linspace(0.05, 1.0, P).astype(np.float32)
  want = _reference(g, None, gammas, n)
  for path in _paths(S, 0, 0):
    res = f.value_iteration_population(_cuda(gammas), n, want_q=True, path=path)
    _check(res, want, (S, P, n, path))
    same = f.value_iteration_population(_cuda(gammas), n, P=P, want_q=True, path=path)
    _check(same, want, (S, P, n, path, 'P given too'))
  # P alone: every member the same problem
  res = f.value_iteration_population(0.75, n, P=P, want_q=True)
  alone = f.value_iteration(0.75, n)
  for m in range(P):
    for k in KEYS:
      _eq(res[k][:, m] if k == 'residual' else res[k][m], alone[k], (S, m, k))


@pytest.mark.parametrize('S', [5, 37])
def test_a_packed_workgroup_the_last_one_short(S):
  """P = 2 051 on 256 compute units: nine (S = 5) or six (S = 37) members to a workgroup, waves that
  hold parts of two or more members, a short last workgroup.  The global path - a workgroup per
  member - is the whole population's reference; numpy's a sample of members, the ends of workgroups
  among them."""
  P, n = 2051, 7
  g = _table(S, dcodes=True)
  f = _game(g)
  f.validate_actions = False
  rewards, ws = _rewards(g, P, S), _weights(S, P, S + 1)
  gammas = np.linspace(0.3, 1.0, P).astype(np.float32)
  start = np.random.RandomState(S).uniform(-2, 2, size=(P, S)).astype(np.float32)
  sample = [0, 1, 5, 6, 8, 9, 10, 17, 18, 1000, 1025, 2042, 2043, 2045, 2046, 2049, 2050]
  dev = dict(rewards=_cuda(rewards), values=_cuda(start), want_q=True)
  a = f.value_iteration_population(_cuda(gammas), n, path=1, **dev)
  b = f.value_iteration_population(_cuda(gammas), n, path=2, **dev)
  for k in KEYS:
    _eq(a[k], b[k], (S, k))
  want = _reference(g, rewards, gammas, n, values=start, members=sample)
  _check({k: a[k][:, sample] if k == 'residual' else a[k][sample] for k in KEYS}, want, (S, 'sample'))
  a = f.evaluate_population(_cuda(ws), _cuda(gammas), n, path=1, **dev)
  b = f.evaluate_population(_cuda(ws), _cuda(gammas), n, path=2, **dev)
  for k in ('values', 'q', 'residual'):
    _eq(a[k], b[k], (S, k, 'policy'))
  want = _reference(g, rewards, gammas, n, ws=ws, values=start, members=sample)
  _check({k: a[k][:, sample] if k == 'residual' else a[k][sample] for k in ('values', 'q', 'residual')},
         want, (S, 'policy sample'))


def _small(S=37, P=17, seed=5):
  g = _table(S, dcodes=True)
  return g, _game(g), _rewards(g, P, seed), _weights(S, P, seed + 1)


def test_permuted_members_give_permuted_results():
  S, P, n = 37, 17, 7
  g, f, rewards, ws = _small(S, P)
  gammas = np.linspace(0.3, 1.0, P).astype(np.float32)
  perm = np.random.RandomState(3).permutation(P)
  for path in (1, 2):
    whole = f.value_iteration_population(_cuda(gammas), n, rewards=_cuda(rewards), want_q=True, path=path)
    mixed = f.value_iteration_population(_cuda(gammas[perm]), n, rewards=_cuda(rewards[perm]), want_q=True,
                                         path=path)
    for k in KEYS:
      _eq(mixed[k], whole[k][:, perm] if k == 'residual' else whole[k][perm], (path, k))
    whole = f.evaluate_population(_cuda(ws), _cuda(gammas), n, rewards=_cuda(rewards), want_q=True, path=path)
    mixed = f.evaluate_population(_cuda(ws[perm]), _cuda(gammas[perm]), n, rewards=_cuda(rewards[perm]),
                                  want_q=True, path=path)
    for k in ('values', 'q', 'residual'):
      _eq(mixed[k], whole[k][:, perm] if k == 'residual' else whole[k][perm], (path, k, 'policy'))
    # a member does not depend on the others: every one alone, as a population of one
    for m in (0, 1, P - 1):
      alone = f.evaluate_population(_cuda(ws[m:m + 1]), _cuda(gammas[m:m + 1]), n, rewards=_cuda(rewards[m:m + 1]),
                                    want_q=True, path=path)
      for k in ('values', 'q', 'residual'):
        _eq(alone[k][:, 0] if k == 'residual' else alone[k][0],
            whole[k][:, m] if k == 'residual' else whole[k][m], (path, m, k))


def test_equal_rows_give_the_bits_of_the_shared_reward():
  S, P, n = 300, 3, 7
  g = _table(S, dcodes=True, perf=True)
  f = _game(g)
  ws = _weights(S, P, 1)
  over = _rewards(g, 2, 9)[1]                    # one random table with NaNs in it
  tiled = _cuda(np.broadcast_to(over, (P, S, 5)))
  perf = f.table_arrays()['perf'].float()
  for path in (1, 2):
    for shared, rows in ((_cuda(over), tiled), (perf, perf.expand(P, -1, -1).contiguous())):
      one = f.evaluate_population(_cuda(ws), 0.9, n, reward=shared, want_q=True, path=path)
      one = {k: one[k].clone() for k in ('values', 'q', 'residual')}
      each = f.evaluate_population(_cuda(ws), 0.9, n, rewards=rows, want_q=True, path=path)
      for k in ('values', 'q', 'residual'):
        _eq(each[k], one[k], (path, k))
      alone = f.value_iteration(0.9, n, reward=shared, path=path)
      each = f.value_iteration_population(0.9, n, rewards=rows, want_q=True, path=path)
      for m in range(P):
        for k in KEYS:
          _eq(each[k][:, m] if k == 'residual' else each[k][m], alone[k], (path, m, k))
  # a shared policy under P rewards: policy.expand(P, -1, -1).contiguous()
  policy = _cuda(ws[0])
  rewards = _rewards(g, P, 4)
  res = f.evaluate_population(policy.expand(P, -1, -1).contiguous(), 0.9, n, rewards=_cuda(rewards))
  for m in range(P):
    alone = f.evaluate_policy(policy, 0.9, n, reward=_cuda(rewards[m]))
    _eq(res['values'][m], alone['values'], m)
    _eq(res['residual'][:, m], alone['residual'], m)


@pytest.mark.parametrize('S,n', [(37, 7), (257, 7), (1025, 2), (1025, 3)])
def test_one_member_gives_the_bits_of_the_single_call(S, n):
  g = _table(S, dcodes=True)
  f = _game(g)
  rewards, ws = _rewards(g, 2, S)[1:], _weights(S, 1, S)
  start = np.random.RandomState(S).uniform(-2, 2, size=(1, S)).astype(np.float32)
  r, v = _cuda(rewards), _cuda(start)
  want = _reference(g, rewards, 0.99, n, values=start)
  want_p = _reference(g, rewards, 0.99, n, ws=ws, values=start)
  for solo_path in (1, 2):
    alone = f.value_iteration(0.99, n, values=v[0], reward=r[0], path=solo_path)
    alone_p = f.evaluate_policy(_cuda(ws[0]), 0.99, n, values=v[0], reward=r[0], path=solo_path)
    for path in (1, 2, 0):
      for gamma in (0.99, torch.full((1,), 0.99, device='cuda')):
        res = f.value_iteration_population(gamma, n, rewards=r, values=v, want_q=True, path=path)
        _check(res, want, (S, path))
        for k in KEYS:
          _eq(res[k][:, 0] if k == 'residual' else res[k][0], alone[k], (S, solo_path, path, k))
        res = f.evaluate_population(_cuda(ws), gamma, n, rewards=r, values=v, want_q=True, path=path)
        _check(res, want_p, (S, path, 'policy'))
        for k in ('values', 'q', 'residual'):
          _eq(res[k][:, 0] if k == 'residual' else res[k][0], alone_p[k], (S, solo_path, path, k, 'policy'))
    # the table's own rewards, one member by P alone
    res = f.value_iteration_population(0.99, n, P=1, want_q=True, path=solo_path)
    alone = f.value_iteration(0.99, n, path=solo_path)
    for k in KEYS:
      _eq(res[k][:, 0] if k == 'residual' else res[k][0], alone[k], (S, solo_path, k, 'own rewards'))
  _eq(v, start, 'the values given are left as they are')


@pytest.mark.parametrize('S', [37, 1025])
def test_continuation_aliasing_and_no_q(S):
  P = 3
  g = _table(S, dcodes=True)
  f = _game(g)
  rewards, ws = _rewards(g, P, 2), _weights(S, P, 3)
  r, w = _cuda(rewards), _cuda(ws)
  for policy in (None, ws):
    call = ((lambda n, **kw: f.value_iteration_population(0.99, n, rewards=r, **kw)) if policy is None else
            (lambda n, **kw: f.evaluate_population(w, 0.99, n, rewards=r, **kw)))
    keys = KEYS if policy is None else ('values', 'q', 'residual')
    whole = _reference(g, rewards, 0.99, 16, ws=policy)
    after7 = _reference(g, rewards, 0.99, 7, ws=policy)
    after14 = _reference(g, rewards, 0.99, 14, ws=policy)
    for path in (1, 2):
      first = call(7, path=path)
      assert 'q' not in first
      _eq(first['values'], after7['values'], (path, 'after 7'))
      if policy is None:
        _eq(first['greedy'], after7['greedy'], (path, 'greedy without q'))
      keep = first['values'].clone()
      rest = call(9, values=first['values'], want_q=True, path=path)
      _eq(first['values'], keep, 'the values given are left as they are')
      _check(dict(rest, residual=torch.cat([first['residual'], rest['residual']])), whole, (path, '7 + 9'), keys)
      # values is out['values']: an odd number of sweeps (on path 2 the start is copied aside), then an even one
      out = f.population_sweep_buffers(P, 7, greedy=policy is None)
      assert 'q' not in out
      res = call(7, out=out, path=path)
      assert 'q' not in res and res['values'] is out['values']
      res = call(7, values=out['values'], out=out, path=path)
      _eq(res['values'], after14['values'], (path, 'aliased, odd'))
      _eq(res['residual'], after14['residual'][7:], (path, 'aliased residual'))
      two = dict(out, residual=out['residual'][:2])
      res = call(2, values=out['values'], out=two, path=path)
      _eq(res['values'], whole['values'], (path, 'aliased, even'))
      _eq(res['residual'], whole['residual'][14:], (path, 'aliased residual, even'))
      if policy is None:
        _eq(res['greedy'], whole['greedy'], (path, 'aliased greedy'))


def test_a_call_with_out_allocates_nothing():
  S, P, n = 37, 17, 7
  g, f, rewards, ws = _small(S, P)
  r, w = _cuda(rewards), _cuda(ws)
  gammas = torch.full((P,), 0.9, device='cuda')
  for path in (1, 2):
    out = f.population_sweep_buffers(P, n, want_q=True, greedy=True)
    assert sorted(out) == ['gamma', 'greedy', 'q', 'residual', 'rewards', 'scratch', 'values']
    assert tuple(out['rewards'].shape) == (P, S, 5) and tuple(out['greedy'].shape) == (P, S)
    out['rewards'].copy_(r)
    calls = (lambda: f.value_iteration_population(0.9, n, rewards=out['rewards'], want_q=True, out=out, path=path),
             lambda: f.value_iteration_population(gammas, n, rewards=r, values=out['values'], want_q=True,
                                                  out=out, path=path),
             lambda: f.value_iteration_population(gammas, n, out=out, path=path),
             lambda: f.evaluate_population(w, gammas, n, rewards=r, want_q=True, out=out, path=path))
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
  gammas = torch.tensor([0.99, 0.5, 0.9], device='cuda')
  for path in (1, 2):
    out = f.population_sweep_buffers(P, n, want_q=True, greedy=True)
    rewards = out['rewards']
    rewards.copy_(_cuda(_rewards(g, P, 0)))
    call = lambda: f.value_iteration_population(gammas, n, rewards=rewards, want_q=True, out=out, path=path)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
      call()                                    # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, no parallel branches
      call()
    for seed in (1, 2):
      fresh = _rewards(g, P, seed)
      rewards.copy_(_cuda(fresh))
      for k in ('values', 'residual', 'scratch', 'q', 'greedy'):
        out[k].fill_(-1)
      graph.replay()
      torch.cuda.synchronize()
      _check(out, _reference(g, fresh, gammas.cpu().numpy(), n), (path, seed))


def test_bad_rows_are_counted_over_the_members_of_the_policy_form():
  S, P, n = 37, 17, 2
  g, f, rewards, ws = _small(S, P)
  ws[2, 3, 1], ws[2, 30, 4], ws[9, 0] = -1.0, np.nan, 0      # three bad rows in two members
  ws[16, 36] = [1, np.inf, 1, 1, 1]
  r, w = _cuda(rewards), _cuda(ws)
  want = _reference(g, rewards, 0.5, n, ws=ws)
  assert want['bad_rows'] == 4
  message = '^4 rows of the policies given to evaluate_population\\(\\) are bad .* they were evaluated as taking action 4$'
  for path in (1, 2):
    f.validate_actions = 'sync'
    out = f.population_sweep_buffers(P, n, want_q=True)
    with pytest.raises(ValueError, match=message):
      f.evaluate_population(w, 0.5, n, rewards=r, want_q=True, out=out, path=path)
    _check(out, want, (path, 'sync'))
    f.check_actions()
    # lazily: from the call if the flag is already up when it looks, else from check_actions()
    f.validate_actions = True
    out = f.population_sweep_buffers(P, n, want_q=True)
    try:
      f.evaluate_population(w, 0.5, n, rewards=r, want_q=True, out=out, path=path)
    except ValueError as e:
      assert str(e).startswith('4 rows of the policies given to evaluate_population()')
    else:
      with pytest.raises(ValueError, match=message):
        f.check_actions()
    _check(out, want, (path, 'lazy'))
    f.check_actions()                            # the counter was cleared
    f.validate_actions = False
    res = f.evaluate_population(w, 0.5, n, rewards=r, want_q=True, path=path)
    f.validate_actions = True
    f.check_actions()                            # nothing was counted
    _check(res, want, (path, 'not validated: still action 4'))
    # the greedy form has no rows to count
    f.value_iteration_population(0.5, n, rewards=r, path=path)
    f.check_actions()


def test_argument_errors_raise_before_any_launch():
  S, P, n = 37, 4, 3
  g, f, rewards, ws = _small(S, P)
  r, w = _cuda(rewards), _cuda(ws)
  out = f.population_sweep_buffers(P, n, want_q=True, greedy=True)
  for t in out.values():
    t.fill_(7)
  launched = []
  from campx_amd import _hip
  real = (_hip.ops.wide_population_solve, _hip.ops.wide_population_sweeps)

  def spy(op):
    def call(*a):
      launched.append(a)
      return op(*a)
    return call

  vi, ev = f.value_iteration_population, f.evaluate_population
  cuda = dict(device='cuda')
  shared = torch.zeros(S, 5, **cuda)
  bad_calls = [
      lambda: vi(0.5, n),                                                          # nothing says P
      lambda: vi(0.5, n, out=out),
      lambda: vi(0.5, n, rewards=r, P=P + 1, out=out),                             # they disagree
      lambda: vi(torch.full((P + 1,), 0.5, **cuda), n, rewards=r, out=out),
      lambda: vi(torch.full((P,), 0.5, **cuda), n, P=P - 1, out=out),
      lambda: vi(0.5, n, P=0),
      lambda: vi(0.5, n, P=-3),
      lambda: vi(0.5, n, P=4.0, out=out),
      lambda: vi(0.5, n, P=True),
      lambda: vi(0.5, n, P=((1 << 31) - 1) // (S * 5) + 1),
      lambda: vi(0.5, n, rewards=r.double(), out=out),
      lambda: vi(0.5, n, rewards=r[:, :-1], out=out),
      lambda: vi(0.5, n, rewards=r[..., :4], out=out),
      lambda: vi(0.5, n, rewards=r[0], out=out),
      lambda: vi(0.5, n, rewards=r.cpu(), out=out),
      lambda: vi(0.5, n, rewards=rewards, out=out),
      lambda: vi(0.5, n, rewards=r[:0]),
      lambda: vi(0.5, n, rewards=r.transpose(0, 1).contiguous().transpose(0, 1), out=out),   # not contiguous
      lambda: vi(float('nan'), n, rewards=r, out=out),
      lambda: vi(float('inf'), n, rewards=r, out=out),
      lambda: vi(1e39, n, rewards=r, out=out),
      lambda: vi('0.5', n, rewards=r, out=out),
      lambda: vi(True, n, rewards=r, out=out),
      lambda: vi(torch.full((P,), 0.5, dtype=torch.float64, **cuda), n, rewards=r, out=out),
      lambda: vi(torch.full((P,), 0.5), n, rewards=r, out=out),
      lambda: vi(torch.full((2 * P,), 0.5, **cuda)[::2], n, rewards=r, out=out),
      lambda: vi(torch.full((P, 1), 0.5, **cuda), n, rewards=r, out=out),
      lambda: vi(0.5, 0, rewards=r, out=out),
      lambda: vi(0.5, 3.0, rewards=r, out=out),
      lambda: vi(0.5, (1 << 20) + 1, rewards=r),
      lambda: vi(0.5, n, rewards=r, values=torch.zeros(P, S, dtype=torch.float64, **cuda), out=out),
      lambda: vi(0.5, n, rewards=r, values=torch.zeros(P, S + 1, **cuda), out=out),
      lambda: vi(0.5, n, rewards=r, values=torch.zeros(S, **cuda), out=out),
      lambda: vi(0.5, n, rewards=r, values=torch.zeros(P + 1, S, **cuda), out=out),
      lambda: vi(0.5, n, rewards=r, path=3, out=out),
      lambda: vi(0.5, n, rewards=r, out={'values': out['values']}),
      lambda: vi(0.5, n, rewards=r, out={k: v for k, v in out.items() if k != 'greedy'}),
      lambda: vi(0.5, n, rewards=r, out=f.population_sweep_buffers(P, n)),            # (no 'greedy' in it)
      lambda: vi(0.5, n, rewards=r, want_q=True, out={k: v for k, v in out.items() if k != 'q'}),
      lambda: vi(0.5, n, rewards=r, path=2, out={k: v for k, v in out.items() if k != 'scratch'}),
      lambda: vi(0.5, n + 1, rewards=r, out=out),                                    # residual of 3
      lambda: vi(0.5, n, rewards=r, out=dict(out, greedy=out['greedy'][0])),
      lambda: vi(0.5, n, rewards=r, out=dict(out, greedy=out['greedy'].int())),
      lambda: vi(0.5, n, rewards=r, values=out['scratch'], out=out, path=2),
      lambda: vi(0.5, n, rewards=r, out=[out]),
      # evaluate_population(rewards=...)
      lambda: ev(w, 0.5, n, reward=shared, rewards=r, out=out),                       # both
      lambda: ev(w, 0.5, n, reward=r, out=out),                                       # 3-D is `rewards`
      lambda: ev(w, 0.5, n, rewards=shared, out=out),
      lambda: ev(w, 0.5, n, rewards=_cuda(_rewards(g, P + 1, 1)), out=out),           # P of the policies
      lambda: ev(w[:P - 1].contiguous(), 0.5, n, rewards=r),
      lambda: ev(w, torch.full((P + 1,), 0.5, **cuda), n, rewards=r, out=out),
      lambda: ev(w, 0.5, n, rewards=r.double(), out=out),
      lambda: ev(w, 0.5, n, rewards=r.cpu(), out=out),
      lambda: ev(w, 0.5, n, rewards=rewards, out=out),
      lambda: ev(w, 0.5, n, rewards=r.transpose(0, 1).contiguous().transpose(0, 1), out=out),
      lambda: f.population_sweep_buffers(0, n, greedy=True),
      lambda: f.population_sweep_buffers(((1 << 31) - 1) // (S * 5) + 1, n, greedy=True),
  ]
  try:
    _hip.ops.wide_population_solve, _hip.ops.wide_population_sweeps = spy(real[0]), spy(real[1])
    for k, call in enumerate(bad_calls):
      with pytest.raises(ValueError):
        call()
      assert not launched, k
    with pytest.raises(ValueError, match=r'value_iteration\(\) is the call'):
      vi(0.5, n)
    with pytest.raises(ValueError, match='rewards says 4, P says 5'):
      vi(0.5, n, rewards=r, P=5)
    with pytest.raises(ValueError, match='not both'):
      ev(w, 0.5, n, reward=shared, rewards=r)
    too_many = ((1 << 31) - 1) // (S * 5) + 1
    with pytest.raises(ValueError, match=r'value_iteration_population\(\): P \* n_states \* 5 = {} x 37 x 5 must be '
                                         r'at most 2\^31 - 1'.format(too_many)):
      vi(0.5, n, P=too_many)
    # path=1 for a table whose one member does not fit WITH its rewards, though it does without
    big = _game(_table(LP + 1))
    ones = torch.ones(2, LP + 1, 5, **cuda)
    with pytest.raises(ValueError, match='path=1'):
      big.evaluate_population(ones, 0.5, n, rewards=ones, path=1)
    assert not launched
    big.evaluate_population(ones, 0.5, n, path=1)
    assert len(launched) == 1
    del launched[:]
    big = _game(_table(LG + 1))
    with pytest.raises(ValueError, match='path=1'):
      big.value_iteration_population(0.5, n, rewards=torch.ones(2, LG + 1, 5, **cuda), path=1)
    assert not launched
  finally:
    del _hip.ops.wide_population_solve, _hip.ops.wide_population_sweeps
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in out.values())                       # nothing was written
  res = vi(0.5, n, rewards=r, want_q=True, out=out)                            # and the dict was fine
  assert sorted(res) == ['greedy', 'q', 'residual', 'sweeps', 'values'] and res['sweeps'] == n
  res = ev(w, 0.5, n, rewards=r, want_q=True, out=out)                         # (a dict with more serves)
  assert sorted(res) == ['q', 'residual', 'sweeps', 'values']


def test_a_game_that_is_not_on_the_tier_refuses_and_one_that_is_forwards():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.its_showtime()
  for call in (lambda: game.value_iteration_population(0.5, 3, P=2),
               lambda: game.population_sweep_buffers(2, 3, greedy=True)):
    with pytest.raises(NotImplementedError, match='state-table tier only'):
      call()
  game = boat_race.build(batch=8, device='cuda')
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  out = game.population_sweep_buffers(3, 4, want_q=True, greedy=True)
  assert [tuple(out[k].shape) for k in ('greedy', 'rewards', 'values')] == [(3, S), (3, S, 5), (3, S)]
  table = game.table_arrays()
  rewards = torch.stack([table['reward'], table['perf'].float(), table['reward'] + table['perf'].float()])
  res = game.value_iteration_population(0.9, 4, rewards=rewards, out=out, want_q=True)
  for m in range(3):                             # (P = 3 need not divide the batch of 8)
    alone = game.value_iteration(0.9, 4, reward=rewards[m])
    for k in KEYS:
      _eq(res[k][:, m] if k == 'residual' else res[k][m], alone[k], (m, k))
