"""`WideGame.evaluate_policy()` / `value_iteration()` / `table_arrays()` on the GPU (csrc/k_plan.hip,
`campx::wide_sweeps`) against tests/planning_reference.py - a numpy float32 restatement of the rule
in include/campx_hip.h - bit for bit: every comparison is on the int32 views of the float arrays,
with no tolerance, except the tie to rollouts, which the signed zero of `0 * q` makes an `==`.

Tables come from `wide_table_reference.make_table()` through the production constructor, as in
tests/test_wide_table_fuzz.py.  Sizes: one state, the kernels' thread counts either side (255,
256, 257; 1 023, 1 025: one state per thread of the LDS workgroup, and two), the plan's largest
table in LDS and the next, for either reduction.  Every case runs both forced paths where the
table fits LDS, so the two kernels are also checked against each other.  Inputs are finite and
away from subnormals (weights >= 2^-20 or exactly 0); tests/test_float_edges.py holds the same
kernels to the rule at subnormals, signed zeros, overflow and NaN.
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
SIZES = [1, 2, 5, 37, 255, 256, 257, 1023, 1025]
SWEEPS = [1, 2, 7, 64]
GAMMAS = [1.0, 0.99, 0.5]
KINDS = ['random', 'zeros', 'onehot', 'bad']


def _plan(S, policy, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_sweeps_plan(S, policy, 0, LDS_MAX, path, out)
  return code, list(out)


def _largest(policy):
  lo, hi = 1, 1 << 14
  while lo < hi:                               # the largest S the plan puts in LDS
    mid = (lo + hi + 1) // 2
    lo, hi = (mid, hi) if _plan(mid, policy)[1][0] == 1 else (lo, mid - 1)
  return lo


def _fits(S, policy):
  return _plan(S, policy, path=1)[0] == 0


@functools.lru_cache(maxsize=None)
def _table(S, dcodes=False, perf=False, any_reward=True):
  return ref.make_table(7000 + S, 4, 4, 2, 1, S, dcodes=dcodes and S >= 4, perf=perf,
                        any_reward=any_reward)


def _game(g, batch=1):
  from campx_amd import wide
  f = wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), batch, 'cuda', g)
  assert f.n_states == g.n_states
  return f


def _policy(S, kind, seed):
  """-> (weights float32 [S, 5], number of bad rows)"""
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


def _bits(x):
  x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
  return x.view(np.int32) if x.dtype == np.float32 else x


def _eq(got, want, what):
  got, want = _bits(got), _bits(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
  assert np.array_equal(got, want), (what, int((got != want).sum()))


def _check(res, want, n, greedy, what):
  assert res['sweeps'] == n
  _eq(res['values'], want['values'], (what, 'values'))
  _eq(res['q'], want['q'], (what, 'q'))
  _eq(res['residual'], want['residual'], (what, 'residual'))
  if greedy:
    _eq(res['greedy'], want['greedy'], (what, 'greedy'))
  else:
    assert 'greedy' not in res


def _reference(g, gamma, n, policy=None, **kw):
  return plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, gamma, n, policy=policy, **kw)


def _paths(S, policy):
  return ([1] if _fits(S, policy) else []) + [2, 0]


def _cases():
  sizes = SIZES + [_largest(0), _largest(0) + 1, _largest(1), _largest(1) + 1]
  return [(S, i) for i, S in enumerate(sizes)]


def test_the_plan_is_the_one_the_sizes_were_chosen_for():
  assert (_largest(0), _largest(1)) == (3068, 2045)
  from campx_amd import _hip
  assert _hip.config_get('wide_lds_max') == LDS_MAX


@pytest.mark.parametrize('S,i', _cases(), ids=lambda x: str(x))
def test_both_paths_equal_the_reference_and_each_other(S, i):
  for j, n in enumerate(SWEEPS):
    gamma, kind, dcodes = GAMMAS[(i + j) % 3], KINDS[(i + j) % 4], (i + j) % 2 == 1
    g = _table(S, dcodes=dcodes)
    f = _game(g)
    f.validate_actions = 'sync'
    what = (S, n, gamma, kind, dcodes)
    # ---- the value of a policy
    w, n_bad = _policy(S, kind, 100 * i + j)
    policy = torch.from_numpy(w).cuda()
    want = _reference(g, gamma, n, policy=w)
    assert want['bad_rows'] == n_bad
    for path in _paths(S, 1):
      if n_bad:
        out = f.sweep_buffers(n, greedy=False)
        with pytest.raises(ValueError, match='^{} rows of the policy given to evaluate_policy'.format(n_bad)):
          f.evaluate_policy(policy, gamma, n, out=out, path=path)
        res = dict(out, sweeps=n)
        del res['scratch']
      else:
        res = f.evaluate_policy(policy, gamma, n, path=path)
      _check(res, want, n, False, what + ('policy', path))
    # ---- value iteration
    want = _reference(g, gamma, n)
    for path in _paths(S, 0):
      _check(f.value_iteration(gamma, n, path=path), want, n, True, what + ('greedy', path))
    f.check_actions()                              # nothing is left counted


def test_table_arrays_are_the_table():
  for S, dcodes, perf, reward in ((37, True, True, True), (5, False, False, True), (300, True, False, False),
                                  (1, False, True, True)):
    g = _table(S, dcodes, perf, reward)
    tabs = _game(g).table_arrays()
    assert sorted(tabs) == ['discount', 'done', 'next_state', 'perf', 'reward']
    assert all(t.device.type == 'cuda' and tuple(t.shape) == (S, 5) and t.is_contiguous() for t in tabs.values())
    _eq(tabs['next_state'], g.st_next.astype(np.int32), 'next_state')
    _eq(tabs['reward'], g.st_reward.astype(np.float32), 'reward')          # bitwise, NaN included
    _eq(tabs['done'], g.st_done.astype(np.uint8), 'done')
    _eq(tabs['discount'], g.st_discount.astype(np.float32), 'discount')
    _eq(tabs['perf'], g.st_perf.astype(np.int8), 'perf')


def test_a_table_without_rewards_keeps_every_value_zero():
  g = _table(37, any_reward=False)
  f = _game(g)
  w, _ = _policy(37, 'random', 5)
  for path in (1, 2):
    res = f.evaluate_policy(torch.from_numpy(w).cuda(), 0.99, 7, path=path)
    _check(res, _reference(g, 0.99, 7, policy=w), 7, False, path)
    assert not res['values'].any() and not res['q'].any() and not res['residual'].any()
    res = f.value_iteration(0.99, 7, path=path)
    _check(res, _reference(g, 0.99, 7), 7, True, path)
    assert not res['values'].any() and not res['greedy'].any()


@pytest.mark.parametrize('S', [37, 1025])
def test_continuation_aliasing_and_want_q(S):
  g = _table(S, dcodes=True)
  f = _game(g)
  w, _ = _policy(S, 'zeros', 11)
  policy = torch.from_numpy(w).cuda()
  for pol, pw in ((policy, w), (None, None)):
    call = (lambda *a, **k: f.evaluate_policy(pol, *a, **k)) if pol is not None else f.value_iteration
    want = _reference(g, 0.99, 16, policy=pw)
    for path in (1, 2):
      # 7 sweeps then 9 more equal 16
      first = call(0.99, 7, path=path)
      _eq(first['values'], want['history'][7], 'after 7')
      keep = first['values'].clone()
      rest = call(0.99, 9, values=first['values'], path=path)
      _eq(first['values'], keep, 'the values given are left as they are')
      _eq(rest['values'], want['values'], '7 + 9')
      _eq(rest['q'], want['q'], '7 + 9 q')
      _eq(torch.cat([first['residual'], rest['residual']]), want['residual'], '7 + 9 residual')
      # the same through out=, v_in aliasing v_out: odd and even numbers of sweeps
      out = f.sweep_buffers(7, want_q=False, greedy=pol is None)
      assert 'q' not in out
      res = call(0.99, 7, out=out, want_q=False, path=path)
      assert 'q' not in res and res['values'] is out['values']
      _eq(out['values'], want['history'][7], 'out=')
      for n, total in ((7, 14), (2, 16)):
        res = call(0.99, n, values=out['values'], out=dict(out, residual=out['residual'][:n]),
                   want_q=False, path=path)
        _eq(res['values'], want['history'][total], ('aliased', total))
        _eq(res['residual'], want['residual'][total - n:total], ('aliased residual', total))
      # one sweep in place
      one = call(0.99, 1, values=rest['values'], out=dict(out, values=rest['values'], residual=out['residual'][:1]),
                 want_q=False, path=path)
      _eq(one['values'], _reference(g, 0.99, 17, policy=pw)['values'], 'one sweep in place')


def test_reward_override_with_the_hidden_performance():
  g = _table(300, dcodes=True, perf=True)
  f = _game(g)
  perf = f.table_arrays()['perf'].float()
  over = g.st_perf.astype(np.float32)
  greedy = f.value_iteration(0.5, 7)['greedy']
  policy = torch.nn.functional.one_hot(greedy.long(), 5).float().contiguous()
  want = _reference(g, 0.5, 7, policy=policy.cpu().numpy(), reward_override=over)
  for path in (1, 2):
    _check(f.evaluate_policy(policy, 0.5, 7, reward=perf, path=path), want, 7, False, path)
  # an override with None in it: NaN counts as 0
  over = g.st_reward.copy()
  over[over == 1e6] = np.nan
  want = _reference(g, 0.99, 7, reward_override=over)
  for path in (1, 2):
    _check(f.value_iteration(0.99, 7, reward=torch.from_numpy(over).cuda(), path=path), want, 7, True, path)


def test_tol_stops_at_the_block_the_residuals_predict():
  g = _table(257)
  f = _game(g)
  want = _reference(g, 0.5, 64)
  tol = float(want['residual'][9])
  first = int(np.flatnonzero(want['residual'] <= np.float32(tol))[0])
  assert first <= 9
  for path in (1, 2):
    for every in (4, 32, 1):
      ran = min(64, (first // every + 1) * every)
      res = f.value_iteration(0.5, 64, tol=tol, check_every=every, path=path)
      assert res['sweeps'] == ran and tuple(res['residual'].shape) == (ran,)
      ref_ran = _reference(g, 0.5, ran)
      _check(res, ref_ran, ran, True, (path, every))
  # a tolerance never met runs them all
  res = f.value_iteration(1.0, 7, tol=0.0, check_every=3)
  _check(res, _reference(g, 1.0, 7), 7, True, 'tol 0')


def test_capture_and_replay_of_an_out_call():
  g = _table(257, dcodes=True)
  f = _game(g)
  w, _ = _policy(257, 'random', 3)
  policy = torch.from_numpy(w).cuda()
  for path in (1, 2):
    out = f.sweep_buffers(7, greedy=False)
    call = lambda: f.evaluate_policy(policy, 0.99, 7, out=out, path=path)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
      call()                                    # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, no parallel branches
      call()
    for seed in (1, 2):
      w2, _ = _policy(257, 'zeros', seed)
      policy.copy_(torch.from_numpy(w2))
      for t in out.values():
        t.fill_(-1)
      graph.replay()
      torch.cuda.synchronize()
      _check(dict(out, sweeps=7), _reference(g, 0.99, 7, policy=w2), 7, False, (path, seed))


def test_bad_rows_raise_lazily_with_their_count():
  g = _table(37)
  f = _game(g)
  w, n_bad = _policy(37, 'bad', 9)
  assert n_bad == 3
  policy = torch.from_numpy(w).cuda()
  want = _reference(g, 0.5, 2, policy=w)
  out = f.sweep_buffers(2, greedy=False)
  message = '^3 rows of the policy given to evaluate_policy'
  # the call does not wait for the count: it raises only if the flag is already up when it looks
  try:
    f.evaluate_policy(policy, 0.5, 2, out=out)
  except ValueError as e:
    assert str(e).startswith(message[1:])
  else:
    with pytest.raises(ValueError, match=message):
      f.check_actions()
  _eq(out['values'], want['values'], 'values under the action-4 rule')
  f.check_actions()
  # counted once per call, however many launches the call makes
  f.validate_actions = 'sync'
  with pytest.raises(ValueError, match=message):
    f.evaluate_policy(policy, 0.5, 2, tol=0.0, check_every=1, out=out)
  _eq(out['values'], want['values'], 'in blocks')
  f.validate_actions = False
  f.evaluate_policy(policy, 0.5, 2)
  f.validate_actions = True
  f.check_actions()


def test_the_values_are_the_returns_of_the_policy_s_rollouts():
  """v_{T-t} at the state frame t starts from IS the discounted return of the T - t frames that
  follow under a deterministic policy: three features, one number."""
  from campx_amd.returns import discounted_returns
  T, B, S = 9, 65, 37
  g = _table(S)
  f = _game(g, batch=B)
  f.showtime()
  def walk(w):                                  # the states a frame starts from, by the table
    s, seen, ends = 0, [], 0
    for _ in range(T):
      seen.append(s)
      a = int(w[s].argmax())
      ends += int(g.st_done[s, a])
      s = 0 if g.st_done[s, a] else int(g.st_next[s, a])
    return len(set(seen)), ends

  # the first seed whose policy leaves the reset state's neighbourhood and ends an episode
  w = next(w for w in (_policy(S, 'onehot', seed)[0] for seed in range(200))
           if walk(w)[0] >= 5 and walk(w)[1] >= 1)
  policy = torch.from_numpy(w).cuda()
  for gamma in (0.99, 0.5):
    out = f.rollout_policy(policy, T, reset_first=True)
    G = discounted_returns(out['reward'], out['done'], gamma, discount=out['discount'])['returns']
    G, states = G.cpu().numpy(), out['states'].cpu().numpy()
    for t in range(T):
      v = f.evaluate_policy(policy, gamma, T - t)['values'].cpu().numpy()
      assert (G[t] == v[states[t]]).all(), (gamma, t)
  assert len(np.unique(states)) == walk(w)[0] and out['done'].any()


def test_argument_errors_raise_before_any_launch():
  g = _table(37)
  f = _game(g)
  S = 37
  w, _ = _policy(S, 'random', 1)
  policy = torch.from_numpy(w).cuda()
  out = f.sweep_buffers(3)
  for t in out.values():
    t.fill_(7)
  launched = []
  from campx_amd import _hip
  real = _hip.ops.wide_sweeps

  class Spy(object):
    def __call__(self, *a):
      launched.append(a)
      return real(*a)

  bad_calls = [
      lambda: f.evaluate_policy(policy.double(), 0.5, 3, out=out),
      lambda: f.evaluate_policy(policy[:-1], 0.5, 3, out=out),
      lambda: f.evaluate_policy(policy.cpu(), 0.5, 3, out=out),
      lambda: f.evaluate_policy(w, 0.5, 3, out=out),
      lambda: f.evaluate_policy(policy, 0.5, 0, out=out),
      lambda: f.value_iteration(0.5, 0, out=out),
      lambda: f.value_iteration(0.5, 3.0, out=out),
      lambda: f.value_iteration(0.5, (1 << 20) + 1),
      lambda: f.value_iteration(float('nan'), 3, out=out),
      lambda: f.value_iteration(float('inf'), 3, out=out),
      lambda: f.value_iteration(1e39, 3, out=out),
      lambda: f.value_iteration('0.5', 3, out=out),
      lambda: f.value_iteration(0.5, 3, values=torch.zeros(S, dtype=torch.float64, device='cuda'), out=out),
      lambda: f.value_iteration(0.5, 3, values=torch.zeros(S + 1, device='cuda'), out=out),
      lambda: f.value_iteration(0.5, 3, values=torch.zeros(S), out=out),
      lambda: f.value_iteration(0.5, 3, reward=torch.zeros(S, 4, device='cuda'), out=out),
      lambda: f.value_iteration(0.5, 3, reward=torch.zeros(S, 5, dtype=torch.int8, device='cuda'), out=out),
      lambda: f.value_iteration(0.5, 3, reward=torch.zeros(S, 5), out=out),
      lambda: f.value_iteration(0.5, 3, tol=-1.0, out=out),
      lambda: f.value_iteration(0.5, 3, tol=float('nan'), out=out),
      lambda: f.value_iteration(0.5, 3, tol=0.1, check_every=0, out=out),
      lambda: f.value_iteration(0.5, 3, path=3, out=out),
      lambda: f.value_iteration(0.5, 3, out={'values': out['values']}),
      lambda: f.value_iteration(0.5, 4, out=out),                               # residual of 3
      lambda: f.value_iteration(0.5, 3, out=dict(out, greedy=out['greedy'].int())),
      lambda: f.value_iteration(0.5, 3, values=out['scratch'], out=out, path=2),
      lambda: f.value_iteration(0.5, 3, out=[out]),
  ]
  try:
    _hip.ops.wide_sweeps = Spy()
    for k, call in enumerate(bad_calls):
      with pytest.raises(ValueError):
        call()
      assert not launched, k
    # path=1 for a table that does not fit
    big = _game(_table(_largest(0) + 1))
    with pytest.raises(ValueError, match='path=1'):
      big.value_iteration(0.5, 3, path=1)
    assert not launched
  finally:
    del _hip.ops.wide_sweeps
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in out.values())                       # nothing was written
  f.value_iteration(0.5, 3, out=out)                                           # and the dict was fine


def test_a_game_that_is_not_on_the_tier_refuses():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.its_showtime()
  for call in (lambda: game.value_iteration(0.5, 3), lambda: game.table_arrays(),
               lambda: game.evaluate_policy(torch.ones(8, 5, device='cuda'), 0.5, 3)):
    with pytest.raises(NotImplementedError, match='state-table tier only'):
      call()
  game = boat_race.build(batch=8, device='cuda')
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  res = game.value_iteration(0.5, 3)
  assert tuple(res['values'].shape) == (S,) and tuple(game.table_arrays()['perf'].shape) == (S, 5)
  res = game.evaluate_policy(torch.ones(S, 5, device='cuda'), 0.5, 3)
  assert tuple(res['q'].shape) == (S, 5)
  with pytest.raises(RuntimeError, match='its_showtime'):
    boat_race.build(batch=8, device='cuda').value_iteration(0.5, 3)
