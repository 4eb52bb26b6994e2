"""The input sets of tests/float_edges.py under the numpy references ALONE: does every set reach
the edges it was built for?  These are conditions on the inputs, not measurements of a kernel - a
comparison on the GPU (tests/test_float_edges.py) that never met a subnormal could not fail on one.
The seeds in tests/float_edges.py were chosen until everything here held.

Per leg: what the leg was built for, and that at least a quarter of every output is finite and
non-zero (pooled over a leg's sweep counts: 64 sweeps of the overflow leg carry infinity to every
state, which is what that count is for).  Per kernel family, over its legs: a subnormal result, a
result that underflowed from non-zero to a zero, a -0.0, an infinity from finite inputs, and - where
a leg asks for one - a NaN from `inf * 0` or `inf - inf`.  No kernel is launched here.
"""

import numpy as np
import pytest

import float_edges as fe
import planning_reference as plan_ref
import policy_reference as policy_ref

F = np.float32
QUARTER = 0.25


def test_the_host_keeps_subnormals_and_the_constants_are_what_they_say():
  assert fe.host_keeps_subnormals()
  bits = lambda x: int(np.array([x], F).view(np.uint32)[0])
  assert bits(fe.SUB_MIN) == 1 and bits(fe.SUB_MAX) == 0x007fffff and bits(fe.NORM_MIN) == 0x00800000
  assert bits(fe.SUB_140) == 1 << 9 and bits(fe.FLT_MAX) == 0x7f7fffff and bits(fe.P127) == 0x7f000000
  assert bits(fe.PZERO) == 0 and bits(fe.NZERO) == 0x80000000
  assert bits(fe.PINF) == 0x7f800000 and bits(fe.NINF) == 0xff800000 and np.isnan(fe.NAN)
  assert fe.subnormal(fe.EDGES).sum() == 6 and len(fe.EDGES) == 17


def test_same_bits_or_nan_tells_zeros_and_subnormals_apart_and_places_nan():
  same = fe.same_bits_or_nan
  a = np.array([0.0, -0.0, fe.SUB_MIN, np.nan, np.inf], F)
  assert same(a, a.copy())
  assert same(a, np.array([0.0, -0.0, fe.SUB_MIN, -np.nan, np.inf], F))      # any NaN for a NaN
  flipped = a.copy()
  flipped.view(np.uint32)[3] ^= 0x80000001                                   # another payload and sign
  assert np.isnan(flipped[3]) and same(a, flipped)
  assert not same(a, np.array([-0.0, -0.0, fe.SUB_MIN, np.nan, np.inf], F))
  assert not same(a, np.array([0.0, -0.0, 0.0, np.nan, np.inf], F))
  assert not same(a, np.array([0.0, -0.0, 2 * fe.SUB_MIN, np.nan, np.inf], F))
  assert not same(a, np.array([0.0, -0.0, fe.SUB_MIN, np.inf, np.inf], F))   # a NaN's place counts
  assert not same(a, np.array([0.0, np.nan, fe.SUB_MIN, np.nan, np.inf], F))
  assert not same(a, a[:4]) and not same(a.reshape(1, 5), a)


# ------------------------------------------------------------------ returns

def _returns_facts(leg):
  """What the leg's reference outputs hold, over all its runs and the four combinations."""
  x = fe.returns_inputs(leg)
  r = np.where(np.isnan(x['reward']), F(0), x['reward'])
  live = x['done'][:-1] == 0
  facts = dict(sub=0, under=0, nzero=0, inf=0, nan_made=0, shares=[])
  for i, (gamma, lam) in enumerate(x['runs']):
    for with_discount, with_values in fe.COMBOS:
      G, A = fe.returns_want(leg, i, with_discount, with_values)
      with np.errstate(all='ignore'):
        c = (F(gamma) * x['discount']).astype(F) if with_discount else np.full(G.shape, F(gamma), F)
      nxt = G[1:]
      facts['sub'] += int(fe.subnormal(G).sum())
      facts['nzero'] += int(fe.negative_zero(G).sum())
      # c * G_next left nothing of two non-zero factors: the frame's return is its (zero) reward
      facts['under'] += int((live & (r[:-1] == 0) & (c[:-1] != 0) & fe.finite_nonzero(nxt) & (G[:-1] == 0)).sum())
      facts['inf'] += int((live & np.isinf(G[:-1]) & np.isfinite(c[:-1]) & np.isfinite(nxt)).sum())
      # a NaN where the frame after holds none: made here, by 0 * inf or inf - inf
      facts['nan_made'] += int((live & np.isnan(G[:-1]) & ~np.isnan(nxt)).sum())
      facts['shares'].append(fe.share_finite_nonzero(G))
      if with_values:
        facts['sub'] += int(fe.subnormal(A).sum())
        facts['nzero'] += int(fe.negative_zero(A).sum())
        facts['nan_made'] += int((np.isnan(A) & ~np.isnan(G) & ~np.isnan(x['values'])).sum())
        facts['shares'].append(fe.share_finite_nonzero(A))
  return facts


@pytest.mark.parametrize('leg', fe.RETURNS_LEGS)
def test_returns_legs_reach_what_they_were_built_for(leg):
  x = fe.returns_inputs(leg)
  T, B = fe.RETURNS_T, fe.RETURNS_B
  assert x['reward'].shape == (T, B) and T == 5 * 8 + 1
  assert not x['done'][:, 1:8].any() and x['done'][:, 8].all()      # never done, always done
  facts = _returns_facts(leg)
  assert min(facts['shares']) >= QUARTER, facts['shares']
  if leg in ('underflow', 'lam'):
    assert facts['sub'] > 1000 and facts['under'] > 10 and facts['nzero'] > 10
    assert np.isnan(x['reward']).any() and np.isnan(x['values']).any() and np.isnan(x['bootstrap']).any()
  if leg == 'underflow':
    assert set(np.unique(x['discount'])) == {0.0, 0.5, 1.0}
    G, A = fe.returns_want(leg, 0, True, True)
    # the forced columns: down through the subnormals to a zero, G's of the reward's sign (A's is +0: its
    # delta ends in the difference of two equal zeros)
    for col, sign in ((0, 0), (1, 1), (2, 0), (3, 1)):
      for out in (G, A):
        assert fe.subnormal(out[:, col]).sum() >= 10 and out[0, col] == 0, col
      assert bool(fe.negative_zero(G[0, col])) == bool(sign) and not fe.negative_zero(A[0, col]), col
    for other in (False, True):                      # a NaN value reaches A and never G
      G2, A2 = fe.returns_want(leg, 0, other, True)
      assert np.isnan(A2).sum() > np.isnan(G2).sum() > 0
  if leg == 'signed_zero':
    assert facts['nzero'] > 1000
    plus, _ = fe.returns_want(leg, 0, True, False)         # gamma 0.5
    minus, _ = fe.returns_want(leg, 1, True, False)        # gamma -0.5
    always = x['reward'][:, 8]
    assert fe.negative_zero(plus[::2, 8]).all() and fe.same_bits_or_nan(plus[:, 8], always)
    assert (plus[:, 0] == 0).all() and not fe.negative_zero(plus[:, 0]).any()     # -0 + +0 = +0
    assert fe.negative_zero(minus[T - 1, 0]) and fe.negative_zero(minus[:, 0]).any() \
        and not fe.negative_zero(minus[:, 0]).all()                                # -0 + -0 = -0
    assert plus[T - 1, 1] < 0 and fe.negative_zero(plus[T - 2, 1])      # 0 * negative = -0
    assert minus[T - 2, 1] == 0 and not fe.negative_zero(minus[T - 2, 1])
  if leg == 'overflow':
    assert facts['inf'] > 100 and facts['nan_made'] > 100
    assert np.isfinite(x['reward']).all() and np.isinf(x['values']).any()
    G, A = fe.returns_want(leg, 0, True, True)             # gamma 2.0
    assert np.isfinite(G[40, 0]) and np.isposinf(G[21, 0]) and np.isnan(G[20, 0]) and np.isnan(G[11, 0])
    assert np.isfinite(G[:11, 0]).all()                    # the done at t = 10 restarts the chain
    for i in (0, 1):                                       # and gamma 1.0 with discounts of 2.0
      G, A = fe.returns_want(leg, i, True, True)
      assert np.isinf(G).sum() > 100 and (np.isnan(A) & ~np.isnan(G)).any()        # inf - inf in delta
  if leg == 'gamma_zero':
    assert set(np.unique(x['discount'])) == {-1.0, 0.0, 0.5, 1.0, 2.0}
    assert facts['nzero'] > 100 and facts['nan_made'] > 100 and facts['sub'] > 100
    G, _ = fe.returns_want(leg, 0, True, False)
    last = x['done'][-1] == 0
    assert np.array_equal(np.isnan(G[-1]), last & np.isinf(x['bootstrap']))        # 0 * inf


def test_the_returns_legs_together_reach_every_edge():
  total = {}
  for leg in fe.RETURNS_LEGS:
    for k, v in _returns_facts(leg).items():
      if k != 'shares':
        total[k] = total.get(k, 0) + v
  assert all(total[k] > 0 for k in ('sub', 'under', 'nzero', 'inf', 'nan_made')), total


# ------------------------------------------------------------------ policy rows

def test_the_edge_rows_are_what_their_names_say():
  for S in fe.SWEEP_SIZES:
    w = fe.edge_policy(S)
    c4, bad = plan_ref.policy_total(w)
    kinds = np.array([fe.row_kind(s) for s in range(S)])
    for kind in fe.ROW_KINDS:
      assert (kinds == kind).sum() >= 3
    assert fe.subnormal(c4[kinds == 'subnormal']).all() and not bad[kinds == 'subnormal'].any()
    assert (c4[kinds == 'one_max'] == fe.FLT_MAX).all() and not bad[kinds == 'one_max'].any()
    assert np.isposinf(c4[kinds == 'two_max']).all() and bad[kinds == 'two_max'].all()
    assert fe.negative_zero(w[kinds == 'negative_zero']).any() and not bad[kinds == 'negative_zero'].any()
    assert int(bad.sum()) == int((kinds == 'two_max').sum())
    # the sampler's and the visitation's tests of a row agree with the planner's
    assert np.array_equal(policy_ref.thresholds(w)[1], bad)
    assert np.array_equal(fe.visit_ref.thresholds(w)[1], bad)


# ------------------------------------------------------------------ sweeps

def _pooled(leg, S, with_policy, key):
  return np.concatenate([fe.sweep_want(leg, S, n, with_policy)[key].reshape(-1) for n in fe.SWEEP_COUNTS])


def _underflowed_backups(leg, S, n, with_policy):
  """Entries of q_n whose product c * v[n] came to a zero from two non-zero factors."""
  g, x = fe.sweep_table(S), fe.sweep_inputs(leg, S)
  want = fe.sweep_want(leg, S, n, with_policy)
  r = np.where(np.isnan(x['reward']), F(0), x['reward'])
  c = (F(x['gamma']) * g.st_discount.astype(F)).astype(F)
  vn = want['history'][-2][g.st_next.astype(np.int64)]
  return (g.st_done == 0) & (r == 0) & (c != 0) & fe.finite_nonzero(vn) & (want['q'] == 0)


@pytest.mark.parametrize('S', fe.SWEEP_SIZES)
@pytest.mark.parametrize('leg', sorted(fe.SWEEP_LEGS))
def test_sweep_legs_reach_what_they_were_built_for(leg, S):
  g, x = fe.sweep_table(S), fe.sweep_inputs(leg, S)
  assert (g.st_dcode != 0).any() and len(set(np.unique(g.st_discount))) > 3
  kinds = np.array([fe.row_kind(s) for s in range(S)])
  n_bad = int((kinds == 'two_max').sum())
  for with_policy in (True, False):
    for key in ('values', 'q'):
      assert fe.share_finite_nonzero(_pooled(leg, S, with_policy, key)) >= QUARTER, (with_policy, key)
    # (a residual is a maximum over the states: one infinite difference makes it infinite, which
    # the overflow leg is for from its first sweep on)
    if leg != 'overflow':
      assert fe.share_finite_nonzero(_pooled(leg, S, with_policy, 'residual')) >= QUARTER
    for n in fe.SWEEP_COUNTS:
      assert fe.sweep_want(leg, S, n, with_policy)['bad_rows'] == (n_bad if with_policy and leg == 'rows' else 0)
  if leg == 'underflow':
    assert fe.subnormal(x['values']).sum() > S // 2 and fe.subnormal(x['reward']).any()
    for with_policy in (True, False):
      want = fe.sweep_want(leg, S, 7, with_policy)
      assert fe.subnormal(want['values']).any() and fe.subnormal(want['q']).sum() > S // 4
      assert fe.negative_zero(want['q']).any() and fe.subnormal(want['residual']).any()
      assert sum(_underflowed_backups(leg, S, n, with_policy).sum() for n in fe.SWEEP_COUNTS) > 0
  if leg == 'overflow':
    assert (np.abs(x['values']) == fe.FLT_MAX).sum() >= 2 and np.isfinite(x['values']).all()
    assert np.isfinite(x['reward'][~np.isnan(x['reward'])]).all()
    for with_policy in (True, False):
      first = fe.sweep_want(leg, S, 1, with_policy)         # an infinity out of finite inputs
      assert np.isinf(first['q']).any() and np.isinf(first['values']).any()
      want = fe.sweep_want(leg, S, 64, with_policy)
      res = want['residual']
      assert np.isinf(res).any() and np.isnan(res).any()
      assert with_policy or np.isinf(want['values']).any()      # (the average is all NaN by then)
      assert np.flatnonzero(np.isinf(res))[0] < np.flatnonzero(np.isnan(res))[0]   # inf, then inf - inf
    q, greedy = (fe.sweep_want(leg, S, 64, False)[k] for k in ('q', 'greedy'))
    some_nan, many_inf = np.isnan(q).any(axis=1), np.isposinf(q).sum(axis=1) >= 2
    assert some_nan.sum() >= 3 and many_inf.sum() >= 3 and (some_nan & ~np.isnan(q[:, 0])).sum() >= 3
    first_inf = np.argmax(np.isposinf(q), axis=1)
    lead = ~np.isnan(q[:, 0])                               # (a NaN q0 is never displaced)
    assert (greedy[many_inf & lead] == first_inf[many_inf & lead]).all()
    assert not np.isnan(q[np.arange(S), greedy.astype(np.int64)])[lead].any()      # NaN never wins
  if leg == 'rows':
    want = fe.sweep_want(leg, S, 7, True)
    w, q = fe.edge_policy(S), want['q']
    with np.errstate(all='ignore'):
      products = (w * q).astype(F)
    tiny = kinds == 'tiny'
    assert fe.subnormal(products[tiny]).mean() > 0.25                               # w * q underflows
    assert ((products == 0) & (w != 0) & fe.finite_nonzero(q))[tiny].any()          # (some to nothing)
    assert fe.subnormal(products[kinds == 'subnormal']).any()                      # num / c4 by a subnormal
    assert fe.finite_nonzero(want['values'][kinds == 'subnormal']).any()
    assert fe.same_bits_or_nan(want['values'][kinds == 'two_max'], q[kinds == 'two_max', 4])


def test_the_sweep_legs_together_reach_every_edge():
  for with_policy in (True, False):
    under = fe.sweep_want('underflow', 37, 7, with_policy)
    over = fe.sweep_want('overflow', 37, 64, with_policy)
    first = fe.sweep_want('overflow', 37, 1, with_policy)
    assert fe.subnormal(under['q']).any() and fe.negative_zero(under['q']).any()
    assert sum(_underflowed_backups('underflow', 37, n, with_policy).sum() for n in fe.SWEEP_COUNTS) > 0
    assert np.isinf(first['values']).any() and np.isnan(over['q']).any()


# ------------------------------------------------------------------ sampler

def test_the_sampler_set_decides_actions_among_subnormals():
  """Integer outputs: the edges are in the sampler's own intermediates, restated here - the
  thresholds and r = u * c4 of every environment-frame - and the condition on the outputs is that
  a quarter of the frames or more sample from an edge row that leaves the action open (so the
  comparison is decided by the f32 product, not by the bad-row rule), with every action taken."""
  S, B, T = fe.SAMPLER_S, fe.SAMPLER_B, fe.SAMPLER_T
  walker, want = fe.sampler_want()
  w = fe.edge_policy(S)
  states, actions = want['states'].astype(np.int64), want['actions']
  kinds = np.array([fe.row_kind(s) for s in range(S)])[states]
  assert want['bad'] == int((kinds == 'two_max').sum()) > 0
  assert (actions[kinds == 'two_max'] == 4).all()
  for kind in fe.ROW_KINDS:
    assert (kinds == kind).sum() >= 20, kind
  open_edge = np.isin(kinds, ('subnormal', 'negative_zero', 'tiny'))
  assert open_edge.mean() >= QUARTER
  assert (kinds[0] == 'subnormal').all()                     # every environment starts at the reset state
  frames = fe.SAMPLER_FIRST + np.arange(T)[:, None]
  x = policy_ref.words(fe.SAMPLER_SEED, np.arange(B, dtype=np.uint64)[None, :], frames)
  c, bad = policy_ref.thresholds(w[states])
  u = ((x >> np.uint32(8)).astype(F) * F(2.0 ** -24)).astype(F)
  with np.errstate(all='ignore'):
    r = (u * c[..., 4]).astype(F)
  sub = kinds == 'subnormal'
  assert fe.subnormal(c[sub][:, [0, 1, 3, 4]]).all() and fe.subnormal(r[sub]).mean() > 0.9
  assert set(np.unique(actions[sub])) == {0, 1, 3, 4}         # (weight 2 is exactly 0: never taken)
  assert np.isposinf(c[kinds == 'two_max'][:, 4]).all()         # an infinity out of finite weights
  assert set(np.unique(actions[kinds == 'negative_zero'])) == {1, 3, 4}
  assert set(np.unique(actions[kinds == 'one_max'])) <= {0, 1, 2} and (actions[kinds == 'one_max'] == 1).mean() > 0.9
  assert len(np.unique(states)) >= 12 and want['done'].any()


def test_the_visitation_counts_of_a_subnormal_row_follow_its_weights():
  S = fe.SAMPLER_S
  want = fe.visitation_want()
  kinds = np.array([fe.row_kind(s) for s in range(S)])
  assert want['bad_rows'] == int((kinds == 'two_max').sum()) >= 3
  counts = want['counts'].astype(np.int64)
  assert (counts.sum(axis=1) == 1 << 24).all()
  sub = counts[kinds == 'subnormal']
  assert (sub == sub[0]).all()
  ideal = np.array([1, 3, 0, 2, 1]) / 7.0 * (1 << 24)
  # c4 = 7 * 2^9 units of 2^-149 and r is rounded to a whole unit: an action's share of the 2^24
  # words is within one unit's worth, 2^24 / 3584, of its weight's (plus the rounding of both ends)
  assert np.abs(sub[0] - ideal).max() <= 2 * (1 << 24) / 3584 + 2, (sub[0], ideal)
  assert sub[0][2] == 0
  assert (counts[kinds == 'two_max'] == [0, 0, 0, 0, 1 << 24]).all()
  assert (counts[kinds == 'negative_zero'][:, [0, 2]] == 0).all()
  assert len(np.flatnonzero(want['final'])) >= 12 and want['finished'].any()


# ------------------------------------------------------------------ learner

@pytest.mark.parametrize('rule', fe.learn_ref.RULES)
def test_the_learner_set_reaches_every_edge(rule):
  x = fe.learner_inputs()
  B, S, T = fe.LEARN_B, fe.LEARN_S, fe.LEARN_T
  q0 = x['q']
  for edge in fe.EDGES:
    same = np.isnan(q0) if np.isnan(edge) else (q0.view(np.uint32) == np.array([edge], F).view(np.uint32)[0])
    assert same.sum() >= 20, edge
  combos = set(zip(x['alpha'].tolist(), x['gamma'].tolist(), x['epsilon'].tolist()))
  assert len(combos) == 5 * 4 * 4
  L, want = fe.learner_want(rule)
  assert want['bad'] == 0
  changed = L.q.view(np.uint32) != q0.view(np.uint32)
  changed &= ~(np.isnan(L.q) & np.isnan(q0))
  assert changed.sum() > B                                    # the learners do learn
  assert fe.share_finite_nonzero(L.q) >= QUARTER and fe.share_finite_nonzero(want['reward_sum']) >= QUARTER
  assert fe.subnormal(L.q[changed]).any()                     # a subnormal result
  step, delta = want['step'], want['delta']
  alpha = np.broadcast_to(x['alpha'], step.shape)
  assert ((step == 0) & fe.finite_nonzero(delta) & (alpha != 0)).any()        # alpha * delta underflowed
  assert fe.subnormal(step).any()
  assert fe.negative_zero(L.q[changed]).any() or fe.negative_zero(step).any()  # a -0.0 out of arithmetic
  finite_before = np.isfinite(q0).all(axis=(1, 2))
  assert np.isinf(L.q[finite_before]).any()                   # an infinity out of a finite table
  assert (np.isnan(L.q) & ~np.isnan(q0)).any()                # a NaN made by inf - inf or 0 * inf
  assert want['explored'].any() and not want['explored'].all() and want['episodes'].any()
  assert np.abs(want['perf_sum']).max() > 0


# ------------------------------------------------------------------ what the comparison can see

def test_a_flushing_or_fused_restatement_differs_on_these_sets():
  """The two usual drifts, restated on the host, are visible to `same_bits_or_nan` on the returns
  sets: subnormal results flushed to a zero of their sign, and `r + c * G_next` as ONE rounding (the
  product of two float32 is exact in float64) where the rule has two."""
  for leg in ('underflow', 'gamma_zero'):
    G, _ = fe.returns_want(leg, 0, True, False)
    flushed = np.where(fe.subnormal(G), np.copysign(F(0), G), G).astype(F)
    assert not fe.same_bits_or_nan(flushed, G)
  x = fe.returns_inputs('lam')
  gamma, lam = x['runs'][3]
  assert gamma == 0.75
  G, _ = fe.returns_want('lam', 3, True, False)
  r = np.where(np.isnan(x['reward']), F(0), x['reward'])
  c = (F(gamma) * x['discount']).astype(F)
  with np.errstate(all='ignore'):
    fused = (r[:-1].astype(np.float64) + c[:-1].astype(np.float64) * G[1:].astype(np.float64)).astype(F)
  fused = np.where(x['done'][:-1] != 0, r[:-1], fused).astype(F)
  differ = ~np.isnan(fused) & (fused.view(np.uint32) != G[:-1].view(np.uint32))
  assert fused.shape == G[:-1].shape and differ.sum() >= 20
