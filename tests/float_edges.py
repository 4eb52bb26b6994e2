"""The edges of float32 - subnormals, signed zeros, overflow, infinities, NaN - as inputs of the
kernels whose rule is "every operation an f32 operation rounded on its own" (include/campx_hip.h):
the comparison, the constants and the seeded input sets that tests/test_float_edges_cpu.py (the
references alone: do the sets reach the edges?) and tests/test_float_edges.py (the GPU against the
references) share.  No torch, no HIP.

A set is built once per process and cached; so is every reference result.  The seeds below were
chosen on the CPU, by tests/test_float_edges_cpu.py's conditions, and are part of the sets.
"""

import functools

import numpy as np

import learner_reference as learn_ref
import planning_reference as plan_ref
import policy_reference as policy_ref
import returns_reference as returns_ref
import visitation_reference as visit_ref
import wide_table_reference as table_ref

F = np.float32


def _from_bits(u):
  return np.array([u], np.uint32).view(F)[0]


SUB_MIN = F(2.0 ** -149)              # the smallest subnormal
SUB_140 = F(2.0 ** -140)
SUB_MAX = _from_bits(0x007fffff)      # the largest subnormal
NORM_MIN = F(2.0 ** -126)             # the smallest normal
P120, P127 = F(2.0 ** 120), F(2.0 ** 127)
FLT_MAX = np.finfo(F).max
PZERO, NZERO = F(0.0), F(-0.0)
PINF, NINF, NAN = F(np.inf), F(-np.inf), F(np.nan)
EDGES = np.array([SUB_MIN, -SUB_MIN, SUB_140, -SUB_140, SUB_MAX, -SUB_MAX, NORM_MIN, -NORM_MIN,
                  PZERO, NZERO, FLT_MAX, -FLT_MAX, P127, -P127, PINF, NINF, NAN], F)


def same_bits_or_nan(a, b):
  """Equal shapes, NaN in the same places, and everywhere else the same bits: -0.0 is not 0.0 and
  a subnormal is exact.  The bits of a NaN are not compared: one that arithmetic generates is
  0xffc00000 on x86 and 0x7fc00000 on the GPU, and no rule here defines the payload."""
  a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
  if a.shape != b.shape:
    return False
  na, nb = np.isnan(a), np.isnan(b)
  return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def host_keeps_subnormals():
  """The host's float32 multiply does not flush: 2^-130 * 0.5 is 2^-131, not 0."""
  x = np.multiply(np.array([2.0 ** -130], F), np.array([0.5], F))[0]
  return bool(x == 2.0 ** -131 and x != 0)


# ---- what an array holds (for the CPU conditions)

def subnormal(x):
  x = np.asarray(x, F)
  return (x != 0) & (np.abs(x) < NORM_MIN)


def negative_zero(x):
  return np.asarray(x, F).view(np.uint32) == np.uint32(0x80000000)


def finite_nonzero(x):
  x = np.asarray(x, F)
  return np.isfinite(x) & (x != 0)


def share_finite_nonzero(x):
  return float(finite_nonzero(x).mean())


def _pick(rng, values, shape, p=None):
  values = np.asarray(values, F)
  return values[rng.choice(len(values), size=shape, p=p)]


# ------------------------------------------------------------------ returns (k_returns.hip)

RETURNS_T, RETURNS_B = 41, 257
RETURNS_LEGS = ('underflow', 'signed_zero', 'overflow', 'gamma_zero', 'lam')
RETURNS_SEEDS = {'underflow': 11, 'signed_zero': 12, 'overflow': 13, 'gamma_zero': 14}
COMBOS = ((True, True), (True, False), (False, True), (False, False))       # discount, values


def _done(rng, p, T, B):
  """done with probability p; columns 0 .. 7 never done, column 8 always."""
  done = (rng.random_sample((T, B)) < p).astype(np.uint8)
  done[:, :8] = 0
  done[:, 8] = 1
  return done


@functools.lru_cache(maxsize=None)
def returns_inputs(leg):
  """-> dict(reward, done, discount, values [T, B], bootstrap [B], runs = ((gamma, lam), ...))."""
  T, B = RETURNS_T, RETURNS_B
  if leg == 'lam':
    # any finite lam: the underflow streams under lam -0.5 and 2.0; and under gamma 0.75, whose
    # products with a subnormal are inexact (0.5 only shifts: a fused multiply-add would not show)
    return dict(returns_inputs('underflow'), runs=((0.5, -0.5), (0.5, 2.0), (-0.5, 2.0), (0.75, 2.0)))
  rng = np.random.RandomState(RETURNS_SEEDS[leg])
  tiny = [2.0 ** -120, -2.0 ** -120, 2.0 ** -126, -2.0 ** -126, 2.0 ** -140, -2.0 ** -140]
  if leg == 'underflow':
    # gamma 0.5: G and A walk down through the subnormals to zero along the never-done columns
    reward = _pick(rng, tiny + [0.0, -0.0, np.nan], (T, B))
    discount = _pick(rng, [1, 0.5, 0], (T, B), p=[0.6, 0.3, 0.1])
    values = _pick(rng, tiny + [0.0, -0.0], (T, B))
    bootstrap = _pick(rng, tiny + [0.0, -0.0], (B,))
    done = _done(rng, 0.1, T, B)
    # columns 0 .. 3: one reward on the last frame and nothing else, so that it halves (or
    # quarters) its way to 2^-149, then to a zero of its own sign
    for col, (r, d) in enumerate(((2.0 ** -120, 1), (-2.0 ** -120, 1), (2.0 ** -126, 0.5), (-2.0 ** -140, 1))):
      reward[:, col] = _pick(rng, [0.0, np.nan], (T,)) if r > 0 else -0.0     # (-0 + -0 stays -0)
      reward[T - 1, col] = r
      discount[:, col] = d
      values[:, col] = 0.0
      bootstrap[col] = 0.0
    values[rng.randint(T, size=3), rng.randint(9, B, size=3)] = np.nan       # a NaN value propagates
    bootstrap[B - 1] = np.nan
    runs = ((0.5, 1.0), (0.5, 0.5), (0.5, 0.0))
  elif leg == 'signed_zero':
    reward = _pick(rng, [-0.0, 0.0, 1, -1, 0.5, -0.5], (T, B), p=[0.3, 0.2, 0.125, 0.125, 0.125, 0.125])
    discount = _pick(rng, [1, 0.5, 0], (T, B))
    values = _pick(rng, [0.0, -0.0, 1, -1, 2, -2], (T, B))
    bootstrap = _pick(rng, [0.0, -0.0, 1, -1], (B,))
    done = _done(rng, 0.15, T, B)
    # column 0: r = -0.0 all the way, a zero bootstrap: c * G is +0 under gamma 0.5 (the sum is
    # +0) and -0 under gamma -0.5 (the sum stays -0).  Column 1: a discount of 0 behind a negative
    # G.  Column 8 (always done): G = r = -0.0.
    reward[:, 0], discount[:, 0], bootstrap[0] = -0.0, 1, 0.0
    reward[:, 1], discount[:, 1], bootstrap[1] = -0.0, 0, -1.0
    reward[T - 1, 1], discount[T - 1, 1] = -1.0, 1
    reward[::2, 8] = -0.0
    runs = ((0.5, 1.0), (-0.5, 1.0), (-0.5, 0.5))
  elif leg == 'overflow':
    reward = _pick(rng, [2.0 ** 120, -2.0 ** 120], (T, B), p=[0.7, 0.3])
    discount = _pick(rng, [2, 1, 0], (T, B), p=[0.6, 0.3, 0.1])
    values = _pick(rng, [2.0 ** 100, -2.0 ** 100, 2.0 ** 120, -2.0 ** 121], (T, B))
    values[rng.randint(T, size=12), rng.randint(9, B, size=12)] = _pick(rng, [np.inf, -np.inf], (12,))
    bootstrap = _pick(rng, [2.0 ** 120, -2.0 ** 120, 2.0 ** 127], (B,))
    bootstrap[B - 2:] = [np.inf, np.nan]
    done = _done(rng, 0.3, T, B)
    # column 0: never done, reaches +inf within eight frames of the end; then a discount of 0
    # (0 * inf is NaN) at t = 20 and a done at t = 10, after which the chain is finite again
    reward[:, 0], discount[:, 0], bootstrap[0] = 2.0 ** 120, 2, 2.0 ** 120
    discount[20, 0] = 0
    done[10, 0] = 1
    discount[:10, 0] = 0.5
    runs = ((2.0, 1.0), (1.0, 0.5), (2.0, 0.0))
  elif leg == 'gamma_zero':
    reward = _pick(rng, [1, -1, 0.0, -0.0, 2.0 ** -140, -2.0 ** -140], (T, B))
    discount = _pick(rng, [1, 0.5, 0, -1, 2], (T, B))
    values = _pick(rng, [1, -1, 0.0, -0.0, 3, -3], (T, B))
    values[rng.random_sample((T, B)) < 0.03] = np.inf
    values[rng.random_sample((T, B)) < 0.03] = -np.inf
    bootstrap = _pick(rng, [1, -1, np.inf, -np.inf, 0.0], (B,))
    done = _done(rng, 0.1, T, B)
    runs = ((0.0, 1.0), (-0.0, 1.0), (0.0, 0.5))
  else:
    raise KeyError(leg)
  return dict(reward=reward.astype(F), done=done, discount=discount.astype(F), values=values.astype(F),
              bootstrap=bootstrap.astype(F), runs=runs)


@functools.lru_cache(maxsize=None)
def returns_want(leg, run, with_discount, with_values):
  """(G, A) of run `run` of the leg - the index into its `runs`: 0.0 and -0.0 are one cache key."""
  x = returns_inputs(leg)
  gamma, lam = x['runs'][run]
  with np.errstate(all='ignore'):
    return returns_ref.returns(x['reward'], x['done'], gamma, x['discount'] if with_discount else None,
                               x['values'] if with_values else None, x['bootstrap'], lam)


# ------------------------------------------------------------------ policy rows (wide_table.hip.h)

ROW_KINDS = ('subnormal', 'one_max', 'two_max', 'negative_zero', 'tiny', 'ordinary')
EDGE_ROWS = {
    # test_visitation_cpu.py's SUB row: c4 = 7 * 2^-140 is subnormal, u * c4 too, num / c4 divides by it
    'subnormal': [2.0 ** -140, 3 * 2.0 ** -140, 0, 2 * 2.0 ** -140, 2.0 ** -140],
    'one_max': [0.75, FLT_MAX, 1.5, 0.5, 1.25],         # c4 = FLT_MAX: a good row
    'two_max': [0.75, FLT_MAX, 1.5, FLT_MAX, 1.25],     # c4 = inf: a bad row
    'negative_zero': [-0.0, 1.0, -0.0, 2.0, 0.5],       # -0.0 is not negative: a good row
    'tiny': [2.0 ** -126, 2.0 ** -130, 0, 2.0 ** -126, 2.0 ** -128],     # c4 is normal, w * q underflows
}


@functools.lru_cache(maxsize=None)
def edge_policy(S):
  """float32 [S, 5]: row s is of kind ROW_KINDS[s % 6] - every kind at six or more states of a
  table of 37, the subnormal row at the reset state - the ordinary ones seeded."""
  rng = np.random.RandomState(500 + S)
  w = rng.uniform(0.5, 2.0, size=(S, 5)).astype(F)
  for s in range(S):
    kind = ROW_KINDS[s % len(ROW_KINDS)]
    if kind != 'ordinary':
      w[s] = np.array(EDGE_ROWS[kind], F)
  return w


@functools.lru_cache(maxsize=None)
def ordinary_policy(S):
  rng = np.random.RandomState(600 + S)
  w = rng.uniform(0.5, 2.0, size=(S, 5)).astype(F)
  w[rng.random_sample((S, 5)) < 0.2] = 0
  w[np.arange(S), rng.randint(0, 5, size=S)] = 1.5           # (no row is all zero)
  return w


def row_kind(s):
  return ROW_KINDS[s % len(ROW_KINDS)]


# ------------------------------------------------------------------ sweeps (k_plan.hip)

SWEEP_SIZES = (37, 257, 1025)
SWEEP_COUNTS = (1, 7, 64)
SWEEP_LEGS = {'underflow': 0.5, 'overflow': 1.0, 'rows': 0.9}        # leg -> gamma
# (leg, S) -> seed; 900 + S where none is named.  The overflow seeds are the first from 1000 with
# which both reductions meet an infinite residual before a NaN one and the greedy q of 64 sweeps
# has three rows or more with a NaN and with several +inf; the underflow seed is the first with
# which a quarter of the residuals, pooled over the sweep counts, is non-zero
# (tests/test_float_edges_cpu.py).
SWEEP_SEEDS = {('overflow', 37): 1002, ('overflow', 257): 1000, ('overflow', 1025): 1001,
               ('underflow', 37): 1000}


@functools.lru_cache(maxsize=None)
def sweep_table(S):
  """tests/test_planning.py's table of S states with discount codes."""
  return table_ref.make_table(7000 + S, 4, 4, 2, 1, S, dcodes=True)


@functools.lru_cache(maxsize=None)
def sweep_inputs(leg, S):
  """-> dict(gamma, reward [S, 5] - the override -, values [S])."""
  rng = np.random.RandomState(SWEEP_SEEDS.get((leg, S), 900 + S))
  tiny = [2.0 ** -120, -2.0 ** -120, 2.0 ** -126, -2.0 ** -126, 2.0 ** -140, -2.0 ** -140]
  subs = [SUB_MIN, -SUB_MIN, SUB_140, -SUB_140, SUB_MAX, -SUB_MAX]
  if leg == 'underflow':
    # half the rewards nothing, the others subnormal or 2^-126; two each of +-2^-120: under
    # gamma 0.5 a reward of 2^-120 keeps every state within seven frames of it normal, and more
    # of them would leave no state of a small table subnormal
    reward = np.where(rng.random_sample((S, 5)) < 0.5, _pick(rng, [0.0, -0.0, np.nan], (S, 5)),
                      _pick(rng, tiny[4:] + subs + [NORM_MIN, -NORM_MIN], (S, 5)))
    reward.reshape(-1)[rng.choice(S * 5, size=4, replace=False)] = tiny[:2] * 2
    values = _pick(rng, subs + [NORM_MIN, -NORM_MIN, 0.0, -0.0], (S,))
  elif leg == 'overflow':
    reward = _pick(rng, [2.0 ** 120, -2.0 ** 120, np.nan], (S, 5), p=[0.5, 0.45, 0.05])
    values = _pick(rng, [2.0 ** 120, -2.0 ** 120, 2.0 ** 100, -2.0 ** 100], (S,))
    # up to an eighth of the states (32 at most) start at +-FLT_MAX and 2^127: one reward of 2^120 more is past FLT_MAX
    few = rng.choice(S, size=min(max(6, S // 8), 32), replace=False)
    values[few] = _pick(rng, [FLT_MAX, -FLT_MAX, P127, -P127], (len(few),))
    values[few[:4]] = [FLT_MAX, -FLT_MAX, P127, -P127]
  elif leg == 'rows':
    # small and ordinary rewards, the edge rows of the policy decide: under gamma 0.9 |q| stays
    # below 0.05 / (1 - 0.9) + 0.5, so that a weight of FLT_MAX times q stays finite
    reward = _pick(rng, tiny + [0.05, -0.05, 0.025, 0.0, -0.0, np.nan], (S, 5))
    values = _pick(rng, subs + [0.5, -0.5, 0.0], (S,))
  else:
    raise KeyError(leg)
  return dict(gamma=SWEEP_LEGS[leg], reward=reward.astype(F), values=values.astype(F))


def sweep_policy(leg, S):
  """The edge rows for the leg that is about them; ordinary weights, a fifth of them exactly 0,
  for the other two (a weight of FLT_MAX would turn their backups into infinities at once)."""
  return edge_policy(S) if leg == 'rows' else ordinary_policy(S)


@functools.lru_cache(maxsize=None)
def sweep_want(leg, S, n, with_policy):
  g, x = sweep_table(S), sweep_inputs(leg, S)
  return plan_ref.sweeps(g.st_next, g.st_reward, g.st_done, g.st_discount, x['gamma'], n,
                         policy=sweep_policy(leg, S) if with_policy else None, values=x['values'],
                         reward_override=x['reward'])


# ------------------------------------------------------------------ sampler (k_policy.hip, k_visit.hip)

SAMPLER_S, SAMPLER_B, SAMPLER_T, SAMPLER_FIRST, SAMPLER_SEED = 37, 257, 11, 3, 0x5eed0123456789ab


@functools.lru_cache(maxsize=None)
def sampler_want():
  """-> (the walker after the rollout, its streams): B environments from the reset state, T frames
  from absolute frame 3, the rows of `edge_policy(37)`."""
  g = sweep_table(SAMPLER_S)
  walker = policy_ref.PolicyWalker(g, SAMPLER_B)
  want = walker.rollout(edge_policy(SAMPLER_S), SAMPLER_T, seed=SAMPLER_SEED, first_frame=SAMPLER_FIRST,
                        reset_first=True)
  return walker, want


@functools.lru_cache(maxsize=None)
def visitation_want():
  g = sweep_table(SAMPLER_S)
  return visit_ref.visitation(g.st_next, g.st_done, edge_policy(SAMPLER_S), SAMPLER_T)


# ------------------------------------------------------------------ learner (k_learn.hip)

LEARN_S, LEARN_B, LEARN_T, LEARN_FIRST, LEARN_WINDOW, LEARN_SEED = 7, 257, 23, 3, 4, 0x1234567890abcdef
ALPHAS = np.array([2.0 ** -140, 2.0 ** -126, 0.5, 1.0, -0.5], F)
GAMMAS = np.array([0.0, 0.5, 2.0, -1.0], F)
EPSILONS = np.array([0.0, 2.0 ** -149, 2.0 ** -24, 1.0], F)


@functools.lru_cache(maxsize=None)
def learner_table():
  """tests/test_learner.py's synthetic table of seven states (its learners' tables fit the LDS)."""
  return table_ref.make_table(LEARN_S * 100 + LEARN_B, 4, 5, 4, 2, LEARN_S, dcodes=True, perf=True)


@functools.lru_cache(maxsize=None)
def learner_inputs():
  """-> dict(q [B, S, 5], alpha, gamma, epsilon [B]): every combination of the three (5 x 4 x 4 =
  80 learners), three times over; a third of the cells of q an edge constant."""
  B, S = LEARN_B, LEARN_S
  rng = np.random.RandomState(77)
  q = rng.uniform(-1, 1, size=(B, S, 5)).astype(F)
  edge = rng.random_sample((B, S, 5)) < 1.0 / 3
  q[edge] = _pick(rng, EDGES, (int(edge.sum()),))
  e = np.arange(B)
  return dict(q=q, alpha=ALPHAS[e % 5], gamma=GAMMAS[(e // 5) % 4], epsilon=EPSILONS[(e // 20) % 4])


@functools.lru_cache(maxsize=None)
def learner_want(rule):
  """-> (the learners after the run, what `learn()` returned - with the recorded streams)."""
  x = learner_inputs()
  L = learn_ref.Learners(learner_table(), LEARN_B, x['q'])
  want = L.learn(LEARN_T, x['alpha'], x['gamma'], x['epsilon'], rule=rule, seed=LEARN_SEED,
                 first_frame=LEARN_FIRST, window=LEARN_WINDOW, record=True)
  return L, want
