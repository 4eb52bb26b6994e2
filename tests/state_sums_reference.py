"""The rule of `campx_amd.returns.sum_by_state()` (include/campx_hip.h, "Per-state sums of a
rollout's streams") restated in numpy from the header alone: `np.rint` on float64 for the
quantisation (round to nearest even), `np.add.at` on int64 for the additions.  Integer additions
commute, so the accumulators are compared with `array_equal`.  Also the lookup, and the seeded
inputs the tests share."""

import numpy as np


def limits(N):
  """(n2, lim) for N = T * B frames: n2 = ceil(log2(N)), lim = 2^(62 - n2) quanta."""
  n2 = 0
  while (1 << n2) < N:
    n2 += 1
  return n2, 1 << (62 - n2)


def quantise(x, frac_bits, lim):
  """float32 array -> (int64 quanta, bool mask of the clamped)."""
  d = np.asarray(x, dtype=np.float32).astype(np.float64) * np.float64(2.0 ** frac_bits)
  nan = np.isnan(d)
  with np.errstate(invalid='ignore'):
    over = np.abs(d) > np.float64(lim)             # +-Inf included, NaN is False
  safe = np.where(nan | over, 0.0, d)
  q = np.rint(safe).astype(np.int64)
  q = np.where(over & (d > 0), np.int64(lim), q)
  q = np.where(over & (d < 0), np.int64(-lim), q)
  return q, nan | over


def state_sums(states, actions=None, values=(), n_states=1, n_actions=5, frac_bits=24, raw=None,
               N=None):
  """states int32 [T, B], actions int8 [T, B] or None, values: float32 [T, B] each ->
  dict(raw int64 [K + 1, n_states * A], skipped, clamped).  `raw`: accumulators to add onto.
  `N`: the frame count the limit is derived from (default: the streams' own size)."""
  states = np.asarray(states)
  A = 1 if actions is None else int(n_actions)
  K = len(values)
  n2, lim = limits(states.size if N is None else N)
  assert 0 <= frac_bits <= 62 - n2
  s = states.astype(np.int64).ravel()
  a = np.zeros_like(s) if actions is None else np.asarray(actions).astype(np.int64).ravel()
  good = (s >= 0) & (s < n_states) & (a >= 0) & (a < A)
  bins = (s * A + a)[good]
  acc = np.zeros((K + 1, n_states * A), dtype=np.int64) if raw is None else raw.reshape(K + 1, -1).copy()
  np.add.at(acc[0], bins, 1)
  clamped = 0
  for k, x in enumerate(values):
    q, c = quantise(np.asarray(x).ravel()[good], frac_bits, lim)
    np.add.at(acc[1 + k], bins, q)
    clamped += int(c.sum())
  return dict(raw=acc, skipped=int((~good).sum()), clamped=clamped)


def lookup(table, states, actions=None):
  """table float32 [S] or [S, A] -> (float32 [T, B] with 0.0 at the bad indices, their number)."""
  table = np.asarray(table, dtype=np.float32)
  S = table.shape[0]
  A = 1 if actions is None else table.shape[1]
  s = np.asarray(states).astype(np.int64)
  a = np.zeros_like(s) if actions is None else np.asarray(actions).astype(np.int64)
  good = (s >= 0) & (s < S) & (a >= 0) & (a < A)
  i = np.where(good, s * A + a, 0)
  return np.where(good, table.reshape(-1)[i], np.float32(0)).astype(np.float32), int((~good).sum())


def inputs(T, B, S, A, K, dirty=False, seed=0):
  """Seeded streams.  Clean: states uniform over [0, S), actions over [0, A), value stream 0 from
  {-1, -0.25, 0, 0.5, 1, 3} and the others uniform on [-2, 2] (nothing is clamped at frac_bits 24).
  Dirty: 2 % NaN, a few +-Inf and a few values past the limit in every value stream, 2 % of the
  states out of range (negative and >= S), 2 % of the actions 5 or -1 (that is: A or -1)."""
  rng = np.random.RandomState((1000003 * T + 1009 * B + 31 * S + 7 * A + K + seed) % (2 ** 31))
  states = rng.randint(0, S, size=(T, B)).astype(np.int32)
  actions = rng.randint(0, A, size=(T, B)).astype(np.int8)
  values = []
  for k in range(K):
    if k == 0:
      x = rng.choice(np.array([-1, -0.25, 0, 0.5, 1, 3], dtype=np.float32), size=(T, B))
    else:
      x = rng.uniform(-2, 2, size=(T, B)).astype(np.float32)
    values.append(x.astype(np.float32))
  if dirty:
    n = T * B
    few = max(1, n // 200)
    for x in values:
      flat = x.reshape(-1)
      flat[rng.random_sample(n) < 0.02] = np.nan
      flat[rng.randint(0, n, size=few)] = np.inf
      flat[rng.randint(0, n, size=few)] = -np.inf
      flat[rng.randint(0, n, size=few)] = np.float32(3e30)
      flat[rng.randint(0, n, size=few)] = np.float32(-3e30)
    bad = rng.random_sample((T, B)) < 0.02
    states[bad] = rng.choice(np.array([-1, S, S + 7, -2 ** 31, 2 ** 31 - 1], dtype=np.int64),
                             size=int(bad.sum())).astype(np.int32)
    bad = rng.random_sample((T, B)) < 0.02
    actions[bad] = rng.choice(np.array([A, -1], dtype=np.int8), size=int(bad.sum()))
  return dict(states=states, actions=actions, values=values)
