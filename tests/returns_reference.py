"""The rule of `campx_amd.returns.discounted_returns()` (include/campx_hip.h, csrc/k_returns.hip)
restated in numpy float32: one ufunc per operation - each rounds to float32 on its own, as the
kernel's `__fmul_rn` / `__fadd_rn` / `__fsub_rn` do - and `np.where` for the selects.  Results are
compared as uint32 views.  Also the seeded inputs the tests share."""

import numpy as np

F = np.float32


def returns(reward, done, gamma, discount=None, values=None, bootstrap=None, lam=1.0):
  """reward f32 [T, B], done uint8 [T, B], discount / values f32 [T, B] or None, bootstrap f32 [B]
  or None -> (G f32 [T, B], A f32 [T, B] or None)."""
  reward = np.asarray(reward, dtype=F)
  T, B = reward.shape
  gamma, lam = F(gamma), F(lam)
  boot = np.zeros(B, dtype=F) if bootstrap is None else np.asarray(bootstrap, dtype=F)
  G = np.empty((T, B), dtype=F)
  A = np.empty((T, B), dtype=F) if values is not None else None
  G_next, v_next, A_next = boot, boot, np.zeros(B, dtype=F)
  for t in range(T - 1, -1, -1):
    over = np.asarray(done[t]) != 0
    r = np.where(np.isnan(reward[t]), F(0), reward[t]).astype(F)
    c = np.multiply(gamma, np.asarray(discount[t], dtype=F)) if discount is not None else np.full(B, gamma, dtype=F)
    assert c.dtype == F
    G[t] = np.where(over, r, np.add(r, np.multiply(c, G_next)))
    G_next = G[t]
    if values is not None:
      v = np.asarray(values[t], dtype=F)
      q = np.where(over, r, np.add(r, np.multiply(c, v_next)))
      delta = np.subtract(q, v)
      A[t] = np.where(over, delta, np.add(delta, np.multiply(np.multiply(c, lam), A_next)))
      A_next, v_next = A[t], v
  return G, A


def same_bits(a, b):
  a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def inputs(T, B, seed=0):
  """Seeded streams chosen so that no subnormal arises (the smallest magnitudes are a reward of
  0.25 behind T <= 100 factors of 0.99 * 0.5): rewards from {-1, -0.25, 0, 0.5, 1, 3} with 5 %
  NaN, discounts from {1, 0.5, 0}, values and bootstrap uniform in [-2, 2], done with probability
  0.1 - and, where the batch has room, columns forced all-done, never-done, done only at t = 0 and
  done only at t = T - 1.  (Subnormals, signed zeros, overflow and NaN: tests/float_edges.py.)"""
  rng = np.random.RandomState(1000 * T + B + seed)
  reward = rng.choice(np.array([-1, -0.25, 0, 0.5, 1, 3], dtype=F), size=(T, B))
  reward[rng.random_sample((T, B)) < 0.05] = np.nan
  discount = rng.choice(np.array([1, 0.5, 0], dtype=F), size=(T, B))
  values = rng.uniform(-2, 2, size=(T, B)).astype(F)
  bootstrap = rng.uniform(-2, 2, size=(B,)).astype(F)
  done = (rng.random_sample((T, B)) < 0.1).astype(np.uint8)
  forced = {}
  if B >= 4:
    cols = rng.choice(B, size=4, replace=False)
    done[:, cols[0]] = 1
    done[:, cols[1]] = 0
    done[:, cols[2]] = 0
    done[0, cols[2]] = 1
    done[:, cols[3]] = 0
    done[T - 1, cols[3]] = 1
    forced = dict(zip(('all', 'never', 'first', 'last'), (int(c) for c in cols)))
  return dict(reward=reward.astype(F), done=done, discount=discount, values=values,
              bootstrap=bootstrap, forced=forced)
