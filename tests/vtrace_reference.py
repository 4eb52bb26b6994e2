"""The rule of `campx_amd.returns.vtrace_returns()` (include/campx_hip.h, csrc/k_vtrace.hip)
restated in numpy float32: one ufunc per operation - each rounds to float32 on its own, as the
kernel's `__fmul_rn` / `__fadd_rn` / `__fsub_rn` / `__fdiv_rn` do - and `np.where` for the selects.
Results are compared as uint32 views (`same_bits`, from tests/returns_reference.py, whose seeded
`inputs` the tests here share).  Also the seeded ratio streams and tables."""

import numpy as np

from returns_reference import F, inputs, same_bits  # noqa: F401  (re-exported)

RATIOS = np.array([0, 0.25, 0.5, 1, 1.5, 4], dtype=F)


def table_ratio(target, behaviour, states, actions):
  """-> (w0 f32 [T, B], the number of frames out of range): the table mode's ratio stream.  A
  frame out of range has w0 = 0 and reads neither table."""
  target, behaviour = np.asarray(target, dtype=F), np.asarray(behaviour, dtype=F)
  Nt, A = target.shape
  Nb = behaviour.shape[0]
  assert behaviour.shape[1] == A and Nb % Nt == 0
  s, a = np.asarray(states).astype(np.int64), np.asarray(actions).astype(np.int64)
  ok = (s >= 0) & (s < Nb) & (a >= 0) & (a < A)
  s0, a0 = np.where(ok, s, 0), np.where(ok, a, 0)
  with np.errstate(all='ignore'):
    w0 = np.divide(target[s0 % Nt, a0], behaviour[s0, a0])
  assert w0.dtype == F
  return np.where(ok, w0, F(0)).astype(F), int((~ok).sum())


def vtrace(reward, done, gamma, values, ratio, discount=None, bootstrap=None, lam=1.0, rho_bar=1.0,
           c_bar=1.0, pg_rho_bar=None, variant=None):
  """reward / values / ratio f32 [T, B], done uint8 [T, B], discount f32 [T, B] or None, bootstrap
  f32 [B] or None -> dict(vs, advantages, D, delta), each f32 [T, B].

  `variant` is for the tests of the tests: 'clip_after_product' clips cs * (c * lam) instead of w,
  'carry_across_done' ignores `done` in the recursion of D.  Neither is the rule."""
  reward = np.asarray(reward, dtype=F)
  T, B = reward.shape
  gamma, lam = F(gamma), F(lam)
  rho_bar, c_bar = F(rho_bar), F(c_bar)
  pg_rho_bar = rho_bar if pg_rho_bar is None else F(pg_rho_bar)
  boot = np.zeros(B, dtype=F) if bootstrap is None else np.asarray(bootstrap, dtype=F)
  vs, adv = np.empty((T, B), dtype=F), np.empty((T, B), dtype=F)
  Ds, deltas = np.empty((T, B), dtype=F), np.empty((T, B), dtype=F)
  D_next, v_next, vs_next = np.zeros(B, dtype=F), boot, boot
  with np.errstate(all='ignore'):
    for t in range(T - 1, -1, -1):
      over = np.asarray(done[t]) != 0
      r = np.where(np.isnan(reward[t]), F(0), reward[t]).astype(F)
      c = (np.multiply(gamma, np.asarray(discount[t], dtype=F)) if discount is not None
           else np.full(B, gamma, dtype=F))
      w0 = np.asarray(ratio[t], dtype=F)
      w = np.where(np.greater(w0, F(0)), w0, F(0)).astype(F)
      rho = np.where(np.less(w, rho_bar), w, rho_bar).astype(F)
      cs = np.where(np.less(w, c_bar), w, c_bar).astype(F)
      rpg = np.where(np.less(w, pg_rho_bar), w, pg_rho_bar).astype(F)
      v = np.asarray(values[t], dtype=F)
      q = np.where(over, r, np.add(r, np.multiply(c, v_next)))
      delta = np.multiply(rho, np.subtract(q, v))
      if variant == 'clip_after_product':
        k = np.multiply(np.multiply(c, lam), w)
        k = np.where(np.less(k, c_bar), k, c_bar).astype(F)
      else:
        k = np.multiply(np.multiply(c, lam), cs)
      carried = np.add(delta, np.multiply(k, D_next))
      D = carried if variant == 'carry_across_done' else np.where(over, delta, carried)
      assert c.dtype == F and delta.dtype == F and k.dtype == F and D.dtype == F
      vs[t] = np.add(v, D)
      qs = np.where(over, r, np.add(r, np.multiply(c, vs_next)))
      adv[t] = np.multiply(rpg, np.subtract(qs, v))
      Ds[t], deltas[t] = D, delta
      D_next, v_next, vs_next = D, v, vs[t]
  return dict(vs=vs, advantages=adv, D=Ds, delta=deltas)


def ratios(T, B, seed=0):
  """A seeded ratio stream from {0, 0.25, 0.5, 1, 1.5, 4}, with about 3 % each of NaN, -1 and
  +inf: by the rule none of them reaches the outputs as a NaN."""
  rng = np.random.RandomState(77000 + 1000 * T + B + seed)
  w = rng.choice(RATIOS, size=(T, B))
  u = rng.random_sample((T, B))
  w[u < 0.03] = np.nan
  w[(u >= 0.03) & (u < 0.06)] = -1
  w[(u >= 0.06) & (u < 0.09)] = np.inf
  return w.astype(F)


def tables(Nt, Nb, A=5, seed=0):
  """Seeded strictly positive tables: target f32 [Nt, A], behaviour f32 [Nb, A], rows that sum to
  about one.  A few quotients are above every bar the tests use, a few far below."""
  rng = np.random.RandomState(88000 + 7 * Nt + Nb + seed)
  def rows(n):
    x = rng.uniform(0.02, 1.0, size=(n, A)) ** 3
    return (x / x.sum(axis=1, keepdims=True)).astype(F)
  target, behaviour = rows(Nt), rows(Nb)
  assert (target > 0).all() and (behaviour > 0).all()
  return target, behaviour


def ids(T, B, Nb, A=5, seed=0):
  """Seeded in-range index streams: states int32 [T, B] in [0, Nb), actions int8 [T, B] in [0, A)."""
  rng = np.random.RandomState(99000 + 1000 * T + B + Nb + seed)
  return (rng.randint(0, Nb, size=(T, B)).astype(np.int32), rng.randint(0, A, size=(T, B)).astype(np.int8))
