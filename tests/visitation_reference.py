"""Exact state visitation of a policy on a state table, restated in numpy from the rule in
include/campx_hip.h ("Exact state visitation of a policy on the state table"): the checker of
tests/test_visitation.py.  No torch, no HIP, no code shared with campx_amd/.

A table is two `[S, 5]` arrays, `next_state` and `done`, each entry as a rollout reports the frame
that takes action a in state s (the `st_next`, `st_done` of a `tabulate.TracedGame` or of
`wide_table_reference.make_table()`).  Mass is an int64 in units of 2^-38: one environment is
`UNIT`.  Every addition below is an integer addition.
"""

import numpy as np

N_ACTIONS = 5
FRAC_BITS = 38
UNIT = 1 << FRAC_BITS
WORDS = 1 << 24                 # the sampler's 24-bit values u
MAX_FRAMES = 1 << 20
F = np.float32


def thresholds(policy):
  """-> (c float32 [S, 5], bad bool [S]): the sampler's thresholds of every row - c0 = w0,
  c1 = c0 + w1 ... in float32, in that order - and its test of the row; a bad row's thresholds are
  {-1, -1, -1, -1, 0}."""
  w = np.asarray(policy, F)
  c = np.empty(w.shape, F)
  with np.errstate(all='ignore'):
    c[:, 0] = w[:, 0]
    for k in range(1, N_ACTIONS):
      c[:, k] = (c[:, k - 1] + w[:, k]).astype(F)
    total = c[:, 4]
    good = (w >= 0).all(axis=1) & (total > 0) & (total < np.inf)
  c[~good] = np.array([-1, -1, -1, -1, 0], F)
  return c, ~good


def cumulative_counts(policy):
  """-> (N int64 [S, 5], bad bool [S]).  N[s, i], i < 4: the smallest u in 0 .. 2^24 with
  float32(u) * 2^-24 * c4 >= c_i (2^24 if there is none), found by 25 bisection steps; N[s, 4] =
  2^24."""
  c, bad = thresholds(policy)
  S = len(c)
  N = np.full((S, N_ACTIONS), WORDS, np.int64)
  for i in range(4):
    lo = np.zeros(S, np.int64)
    hi = np.full(S, WORDS, np.int64)
    for _ in range(25):
      mid = (lo + hi) >> 1
      with np.errstate(all='ignore'):
        u = (mid.astype(F) * F(2.0 ** -24)).astype(F)
        r = (u * c[:, 4]).astype(F)
        ok = r >= c[:, i]
      hi = np.where(ok, mid, hi)
      lo = np.where(ok, lo, mid + 1)
    assert (lo >= hi).all()
    N[:, i] = hi
  return N, bad


def counts_of(N):
  """counts[s, a] = N[s, a] - N[s, a - 1], int32 [S, 5]; every row sums to 2^24."""
  N = np.asarray(N, np.int64)
  out = N.copy()
  out[:, 1:] -= N[:, :-1]
  return out.astype(np.int32)


def split(m, N):
  """The mass m int64 [S] (0 <= m < 2^62) of every state over its five actions -> x int64 [S, 5]:
  y_i = (m >> 24) * N_i + (((m & 0xffffff) * N_i) >> 24), x_a = y_a - y_{a-1}."""
  m = np.asarray(m, np.int64)
  N = np.asarray(N, np.int64)
  assert ((m >= 0) & (m < (1 << 62))).all()
  y = (m >> 24)[:, None] * N + (((m & 0xffffff)[:, None] * N) >> 24)
  x = y.copy()
  x[:, 1:] -= y[:, :-1]
  return x


def start_vector(S, start=None):
  if start is None:
    d = np.zeros(S, np.int64)
    d[0] = UNIT
    return d
  d = np.asarray(start)
  assert d.dtype == np.int64 and d.shape == (S,) and (d >= 0).all() and int(d.sum()) <= UNIT
  return d.copy()


def quantise(probs):
  """Probabilities float [S] -> int64 [S] units that total exactly 2^38: every entry rounded down,
  the remainder given to the largest entry (the first of several).  What
  `WideGame.state_visitation()` does with a float `start`; not part of the C rule."""
  p = np.asarray(probs, np.float64)
  d = np.floor(p * float(UNIT)).astype(np.int64)
  d[int(np.argmax(p))] += UNIT - int(d.sum())
  return d


def visitation(next_state, done, policy, frames, start=None, restart=True):
  """-> dict(visits int64 [S, 5], finished int64 [frames], final int64 [S], per_frame int64
  [frames + 1, S], counts int32 [S, 5], bad_rows int)."""
  nxt = np.asarray(next_state, np.int64)
  ends = np.asarray(done) != 0
  S = len(nxt)
  assert 1 <= frames <= MAX_FRAMES
  N, bad = cumulative_counts(policy)
  d = start_vector(S, start)
  visits = np.zeros((S, N_ACTIONS), np.int64)
  finished = np.zeros(frames, np.int64)
  per_frame = np.zeros((frames + 1, S), np.int64)
  per_frame[0] = d
  for t in range(frames):
    x = split(d, N)
    visits += x
    over = int(x[ends].sum())
    finished[t] = over
    new = np.zeros(S, np.int64)
    np.add.at(new, nxt[~ends], x[~ends])
    if restart:
      new[0] += over
    d = new
    per_frame[t + 1] = d
  return dict(visits=visits, finished=finished, final=d, per_frame=per_frame,
              counts=counts_of(N), bad_rows=int(bad.sum()))
