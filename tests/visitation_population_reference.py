"""Exact state visitation of a POPULATION of policies on a state table, restated in numpy from the
rule in include/campx_hip.h ("The same for a population of policies, in one launch" under the
visitation rule): the checker of tests/test_visit_population.py.  No torch, no HIP, no code shared
with campx_amd/.

Everything is vectorised over the flat rows r = m * S + s of all P members: one bisection over
P * S rows, one split per frame, one scatter into the flat `[P * S]` mass with every target shifted
by its member's m * S - so that member m can only be what `visitation_reference.visitation()` gives
for `policies[m]` from member m's start if the flat arithmetic keeps the members apart.  Results
are time-major where there is a frame axis: `finished [frames, P]`, `per_frame [frames + 1, P, S]`.
"""

import numpy as np

from visitation_reference import MAX_FRAMES, N_ACTIONS, UNIT, counts_of, cumulative_counts, quantise, split


def start_rows(P, S, start=None):
  """-> int64 [P, S]: None - one environment in state 0 of every member; `[S]` - shared by all;
  `[P, S]` - per member.  Float probabilities are quantised row by row."""
  if start is None:
    d = np.zeros((P, S), np.int64)
    d[:, 0] = UNIT
    return d
  d = np.asarray(start)
  assert d.shape in ((S,), (P, S))
  if d.dtype != np.int64:
    d = np.stack([quantise(row) for row in d.reshape(-1, S)]).reshape(d.shape)
  d = np.broadcast_to(d, (P, S)).copy()
  assert (d >= 0).all() and int(d.sum(axis=1).max()) <= UNIT
  return d


def visitation(next_state, done, policies, frames, start=None, restart=True, cumulative=None):
  """-> dict(visits int64 [P, S, 5], finished int64 [frames, P], final int64 [P, S], per_frame
  int64 [frames + 1, P, S], counts int32 [P, S, 5], bad_rows int - summed over the members).
  `cumulative`: what `cumulative_counts(policies.reshape(P * S, 5))` gave, for a caller that runs
  the same policies several times and spares the bisection."""
  nxt = np.asarray(next_state, np.int64)
  ends = np.asarray(done) != 0
  w = np.asarray(policies, np.float32)
  P, S = w.shape[0], len(nxt)
  assert w.shape == (P, S, N_ACTIONS) and 1 <= frames <= MAX_FRAMES
  # a row per (member, state)
  N, bad = cumulative if cumulative is not None else cumulative_counts(w.reshape(P * S, N_ACTIONS))
  base = np.repeat(np.arange(P, dtype=np.int64) * S, S)             # row r's member's row 0
  member = base // S
  target = base[:, None] + np.tile(nxt, (P, 1))                     # [P * S, 5], flat
  over_rows = np.tile(ends, (P, 1))
  d = start_rows(P, S, start).reshape(P * S)
  visits = np.zeros((P * S, N_ACTIONS), np.int64)
  finished = np.zeros((frames, P), np.int64)
  per_frame = np.zeros((frames + 1, P * S), np.int64)
  per_frame[0] = d
  for t in range(frames):
    x = split(d, N)
    visits += x
    np.add.at(finished[t], np.broadcast_to(member[:, None], x.shape)[over_rows], x[over_rows])
    new = np.zeros(P * S, np.int64)
    np.add.at(new, target[~over_rows], x[~over_rows])
    if restart:
      new[::S] += finished[t]
    d = new
    per_frame[t + 1] = d
  return dict(visits=visits.reshape(P, S, N_ACTIONS), finished=finished, final=d.reshape(P, S),
              per_frame=per_frame.reshape(frames + 1, P, S),
              counts=counts_of(N).reshape(P, S, N_ACTIONS), bad_rows=int(bad.sum()))
