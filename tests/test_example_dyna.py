"""examples/dyna_q_maze.py at a small batch: three settings of planning x 4 seeds = 12 learners, 130
frames in windows of 50 (the last one short).  The learners' tables and models bit for bit against
tests/dyna_learner_reference.py under the same arguments, the curves - [settings, windows] -
against the reference's window sums, and one printed line per setting."""

import os
import sys

import numpy as np
import pytest

import dyna_learner_reference as dyna_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANNINGS, SEEDS, FRAMES, WINDOW = (0, 5, 50), 4, 130, 50


@pytest.mark.gpu
def test_the_sweep_learns_what_the_reference_learns_and_prints_a_line_per_setting():
  from campx_amd import tabulate
  from campx_amd.games import maze
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import dyna_q_maze
  got = dyna_q_maze.run(PLANNINGS, SEEDS, FRAMES, WINDOW, seed=3)
  B, W = len(PLANNINGS) * SEEDS, 3
  planning = np.repeat(np.array(PLANNINGS, np.int32), SEEDS)
  assert np.array_equal(got['planning'].cpu().numpy(), planning)
  L = dyna_ref.DynaLearners(tabulate.trace(maze.build(16, 16)), B)
  want = L.learn_dyna(FRAMES, planning, 0.5, 0.95, 0.3, 'q', seed=3, reset_first=True, window=WINDOW)
  q = got['q'].cpu().numpy()
  assert q.shape == (B, 159, 5) and np.array_equal(q.view(np.uint32), L.q.view(np.uint32))
  assert np.array_equal(got['model']['n_seen'].cpu().numpy(), L.n_seen)
  assert np.array_equal(got['model']['seen'].cpu().numpy(), L.seen)
  for k, sums in (('episodes', want['episodes']), ('reward', want['reward_sum'])):
    assert tuple(got[k].shape) == (len(PLANNINGS), W), k
    curve = sums.reshape(W, len(PLANNINGS), SEEDS).astype(np.float64).sum(2)
    assert np.allclose(got[k].cpu().numpy(), curve.T, rtol=0, atol=1e-3), k
  # the learners of one setting differ by seed alone, and planning matters
  assert not np.array_equal(L.q[0], L.q[1]) and not np.array_equal(L.q[:SEEDS], L.q[SEEDS:2 * SEEDS])
  printed = dyna_q_maze.lines(PLANNINGS, got['episodes'].cpu())
  assert len(printed) == 3
  for n, line in zip(PLANNINGS, printed):
    assert line.startswith('planning {:4d}  episodes per window '.format(n)) and 'total' in line
