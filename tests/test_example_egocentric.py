"""Smoke test of examples/egocentric_per_state.py: a network that sees only a 5 x 5 window round
the walker, evaluated once per episode on `render_state_windows()` of every state."""

import math
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_egocentric_example_runs_and_equal_windows_get_equal_policy_rows():
  sys.path.insert(0, os.path.join(REPO, 'examples'))
  import egocentric_per_state
  keep = {}
  history = egocentric_per_state.run(batch=257, episodes=3, frames=20, keep=keep)
  assert len(history) == 3
  assert all(math.isfinite(x) for row in history for x in row)      # loss, return, performance
  game, net, obs = keep['game'], keep['net'], keep['obs']
  S = game.fused.n_states
  assert obs.shape == (S, game.fused.n_layers, 5, 5) and obs.dtype == torch.bfloat16
  # a window policy is a per-state table: states whose windows are bit-identical get
  # bit-identical rows from the network
  with torch.no_grad():
    p, _ = net(obs)
  flat = obs.view(torch.int16).reshape(S, -1)
  _, inverse, counts = torch.unique(flat, dim=0, return_inverse=True, return_counts=True)
  assert int(counts.max()) > 1, 'no two states of the maze share a 5 x 5 window'
  assert len(counts) > 1
  first = torch.zeros(len(counts), dtype=torch.long, device=obs.device)
  first.scatter_(0, inverse.flip(0), torch.arange(S, device=obs.device).flip(0))   # lowest state per window
  assert torch.equal(p.view(torch.int32), p[first[inverse]].view(torch.int32))
  assert keep['policy'].shape == p.shape
