#!/usr/bin/env python3
"""Training from a replay buffer of TRACES: keep trajectories compact, render only what is sampled.

The reference's driver feeds its policy every frame it plays
(`layered_board.view(-1).float()`, examples/reinforce.py:123,149).  A learner that samples
minibatches from a replay buffer needs the observations of the N transitions it draws, not of
every frame: here `rollout_trace()` runs episodes without rendering anything and fills a ring with
their traces (one byte per moving thing, frame and environment - 100 frames of 65 536 boat races
are 6.5 MB instead of 1.15 GB), and `render_frames()` materialises the sampled (frame,
environment) pairs as a dense bf16 minibatch, bit for bit what `rollout()` would have written.

    python examples/replay_minibatches.py        # needs an MI355X
"""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from campx_amd.games import boat_race                     # noqa: E402
from reinforce_batched import Policy                      # noqa: E402  (the reference driver's MLP)


def run(batch=4096, frames=100, episodes=4, minibatches=8, n=2048, device='cuda', seed=0):
  torch.manual_seed(seed)
  game = boat_race.build(batch=batch, device=device)
  game.its_showtime()
  f = game.fused
  row = f.n_layers * f.rows * f.cols
  policy = Policy(row).to(device).to(torch.bfloat16)
  # the ring: `episodes` rollouts' traces and rewards one after the other along the frame axis
  ring = torch.empty((f.n_dyn, episodes * frames, batch), dtype=torch.uint8, device=device)
  reward = torch.empty((episodes * frames, batch), dtype=torch.float32, device=device)
  bufs = game.rollout_trace_buffers(frames)
  for ep in range(episodes):
    actions = torch.randint(0, 5, (frames, batch), dtype=torch.int8, device=device)
    out = game.rollout_trace(actions, reset_first=True, out=bufs)
    ring[:, ep * frames:(ep + 1) * frames].copy_(out['trace'])
    reward[ep * frames:(ep + 1) * frames].copy_(out['reward'])
  obs = torch.empty((n, f.n_layers, f.rows, f.cols), dtype=torch.bfloat16, device=device)
  values = []
  for _ in range(minibatches):
    t = torch.randint(0, episodes * frames, (n,), device=device)
    e = torch.randint(0, batch, (n,), device=device)
    game.render_frames(ring, t, e, out=obs)               # [n, L, H, W] bf16 0.0 / 1.0
    with torch.no_grad():
      logp = policy(obs.view(n, row))
    # (a stand-in for a learner's loss: the sampled transitions' rewards weigh the policy's choices)
    values.append(float((logp.float().exp().max(dim=1).values * reward[t, e]).mean()))
  f.check_actions()
  return dict(game=game, ring=ring, ring_bytes=ring.numel(), obs_bytes=episodes * frames * batch * row,
              minibatch=obs, last_t=t, last_e=e, values=values)


if __name__ == '__main__':
  got = run()
  print('replay ring: %.1f MB of trace for %.1f MB of observations; %d minibatches of %s rendered' % (
      got['ring_bytes'] / 1e6, got['obs_bytes'] / 1e6, len(got['values']), tuple(got['minibatch'].shape)))
