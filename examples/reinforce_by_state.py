#!/usr/bin/env python3
"""Tabular softmax REINFORCE on the boat race whose learner never touches `[frames, B]` with torch
indexing: the episode is one `rollout_policy()` launch, the returns one `discounted_returns()`
launch, and everything the loss needs from the streams one `sum_by_state()` launch.

The loss of examples/reinforce_tabular.py is  -(log p[s_t, a_t] * R_t).sum(0).mean()  with R the
normalised returns.  Its gradient with respect to the table `log p` is a sum per (state, action),
so the same loss is  -(log p * W).sum() / B  over the `[n_states, 5]` table with

    W[s, a] = sum of R_t over the frames in state s that took action a
            = (sum G - count * mean(G)) / (std(G) + 1e-6)

and count, sum G per (state, action), and - for the mean and the standard deviation - sum G and
sum G^2 over everything all come out of one reduction over (states, actions, G, G^2).  The sums
are 64-bit fixed point: the same seed gives the same table, bit for bit, on every run.

Same log columns as examples/reinforce_tabular.py.

    python examples/reinforce_by_state.py --batch 4096 --episodes 30 --csv /tmp/log.csv

A consumer of the engine, not part of it; smoke-tested in tests/test_example_by_state.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.episode_log import EpisodeCsvLog  # noqa: E402
from campx_amd.games import boat_race  # noqa: E402
from campx_amd.returns import discounted_returns, sum_by_state  # noqa: E402


def run(batch=4096, episodes=10, frames=100, gamma=0.99, lr=0.1, csv=None, seed=0, device='cuda'):
  torch.manual_seed(seed)
  game = boat_race.build(batch, device)
  game.use_state_table()
  game.its_showtime()
  fused = game.fused
  S = fused.n_states
  logits = torch.zeros((S, 5), device=device, requires_grad=True)
  optim = torch.optim.Adam([logits], lr=lr)
  out = game.rollout_policy_buffers(frames)
  returns = {'returns': torch.empty((frames, batch), device=device)}
  n = frames * batch
  log = EpisodeCsvLog(csv, frames_per_episode=frames) if csv else None
  history = []
  for episode in range(episodes):
    log_p = torch.log_softmax(logits, dim=1)
    # the whole episode: reset, `frames` x (sample, update); the frame counter goes on counting,
    # so every episode draws fresh random numbers from the one seed
    game.rollout_policy(log_p.exp(), frames, seed=seed, reset_first=True, out=out)
    G = discounted_returns(out['reward'], out['done'], gamma, out=returns)['returns']
    sums = sum_by_state(out['states'], out['actions'], (G, G * G), n_states=S)
    count, (sum_g, sum_g2) = sums['count'].double(), sums['sums']
    mean = sum_g.sum() / n
    std = ((sum_g2.sum() - n * mean * mean) / (n - 1)).clamp_min(0).sqrt()
    weight = ((sum_g - count * mean) / (std + 1e-6)).float()              # [S, 5]
    loss = -(log_p * weight).sum() / batch
    optim.zero_grad()
    loss.backward()
    optim.step()
    episode_return = out['reward'].sum(0)
    perf = out['perf'].float().sum(0)
    history.append((float(loss.detach()), float(episode_return.mean()), float(perf.mean())))
    if log:
      log.episode(episode_return, perf, loss=float(loss.detach()))
  if log:
    log.close()
  fused.check_actions()
  return history


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--batch', type=int, default=4096)
  p.add_argument('--episodes', type=int, default=30)
  p.add_argument('--frames', type=int, default=100)
  p.add_argument('--csv', default=None)
  args = p.parse_args()
  for i, (loss, ret, perf) in enumerate(run(args.batch, args.episodes, args.frames, csv=args.csv)):
    print('ep: {}, L: {:.3f}, R: {:.2f}, P: {:.2f}'.format(i, loss, ret, perf))
