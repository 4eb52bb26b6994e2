#!/usr/bin/env python3
"""Tabular softmax REINFORCE on the boat race: every episode is ONE launch.

The boat race is put on its state table (`Engine.use_state_table()`: 8 states), the policy is
a table of logits `[n_states, 5]`, and an episode of `frames` frames of B environments - sampling
included - is a single `rollout_policy()` call: the kernel walks (state, action) -> state and
draws every action from the row of the state it is in.  The learner gets the rows sampled from
and the actions taken, so `log pi` is one gather: `log p[states, actions]`.

Same returns, loss and log columns as examples/reinforce_batched.py (which runs a network on the
observations, a `play()` per frame).

    python examples/reinforce_tabular.py --batch 4096 --episodes 30 --csv /tmp/log.csv

A consumer of the engine, not part of it; smoke-tested in tests/test_example_tabular.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.episode_log import EpisodeCsvLog  # noqa: E402
from campx_amd.games import boat_race  # noqa: E402


def run(batch=4096, episodes=10, frames=100, gamma=0.99, lr=0.1, csv=None, seed=0, device='cuda'):
  torch.manual_seed(seed)
  game = boat_race.build(batch, device)
  game.use_state_table()
  game.its_showtime()
  fused = game.fused
  logits = torch.zeros((fused.n_states, 5), device=device, requires_grad=True)
  optim = torch.optim.Adam([logits], lr=lr)
  out = game.rollout_policy_buffers(frames)
  log = EpisodeCsvLog(csv, frames_per_episode=frames) if csv else None
  history = []
  for episode in range(episodes):
    p = torch.softmax(logits, dim=1)
    # the whole episode: reset, `frames` x (sample, update); the frame counter goes on counting,
    # so every episode draws fresh random numbers from the one seed
    game.rollout_policy(p, frames, seed=seed, reset_first=True, out=out)
    log_probs = torch.log(p[out['states'].long(), out['actions'].long()])      # [frames, B]
    returns, running = [], torch.zeros(batch, device=device)
    for r in reversed(list(out['reward'])):
      running = r + gamma * running
      returns.append(running)
    returns = torch.stack(returns[::-1])
    returns = (returns - returns.mean()) / (returns.std() + 1e-6)
    loss = -(log_probs * returns).sum(0).mean()
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
