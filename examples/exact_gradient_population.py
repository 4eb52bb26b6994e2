#!/usr/bin/env python3
"""P tabular softmax learners on the boat race, each with its own learning rate, each climbing the
EXACT policy gradient - examples/exact_policy_gradient.py for a population, with ONE launch per
half of the gradient per step whatever P is:

    grad J_m = sum_s d_gamma,m(s) sum_a grad pi_m(a | s) q_m(s, a)

    q_m         every member's action values: one `evaluate_population(want_q=True)`
    d_gamma,m   every member's discounted visitation of an episode from the reset state: one
                `visit_population(restart=False, want_frames=True)`, 'per_frame' `[frames + 1, P, S]`

A sweep of learning rates is the plainest population; population-based training, an evolution
strategy that selects on exact returns or a set of seeds take the same two calls.  Each step prints
every member's exact return v_m[0].  (Both halves are cut after `frames` frames: gamma^frames of
the weight is left out.)

    python examples/exact_gradient_population.py --members 8 --steps 40 --lr-min 0.25 --lr-max 8

A consumer of the engine, not part of it; smoke-tested in
tests/test_example_exact_gradient_population.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402


def run(members=8, steps=40, frames=64, gamma=0.9, lr_min=0.25, lr_max=8.0, device='cuda', log=None):
  game = boat_race.build(1, device)
  game.use_state_table()
  game.its_showtime()
  S, P = game.fused.n_states, members
  # learning rates spaced evenly in the logarithm, the smallest first
  ramp = torch.linspace(0.0, 1.0, P, dtype=torch.float64, device=device) if P > 1 else \
      torch.zeros(1, dtype=torch.float64, device=device)
  lr = lr_min * (lr_max / lr_min) ** ramp
  theta = torch.zeros((P, S, 5), dtype=torch.float64, device=device)
  weight = gamma ** torch.arange(frames, dtype=torch.float64, device=device)
  sweep_out = game.population_sweep_buffers(P, frames, want_q=True)
  visit_out = game.visit_population_buffers(P, frames, want_frames=True)
  history = []
  for step in range(steps + 1):
    pi = torch.softmax(theta, dim=2)
    policies = pi.float().contiguous()
    value = game.evaluate_population(policies, gamma, frames, want_q=True, out=sweep_out)
    history.append(value['values'][:, 0].tolist())
    if log:
      log('step {:3d}   '.format(step) + '  '.join('{:8.4f}'.format(v) for v in history[-1]))
    if step == steps:
      break
    visit = game.visit_population(policies, frames, restart=False, want_frames=True, out=visit_out)
    d_t = visit['per_frame'][:frames].double() / float(visit['unit'])          # [frames, P, S]
    d_gamma = (weight[:, None, None] * d_t).sum(0)                             # [P, S]
    q = value['q'].double()
    v = (pi * q).sum(2, keepdim=True)
    theta += lr[:, None, None] * d_gamma[:, :, None] * pi * (q - v)
  game.fused.check_actions()
  return {'values': history, 'lr': lr.tolist(), 'policies': torch.softmax(theta, dim=2).cpu()}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--members', type=int, default=8)
  p.add_argument('--steps', type=int, default=40)
  p.add_argument('--frames', type=int, default=64)
  p.add_argument('--gamma', type=float, default=0.9)
  p.add_argument('--lr-min', type=float, default=0.25)
  p.add_argument('--lr-max', type=float, default=8.0)
  args = p.parse_args()
  res = run(args.members, args.steps, args.frames, args.gamma, args.lr_min, args.lr_max,
            log=print)
  print('learning rates ' + '  '.join('{:8.4f}'.format(x) for x in res['lr']))
