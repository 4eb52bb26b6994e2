#!/usr/bin/env python3
"""A tabular softmax policy on the boat race trained by the EXACT policy gradient: no rollout, no
sampling noise, no baseline to tune.  The game's state table is its complete deterministic MDP, so
both halves of the policy-gradient theorem can be computed from it:

    grad J = sum_s d_gamma(s) sum_a grad pi(a | s) q(s, a)

    d_gamma = sum_t gamma^t d_t     the discounted state visitation of an episode from the reset
                                    state: `state_visitation(restart=False, want_frames=True)`
    q                               the policy's action values: `evaluate_policy()`

For a softmax policy pi = softmax(theta) the inner sum is pi(b | s) * (q(s, b) - v(s)) for logit
theta[s, b].  Each iteration prints v[0], the policy's exact value at the reset state, beside the
optimum that `value_iteration()` finds; plain gradient ascent climbs to it.  (Both the visitation
and the values are cut after `frames` frames: gamma^frames of the weight is left out.)

    python examples/exact_policy_gradient.py --iterations 60 --frames 64 --gamma 0.9

A consumer of the engine, not part of it; smoke-tested in tests/test_example_exact_gradient.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402


def run(iterations=60, frames=64, gamma=0.9, lr=4.0, device='cuda', log=None):
  game = boat_race.build(1, device)
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  optimum = float(game.value_iteration(gamma, frames, want_q=False)['values'][0])
  theta = torch.zeros((S, 5), dtype=torch.float64, device=device)
  weight = gamma ** torch.arange(frames, dtype=torch.float64, device=device)
  visit_out = game.visitation_buffers(frames, want_frames=True)
  sweep_out = game.sweep_buffers(frames, greedy=False)
  history = []
  for it in range(iterations + 1):
    pi = torch.softmax(theta, dim=1)
    policy = pi.float().contiguous()
    value = game.evaluate_policy(policy, gamma, frames, out=sweep_out)
    history.append(float(value['values'][0]))
    if log:
      log('iteration {:3d}   v[0] {:9.5f}   optimum {:9.5f}'.format(it, history[-1], optimum))
    if it == iterations:
      break
    visit = game.state_visitation(policy, frames, restart=False, want_frames=True, out=visit_out)
    d_t = visit['per_frame'][:frames].double() / float(visit['unit'])          # [frames, S]
    d_gamma = (weight[:, None] * d_t).sum(0)
    q = value['q'].double()
    v = (pi * q).sum(1, keepdim=True)
    theta += lr * d_gamma[:, None] * pi * (q - v)
  game.fused.check_actions()
  return {'values': history, 'optimum': optimum, 'policy': torch.softmax(theta, dim=1).cpu()}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--iterations', type=int, default=60)
  p.add_argument('--frames', type=int, default=64)
  p.add_argument('--gamma', type=float, default=0.9)
  p.add_argument('--lr', type=float, default=4.0)
  args = p.parse_args()
  res = run(args.iterations, args.frames, args.gamma, args.lr, log=print)
  print('last v[0] {:.5f} of {:.5f}'.format(res['values'][-1], res['optimum']))
