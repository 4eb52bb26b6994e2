#!/usr/bin/env python3
"""Synchronous advantage actor-critic (A2C) on the boat race: P learners, each ONE softmax policy
and ONE critic fed by n parallel actors, a sweep of the actor's step size across the learners - all
in one launch per call.

`learn_actor_critic_shared()` runs the P x n environments for T frames: within a frame every actor
of a learner samples from the same policy and bootstraps from the same critic, the one-step errors
are summed per (state, action) in fixed point, and every visited state moves once, by the step size
times the mean update of its visitors - the step size does not depend on n, and a run repeats bit
for bit.

Per learner the script prints the learning curve - reward per actor and frame of every window, from
the call's window sums - and the exact discounted return from the start state of the policy it
learnt, `evaluate_population(softmax_weights(prefs))`, beside the uniform policy's.

    python examples/a2c_parallel_actors.py --learners 4 --actors 64 --frames 2000 --window 500

A consumer of the engine, not part of it; tested in tests/test_example_a2c_parallel_actors.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd import returns  # noqa: E402
from campx_amd.games import boat_race  # noqa: E402


def step_sizes(learners, lowest=0.01, highest=0.5):
  """`learners` actor step sizes, evenly spaced in the logarithm."""
  if learners == 1:
    return [highest]
  ratio = (highest / lowest) ** (1.0 / (learners - 1))
  return [lowest * ratio ** m for m in range(learners)]


def run(learners=4, actors=64, frames=2000, window=500, alpha_critic=0.2, gamma=0.9, seed=0,
        sweeps=400, device='cuda'):
  """-> dict for `learners` learners of `actors` actors: 'alpha_actor' [P]; 'prefs' [P, S, 5] and
  'values' [P, S]; 'curve' [W, P], reward per actor and frame of every window; 'perf' [W, P], the
  hidden performance likewise; 'return' [P], the exact return of each learnt policy from state 0;
  'uniform_return', that of the uniform policy; 'clamped' [P]."""
  P, n = learners, actors
  game = boat_race.build(P * n, device)
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  alpha_actor = torch.tensor(step_sizes(P), dtype=torch.float32, device=device)
  prefs = torch.zeros((P, S, 5), device=device)
  values = torch.zeros((P, S), device=device)
  res = game.learn_actor_critic_shared(frames, prefs, values, alpha_actor=alpha_actor,
                                       alpha_critic=alpha_critic, gamma=gamma, seed=seed,
                                       reset_first=True, window=window)
  W = res['reward_sum'].shape[0]
  in_window = torch.full((W, 1), float(window), device=device)
  in_window[-1] = frames - (W - 1) * window                  # the last window may be short
  policies = torch.cat([returns.softmax_weights(prefs), torch.ones((1, S, 5), device=device)])
  exact = game.evaluate_population(policies, gamma, sweeps)['values'][:, 0]
  game.fused.check_actions()
  return {'alpha_actor': alpha_actor, 'prefs': prefs, 'values': values,
          'curve': res['reward_sum'].view(W, P, n).mean(2) / in_window,
          'perf': res['perf_sum'].float().view(W, P, n).mean(2) / in_window,
          'return': exact[:P], 'uniform_return': exact[P], 'clamped': res['clamped']}


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--learners', type=int, default=4)
  p.add_argument('--actors', type=int, default=64)
  p.add_argument('--frames', type=int, default=2000)
  p.add_argument('--window', type=int, default=500)
  p.add_argument('--alpha-critic', type=float, default=0.2)
  p.add_argument('--gamma', type=float, default=0.9)
  args = p.parse_args()
  r = run(learners=args.learners, actors=args.actors, frames=args.frames, window=args.window,
          alpha_critic=args.alpha_critic, gamma=args.gamma)
  print('uniform policy\'s return: {:.3f}'.format(float(r['uniform_return'])))
  print('learner  alpha_actor  return   reward per actor and frame, window by window')
  for m in range(args.learners):
    print('{:7d}  {:11.4f}  {:6.3f}   {}'.format(
        m, float(r['alpha_actor'][m]), float(r['return'][m]),
        '  '.join('{:6.3f}'.format(float(c)) for c in r['curve'][:, m])))
