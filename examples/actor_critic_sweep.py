#!/usr/bin/env python3
"""A sweep of one-step actor-critic learners on the boat race (`learn_actor_critic()`): how fast,
as a function of the ACTOR's step size, does a softmax policy find what the reward pays for - round
and round past the same two arrows - and what happens to the hidden performance meanwhile?

Every environment is its own learner with its own preferences and its own critic; learner
i * seeds + k is seed k of `alphas[i]`, every other hyper-parameter shared.  The run is ONE launch of
`frames` frames - what examples/actor_critic_per_state.py does as a rollout, a returns pass, a
`sum_by_state()` and a torch step per update, for one learner.  The learning curves are the
launch's window sums of reward AND of hidden performance; no [T, B] stream is written.

What the learnt policies are worth is not estimated from those samples: the first `evaluate` of each
setting's learners go through `evaluate_population(softmax_weights(prefs))` - exact policy
evaluation of exactly the probabilities the learners sampled from - once under the game's reward
and once under its hidden performance.

Per setting the script prints one line: reward and hidden performance per frame in the first and
the last window, and the exact values of the start state.

    python examples/actor_critic_sweep.py --frames 4000 --window 500

A consumer of the engine, not part of it; tested in tests/test_example_actor_critic_sweep.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402
from campx_amd.returns import softmax_weights  # noqa: E402

ALPHAS = tuple(round(0.01 * 2 ** i, 2) for i in range(8))             # 0.01 .. 1.28


def run(alphas=ALPHAS, seeds=64, frames=4000, window=500, alpha_critic=0.1, gamma=0.9, seed=0,
        evaluate=4, sweeps=200, device='cuda'):
  """-> dict: 'prefs' [B, S, 5], 'values' [B, S]; per setting [len(alphas), W]: 'reward' and
  'perf', the window sums averaged over the setting's learners and divided by the window's frames;
  'fitness' and 'hidden' [len(alphas), evaluate]: the exact value of the start state of the
  setting's first `evaluate` learners under the reward and under the hidden performance."""
  B = len(alphas) * seeds
  game = boat_race.build(B, device)
  game.use_state_table()
  game.its_showtime()
  alpha_actor = torch.tensor([a for a in alphas for _ in range(seeds)], dtype=torch.float32,
                             device=device)
  res = game.learn_actor_critic(frames, alpha_actor=alpha_actor, alpha_critic=alpha_critic,
                                gamma=gamma, seed=seed, reset_first=True, window=window)
  W = res['reward_sum'].shape[0]
  cells = (W, len(alphas), seeds)
  in_window = torch.full((W,), float(window), device=device)
  in_window[-1] = frames - (W - 1) * window
  # exact fitness: the probabilities the learners sampled from, evaluated on the game's table
  picked = res['prefs'].view(len(alphas), seeds, -1, 5)[:, :evaluate].reshape(-1, res['prefs'].shape[1], 5)
  policies = softmax_weights(picked.contiguous())
  fitness = game.evaluate_population(policies, gamma, sweeps)['values'][:, 0].clone()
  perf = game.fused.table_arrays()['perf'].float()
  hidden = game.evaluate_population(policies, gamma, sweeps, reward=perf)['values'][:, 0].clone()
  game.fused.check_actions()
  return {'prefs': res['prefs'], 'values': res['values'], 'alpha_actor': alpha_actor,
          'reward': (res['reward_sum'].view(cells).mean(2) / in_window[:, None]).t(),
          'perf': (res['perf_sum'].float().view(cells).mean(2) / in_window[:, None]).t(),
          'fitness': fitness.view(len(alphas), -1), 'hidden': hidden.view(len(alphas), -1)}


def lines(alphas, r):
  return ['alpha_actor {:5.2f}  reward/frame {:6.3f} -> {:6.3f}  performance/frame {:6.3f} -> {:6.3f}  '
          'exact value {:7.3f}  exact hidden value {:7.3f}'.format(
              a, float(r['reward'][i, 0]), float(r['reward'][i, -1]), float(r['perf'][i, 0]),
              float(r['perf'][i, -1]), float(r['fitness'][i].mean()), float(r['hidden'][i].mean()))
          for i, a in enumerate(alphas)]


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--seeds', type=int, default=64)
  p.add_argument('--frames', type=int, default=4000)
  p.add_argument('--window', type=int, default=500)
  p.add_argument('--alpha-critic', type=float, default=0.1)
  p.add_argument('--gamma', type=float, default=0.9)
  args = p.parse_args()
  r = run(seeds=args.seeds, frames=args.frames, window=args.window, alpha_critic=args.alpha_critic,
          gamma=args.gamma)
  for line in lines(ALPHAS, {k: v.cpu() for k, v in r.items()}):
    print(line)
