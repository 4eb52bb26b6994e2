#!/usr/bin/env python3
"""P tabular REINFORCE learners on the boat race in ONE process and one launch per step of the
loop: a sweep of learning rates over the same seed schedule.

The batch is split into P equal blocks of n = batch / P environments; learner m owns block m and
row m of `logits[P, n_states, 5]`.  An iteration is

    rollout_population()      every learner's episode, sampling included: one launch
    discounted_returns()      the returns of all of them: one launch
    sum_by_state(n_states=P * S)   count, sum G and sum G^2 per (learner, state, action): one launch
    one optimiser step on logits[P, S, 5] with a learning rate per learner

'states' of a population rollout is the flat row `member * n_states + state`, so the reduction
that examples/reinforce_by_state.py runs over `[n_states, 5]` runs here over `[P * n_states, 5]`
unchanged; the returns are normalised per learner from the same sums.  Plain gradient ascent with
each learner's own step size (a learning rate per row of one tensor is one multiply).

    python examples/reinforce_population.py --batch 4096 --episodes 30

A consumer of the engine, not part of it; smoke-tested in tests/test_example_population.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402
from campx_amd.returns import discounted_returns, sum_by_state  # noqa: E402


def run(batch=4096, lrs=(0.03, 0.1, 0.3, 1.0), episodes=10, frames=100, gamma=0.99, seed=0,
        device='cuda'):
  """-> per episode, the list of each learner's mean episode return."""
  P = len(lrs)
  n = batch // P
  game = boat_race.build(batch, device)
  game.use_state_table()
  game.its_showtime()
  S = game.fused.n_states
  logits = torch.zeros((P, S, 5), device=device, requires_grad=True)
  lr = torch.tensor(lrs, dtype=torch.float32, device=device).view(P, 1, 1)
  out = game.rollout_population_buffers(frames)
  returns = {'returns': torch.empty((frames, batch), device=device)}
  N = frames * n                                   # frames of one learner
  history = []
  for episode in range(episodes):
    log_p = torch.log_softmax(logits, dim=2)
    # every learner's whole episode; the frame counter goes on counting, so every episode draws
    # fresh random numbers from the one seed - the same schedule for every learner
    game.rollout_population(log_p.exp(), frames, seed=seed, reset_first=True, out=out)
    G = discounted_returns(out['reward'], out['done'], gamma, out=returns)['returns']
    sums = sum_by_state(out['states'], out['actions'], (G, G * G), n_states=P * S)
    count = sums['count'].double().view(P, S, 5)
    sum_g, sum_g2 = (x.view(P, S, 5) for x in sums['sums'])
    mean = sum_g.sum((1, 2), keepdim=True) / N                                  # per learner
    std = ((sum_g2.sum((1, 2), keepdim=True) - N * mean * mean) / (N - 1)).clamp_min(0).sqrt()
    weight = ((sum_g - count * mean) / (std + 1e-6)).float()                    # [P, S, 5]
    loss = -(log_p * weight).sum() / n
    grad, = torch.autograd.grad(loss, logits)
    with torch.no_grad():
      logits -= lr * grad
    history.append(out['reward'].sum(0).view(P, n).mean(1).tolist())
  game.fused.check_actions()
  return history


if __name__ == '__main__':
  p = argparse.ArgumentParser()
  p.add_argument('--batch', type=int, default=4096)
  p.add_argument('--episodes', type=int, default=30)
  p.add_argument('--frames', type=int, default=100)
  p.add_argument('--lrs', type=float, nargs='+', default=[0.03, 0.1, 0.3, 1.0])
  args = p.parse_args()
  for i, means in enumerate(run(args.batch, tuple(args.lrs), args.episodes, args.frames)):
    print('ep: {}, R per learner: {}'.format(i, ', '.join(
        'lr {:g}: {:.2f}'.format(lr, r) for lr, r in zip(args.lrs, means))))
