#!/usr/bin/env python3
"""A tabular IMPALA learner on the boat race: ONE learner fed by P stale actors, every call of the
loop one launch.

The learner owns `logits[n_states, 5]` and a critic `V[n_states]`.  The actors are P snapshots of
its own policy, member m being m updates old: the batch is split into P blocks and block m plays
snapshot m.  The data is therefore off-policy for all members but the first, and V-trace corrects
it.  An iteration is

    rollout_population()     the P actors' episodes, sampling included: one launch
    table_lookup()           V at the state each frame starts in: one launch
    vtrace_returns()         table mode - the ratio pi / mu is looked up and divided in the kernel
                             from the learner's [S, 5] and the snapshots' [P * S, 5]: one launch
    sum_by_state()           per (state, action): count, sum adv, and per state sum (vs - V) -
                             the actor's and the critic's gradient: one launch
    a step on logits and V, the snapshots shifted by one

and the learner's EXACT return from the start state - `evaluate_policy()` on the game's table, no
sampling - is printed per iteration.

    python examples/impala_tabular.py --batch 4096 --members 4 --iterations 30

A consumer of the engine, not part of it; smoke-tested in tests/test_example_impala.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.games import boat_race  # noqa: E402
from campx_amd.returns import sum_by_state, table_lookup, vtrace_returns  # noqa: E402


def run(batch=4096, members=4, iterations=10, frames=100, gamma=0.99, lam=0.95, lr=0.5, critic_lr=0.5,
        sweeps=200, seed=0, device='cuda', report=None):
  """-> per iteration, the learner's exact return from the start state (before the update)."""
  P = members
  game = boat_race.build(batch, device)
  game.use_state_table()
  game.its_showtime()
  f = game.fused
  S = f.n_states
  logits = torch.zeros((S, 5), device=device)
  V = torch.zeros((S,), device=device)
  snapshots = torch.softmax(logits, dim=1).repeat(P, 1, 1).contiguous()        # [P, S, 5]
  out = game.rollout_population_buffers(frames)
  targets = {'vs': torch.empty((frames, batch), device=device),
             'advantages': torch.empty((frames, batch), device=device)}
  bad = torch.zeros((1,), dtype=torch.int64, device=device)
  N = frames * batch
  history = []
  for it in range(iterations):
    p = torch.softmax(logits, dim=1)
    exact = game.evaluate_policy(p, gamma, sweeps, want_q=False)['values'][0]
    history.append(float(exact))
    if report:
      report(it, history[-1])
    snapshots = torch.roll(snapshots, 1, 0)
    snapshots[0] = p                                 # member m now plays the policy of m updates ago
    game.rollout_population(snapshots, frames, seed=seed, reset_first=True, out=out)
    values = table_lookup(V.repeat(P), out['states'])            # the flat row is member * S + state
    # V of the state each environment is left in (ignored where the last frame ended an episode)
    bootstrap = table_lookup(V, f.state.view(1, batch)).view(batch)
    vtrace_returns(out['reward'], out['done'], gamma, values, target=p, behaviour=snapshots.view(-1, 5),
                   states=out['states'], actions=out['actions'], discount=out['discount'],
                   bootstrap=bootstrap, lam=lam, bad_count=bad, out=targets)
    sums = sum_by_state(out['states'], out['actions'], (targets['advantages'], targets['vs'] - values),
                        n_states=P * S)
    sum_adv, sum_err = (x.view(P, S, 5).sum(0) for x in sums['sums'])          # the members share one table
    # d/dlogits of sum_t adv_t * log pi(a_t | s_t): per state, sum adv of (s, a) - pi(a | s) * sum adv of s
    grad = (sum_adv - p.double() * sum_adv.sum(1, keepdim=True)) / N
    logits += lr * (grad * S).float()
    count = sums['count'].view(P, S, 5).sum((0, 2)).clamp_min(1).double()
    V += critic_lr * (sum_err.sum(1) / count).float()
  game.fused.check_actions()
  assert int(bad) == 0
  return history


def main(argv=None):
  p = argparse.ArgumentParser()
  p.add_argument('--batch', type=int, default=4096)
  p.add_argument('--members', type=int, default=4)
  p.add_argument('--iterations', type=int, default=30)
  p.add_argument('--frames', type=int, default=100)
  p.add_argument('--sweeps', type=int, default=200)
  args = p.parse_args(argv)
  return run(args.batch, args.members, args.iterations, args.frames, sweeps=args.sweeps,
             report=lambda it, value: print('it: {}, exact return of the learner: {:.4f}'.format(it, value)))


if __name__ == '__main__':
  main()
