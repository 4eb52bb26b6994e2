#!/usr/bin/env python3
"""Actor-critic on the boat race with a NETWORK for a policy: four launches per episode.

`rollout_policy()` samples every action of an episode on the device from a table over the game's
states.  Here that table is not learned directly (examples/reinforce_tabular.py) but computed by
a small MLP with a policy head and a value head, evaluated once per episode on the observation of
every state:

    obs    = game.render_states(obs_dtype=torch.bfloat16)      # [n_states, L, H, W], one render
    p, V   = net(obs)                                          # one forward over n_states rows
    out    = game.rollout_policy(p, frames, ...)               # the whole episode, one launch
    G, A   = discounted_returns(..., values=V[states], ...)    # one backward pass, one launch

`out['states']` names the state each action was sampled from, so `log pi` and the critic's
prediction at every frame are gathers from the n_states rows the network produced - the gradient
flows back through them into the network.  Returns and advantages are episode-aware: nothing
leaks across a `done` inside the rollout, and the value of the state the rollout ended in
bootstraps the last frames.

Same log columns as the other examples.

    python examples/actor_critic_per_state.py --batch 4096 --episodes 30 --csv /tmp/log.csv

A consumer of the engine, not part of it; smoke-tested in tests/test_example_actor_critic.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.episode_log import EpisodeCsvLog  # noqa: E402
from campx_amd.games import boat_race  # noqa: E402
from campx_amd.returns import discounted_returns  # noqa: E402


class ActorCritic(torch.nn.Module):
  """Observation -> (action probabilities [., 5], state value [.])."""

  def __init__(self, n_inputs, hidden=64):
    super().__init__()
    self.body = torch.nn.Sequential(torch.nn.Linear(n_inputs, hidden), torch.nn.Tanh())
    self.actor = torch.nn.Linear(hidden, 5)
    self.critic = torch.nn.Linear(hidden, 1)

  def forward(self, obs):
    h = self.body(obs.flatten(1).float())
    return torch.softmax(self.actor(h), dim=1), self.critic(h).squeeze(1)


def run(batch=4096, episodes=10, frames=100, gamma=0.99, lam=0.95, lr=0.01, value_weight=0.5,
        csv=None, seed=0, device='cuda'):
  torch.manual_seed(seed)
  game = boat_race.build(batch, device)
  game.use_state_table()
  game.its_showtime()
  fused = game.fused
  S, L, H, W = fused.n_states, fused.n_layers, fused.rows, fused.cols
  net = ActorCritic(L * H * W).to(device)
  optim = torch.optim.Adam(net.parameters(), lr=lr)
  # (a table's observations never change, so one render before the loop would do for this game;
  # it is part of the loop here as the per-episode cost it is: one launch into one buffer)
  obs = torch.empty((S, L, H, W), dtype=torch.bfloat16, device=device)
  out = game.rollout_policy_buffers(frames)
  log = EpisodeCsvLog(csv, frames_per_episode=frames) if csv else None
  history = []
  for episode in range(episodes):
    game.render_states(obs_dtype=torch.bfloat16, out=obs)
    p, value = net(obs)                                         # [S, 5], [S]
    game.rollout_policy(p, frames, seed=seed, reset_first=True, out=out)
    states, actions = out['states'].long(), out['actions'].long()
    log_probs = torch.log(p[states, actions])                   # [frames, B]
    v = value[states]                                           # the critic where each frame starts
    # the state the rollout ended in is worth nothing if the episode ended with it
    bootstrap = value.detach()[fused.state.long()] * (1.0 - fused.done.float())
    ret = discounted_returns(out['reward'], out['done'], gamma, discount=out['discount'],
                             values=v, bootstrap=bootstrap, lam=lam)
    adv = ret['advantages']
    adv = (adv - adv.mean()) / (adv.std() + 1e-6)
    actor_loss = -(log_probs * adv).sum(0).mean()
    critic_loss = torch.nn.functional.smooth_l1_loss(v, ret['returns'])
    loss = actor_loss + value_weight * critic_loss
    optim.zero_grad()
    loss.backward()
    optim.step()
    episode_return = torch.nan_to_num(out['reward']).sum(0)
    perf = out['perf'].float().sum(0)
    history.append((float(loss.detach()), float(episode_return.mean()), float(perf.mean())))
    if log:
      log.episode(episode_return, perf, loss=float(loss.detach()))
  if log:
    log.close()
  fused.check_actions()
  return history


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=4096)
  ap.add_argument('--episodes', type=int, default=30)
  ap.add_argument('--frames', type=int, default=100)
  ap.add_argument('--csv', default=None)
  args = ap.parse_args()
  for i, (loss, ret, perf) in enumerate(run(args.batch, args.episodes, args.frames, csv=args.csv)):
    print('ep: {}, L: {:.3f}, R: {:.2f}, P: {:.2f}'.format(i, loss, ret, perf))
