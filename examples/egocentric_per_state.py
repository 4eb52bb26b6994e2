#!/usr/bin/env python3
"""Actor-critic on the 16x16 maze with a network that sees only a 5x5 window round the walker.

examples/actor_critic_per_state.py with partial observability: the network is fed not the board
but what the agent sees - five by five cells centred on it, walls where the window hangs over the
edge.  The window round the agent is a function of the state, so the network's output is still a
table over the game's states, and the closed loop costs what it cost before:

    obs    = game.render_state_windows(Window(5, 5, 'A', pad='#'))   # [n_states, L, 5, 5], one render
    p, V   = net(obs)                                                # one forward over n_states rows
    out    = game.rollout_policy(p, frames, ...)                     # the whole episode, one launch
    G, A   = discounted_returns(..., values=V[states], ...)          # one backward pass, one launch

The render writes `L * 25` elements per state where `render_states()` writes `L * 256`.  Two states
whose windows are the same get the same policy row: that is all "partially observable" means here.

Same log columns as the other examples.

    python examples/egocentric_per_state.py --batch 4096 --episodes 30 --csv /tmp/log.csv

A consumer of the engine, not part of it; smoke-tested in tests/test_example_egocentric.py.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from campx_amd.episode_log import EpisodeCsvLog  # noqa: E402
from campx_amd.games import maze  # noqa: E402
from campx_amd.returns import discounted_returns  # noqa: E402
from campx_amd.windows import Window  # noqa: E402

WINDOW = Window(5, 5, 'A', pad='#')        # the maze's walker and its wall


class ActorCritic(torch.nn.Module):
  """Window -> (action probabilities [., 5], state value [.])."""

  def __init__(self, n_inputs, hidden=64):
    super().__init__()
    self.body = torch.nn.Sequential(torch.nn.Linear(n_inputs, hidden), torch.nn.Tanh())
    self.actor = torch.nn.Linear(hidden, 5)
    self.critic = torch.nn.Linear(hidden, 1)

  def forward(self, obs):
    h = self.body(obs.flatten(1).float())
    return torch.softmax(self.actor(h), dim=1), self.critic(h).squeeze(1)


def run(batch=4096, episodes=10, frames=100, gamma=0.99, lam=0.95, lr=0.01, value_weight=0.5,
        csv=None, seed=0, device='cuda', window=WINDOW, keep=None):
  """`keep`: a dict that receives 'game', 'net', 'obs' and the last 'policy' (for the test)."""
  torch.manual_seed(seed)
  game = maze.build(16, 16, batch=batch, device=device)
  game.its_showtime()
  fused = game.fused
  S, L = fused.n_states, fused.n_layers
  net = ActorCritic(L * window.height * window.width).to(device)
  optim = torch.optim.Adam(net.parameters(), lr=lr)
  obs = torch.empty((S, L, window.height, window.width), dtype=torch.bfloat16, device=device)
  out = game.rollout_policy_buffers(frames)
  log = EpisodeCsvLog(csv, frames_per_episode=frames) if csv else None
  history = []
  for episode in range(episodes):
    game.render_state_windows(window, out=obs)                  # one launch into one buffer
    p, value = net(obs)                                         # [S, 5], [S]
    game.rollout_policy(p, frames, seed=seed, reset_first=True, out=out)
    states, actions = out['states'].long(), out['actions'].long()
    log_probs = torch.log(p[states, actions])                   # [frames, B]
    v = value[states]
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
    perf = (out['perf'].float().sum(0) if out.get('perf') is not None
            else torch.zeros_like(episode_return))
    history.append((float(loss.detach()), float(episode_return.mean()), float(perf.mean())))
    if log:
      log.episode(episode_return, perf, loss=float(loss.detach()))
    if keep is not None:
      keep.update(game=game, net=net, obs=obs, policy=p.detach())
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
