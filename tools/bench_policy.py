#!/usr/bin/env python3
"""Closed-loop rollouts measured: `rollout_policy()` beside the two things it stands between.

Boat race on its state table at B = 4 096 and 65 536, the 16x16 maze at B = 65 536, T = 100:

  * `rollout_policy()`: the episode, sampling included, in one launch;
  * `rollout_trace()` of the same game on the actions that produced: the same walk with the
    actions loaded instead of sampled - the floor the sampling adds to (reported, not gated);
  * a `capture_play(100, policy=...)` graph replay whose policy is `weights[state]` ->
    `torch.multinomial`: the existing way to close the loop on the device.

GATE: `rollout_policy()` is faster than the graph replay at all three points (exit status 1
otherwise; a ratio below 2 is flagged - a hundred kernel nodes against one launch).

Settled clocks (warm-up launches first), event pairs, median of 25 runs.

    python tools/bench_policy.py [out.txt]        # default: profiles/r08_policy.txt
"""
import functools
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)
import torch  # noqa: E402

RUNS, WARM, T = 25, 10, 100
median = functools.partial(benchlib.median_ms, runs=RUNS, warm=WARM)


def point(name, B, lines):
  game = benchlib.state_table_game(name, B)
  f = game.fused
  gen = torch.Generator(device='cuda').manual_seed(1)
  weights = torch.rand((f.n_states, 5), generator=gen, device='cuda') + 0.05
  bufs = f.rollout_policy_buffers(T)
  closed = median(lambda: f.rollout_policy(weights, T, seed=1, reset_first=True, out=bufs))
  acts = bufs['actions'].contiguous()
  lean = f.rollout_trace_buffers(T)
  floor = median(lambda: f.rollout_trace(acts, reset_first=True, out=lean))
  lean_ns = f.rollout_policy_buffers(T, want_states=False)
  no_states = median(lambda: f.rollout_policy(weights, T, seed=1, reset_first=True, out=lean_ns,
                                                 want_states=False))

  def act(observation, t):       # the frame starts from row 0 when the last one ended the episode
    row = torch.where(f.done.bool(), torch.zeros_like(f.state), f.state).long()
    return torch.multinomial(weights[row], 1).squeeze(1)
  f.reset()
  graph = game.capture_play(T, policy=act)
  replay = median(graph.replay)
  lines.append('%-10s S=%-4d B=%-6d T=%d  rollout_policy() %.4f ms (without states %.4f)   '
               'rollout_trace() on its actions %.4f ms (x%.2f)   capture_play graph replay %.4f ms (x%.1f)'
               % (name, f.n_states, B, T, closed, no_states, floor, closed / floor, replay, replay / closed))
  del graph, bufs, lean, lean_ns, game
  torch.cuda.empty_cache()
  return closed, replay


def main():
  path = benchlib.out_path(sys.argv[1:], 'r08_policy.txt')
  lines = ['# tools/bench_policy.py: median of %d event pairs after %d warm-up runs, %s'
           % (RUNS, WARM, torch.cuda.get_device_name(0))]
  ok = True
  for name, B in (('boat_race', 4096), ('boat_race', 65536), ('maze16', 65536)):
    closed, replay = point(name, B, lines)
    if closed >= replay:
      ok = False
      lines.append('  GATE MISSED: rollout_policy() is not faster than the graph replay')
    elif replay / closed < 2.0:
      lines.append('  (ratio below 2: look at a kernel trace before trusting this point)')
  lines.append('gate (rollout_policy() faster than the graph replay at every point): %s'
               % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
