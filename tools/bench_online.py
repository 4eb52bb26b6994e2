#!/usr/bin/env python3
"""`learn_tabular()` measured: T frames of online Q-learning for B independent learners in ONE
launch, beside what a user pays for the same frames today.

T = 1 000, B = 65 536.  Rows: the boat race on its state table with both paths forced (1 = the
learners' tables in LDS, 2 = through L1 / L2) and the 16x16 maze on the global path (its 159 states
do not fit path 1).  The comparator of every row is a torch restatement of the same T frames on the
same device and the same game: per frame an epsilon-greedy action from `q` (gather, argmax, rand),
one `play()`, and the update through gather / `scatter_` on `q` - a handful of torch ops and one
launch of the engine per frame.  It draws torch's random numbers, not the kernel's: it is the
comparator for the time, not for the bits (tests/test_learner.py has those).

GATE: the launch is no slower than the torch loop, every row (exit status 1 otherwise).  A row that
fails or outlasts its time limit ends the run (exit status 2): nothing more is started on the
device, and what was collected is written.

A fresh process per row; warm-up first, event pairs, the median of 15 launches and of 3 torch loops.

    python tools/bench_online.py [out.txt]      # default: profiles/r15_online.txt
"""
import ctypes
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 50     # torch loops of T frames
ROWS = (('boat_race', 1), ('boat_race', 2), ('maze16', 2))
GATE_MISSED = 3            # exit status of a row that ran and missed the gate
ROW_SECONDS = 240          # a row builds one game and runs 18 launches and 3 050 torch frames: seconds
ALPHA, GAMMA, EPSILON = 0.1, 0.9, 0.1


def build(name):
  from campx_amd.games import boat_race, maze
  if name == 'boat_race':
    game = boat_race.build(B, 'cuda')
    game.use_state_table()
  else:
    game = maze.build(16, 16, batch=B, device='cuda')
  game.its_showtime()
  game.fused.validate_actions = False
  return game


def timed_ms(fn, runs):
  import torch
  times = []
  for _ in range(runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1))
  return statistics.median(times)


def torch_frames(game, q, frames):
  """`frames` frames of epsilon-greedy Q-learning on `q` [B, S, 5], a learner per environment, in
  torch ops and one `play()` per frame."""
  import torch
  f = game.fused
  lanes = torch.arange(B, device='cuda')
  flat = q.view(B, -1)
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    greedy = q[lanes, s].argmax(1)
    explore = torch.rand((B,), device='cuda') < EPSILON
    a = torch.where(explore, torch.randint(0, 5, (B,), device='cuda'), greedy)
    _, reward, discount = game.play(a.to(torch.int8))
    r = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    b = q[lanes, f.state.long()].max(1).values
    target = r + (GAMMA * discount) * b            # (a frame that ends the episode reports discount 0)
    at = (s * 5 + a)[:, None]
    old = flat.gather(1, at)
    flat.scatter_(1, at, old + ALPHA * (target[:, None] - old))


def row(name, path):
  """One row, in this process: prints it; exit status GATE_MISSED when the gate is missed."""
  import torch
  from campx_amd import _hip
  game = build(name)
  f = game.fused
  S = f.n_states
  plan = (ctypes.c_int64 * 4)()
  _hip.check(_hip.lib.campx_wide_learn_plan(S, int(f.has_perf), B, _hip.config_get('wide_lds_max'),
                                            path, plan), 'campx_wide_learn_plan')
  q = torch.zeros((B, S, 5), device='cuda')
  hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  out = game.learner_buffers(T, 100)
  launch = lambda: game.learn_tabular(T, q, *hyper, seed=1, window=100, out=out, path=path)
  for _ in range(WARM):
    launch()
  torch.cuda.synchronize()
  ours = timed_ms(launch, RUNS)
  q.zero_()
  torch_frames(game, q, LOOP_WARM_FRAMES)
  torch.cuda.synchronize()
  loop = timed_ms(lambda: torch_frames(game, q, T), LOOP_RUNS)
  ok = ours <= loop
  print('%-10s S=%-4d B=%d T=%d  path %d (%6d B LDS, entries %s)   learn_tabular() %.3f ms = %.2f us / frame   '
        'torch loop %.1f ms = %.1f us / frame (x%.0f)%s'
        % (name, S, B, T, plan[0], plan[1], 'in LDS' if plan[3] else 'through L1 / L2', ours,
           ours * 1000 / T, loop, loop * 1000 / T, loop / ours, '' if ok else '   GATE MISSED'))
  return 0 if ok else GATE_MISSED


def main():
  if len(sys.argv) == 4 and sys.argv[1] == '--row':
    return row(sys.argv[2], int(sys.argv[3]))
  import torch
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'r15_online.txt')
  lines = ['# tools/bench_online.py: a process per row; event pairs, the median of %d launches after %d '
           'warm-up launches and of %d torch loops after %d warm-up frames; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, torch.cuda.get_device_name(0))]
  ok, broke = True, False
  for name, forced in ROWS:
    try:
      done = subprocess.run([sys.executable, os.path.abspath(__file__), '--row', name, str(forced)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            timeout=ROW_SECONDS)
    except subprocess.TimeoutExpired as late:
      lines.append('%s path %d  ROW TIMED OUT after %d s\n%s'
                   % (name, forced, ROW_SECONDS, (late.stderr or '')[-2000:]))
      ok, broke = False, True
      break                      # nothing more is started on the device after a failure
    lines.append(done.stdout.rstrip('\n'))
    if done.returncode not in (0, GATE_MISSED):
      lines.append('  ROW FAILED (exit status %d)\n%s' % (done.returncode, done.stderr.rstrip('\n')))
      ok, broke = False, True
      break                      # nothing more is started on the device after a failure
    if done.returncode == GATE_MISSED:
      ok = False
  if broke:
    lines.append('the run ended at the row above; the rows after it were not started')
  lines.append('gate (learn_tabular() no slower than the torch loop of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 2 if broke else (0 if ok else 1)


if __name__ == '__main__':
  sys.exit(main())
