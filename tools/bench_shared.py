#!/usr/bin/env python3
"""`learn_shared()` measured: T frames of online Q-learning for P shared learners of n actors each
in ONE launch, beside what a user pays for the same frames today.

T = 1 000, B = 65 536.  Rows: the boat race and the 16x16 maze on their state tables, n = 1, 16, 256
and 1 024 actors per learner (P = B / n learners), each path forced where the plan allows it
(1 = tables and accumulators in LDS, 2 = in global memory).  Two baselines in the same process:
  * a torch restatement of the same T frames on the same device and game: per frame an
    epsilon-greedy action from `q[member]` (gather, argmax, rand), one `play()`, the TD errors, and
    their mean per (learner, state, action) through two `index_put_(accumulate=True)` - floats
    added in arrival order, so it does not repeat; it is the comparator for the time, not for the
    bits (tests/test_shared_learner.py has those);
  * `learn_tabular()` at the same B and T - a table per environment - for information only.

GATE: the launch is no slower than the torch loop, every row (exit status 1 otherwise).  A row that
fails or outlasts its time limit ends the run (exit status 2): nothing more is started on the
device, and what was collected is written.

A fresh process per row; warm-up first, event pairs, the median of 15 launches and of 3 torch loops.

    python tools/bench_shared.py [out.txt]      # default: profiles/r19_shared.txt
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
ACTORS = (1, 16, 256, 1024)
ROWS = tuple((name, n, path) for name in ('boat_race', 'maze16') for n in ACTORS for path in (1, 2))
GATE_MISSED = 3            # exit status of a row that ran and missed the gate
SKIPPED = 4                # ... of a row whose forced path the plan refuses
ROW_SECONDS = 240          # a row builds one game and runs 36 launches and 3 050 torch frames: seconds
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


def torch_frames(game, q, n, frames):
  """`frames` frames of synchronous epsilon-greedy Q-learning on `q` [P, S, 5], n environments per
  learner, in torch ops and one `play()` per frame."""
  import torch
  f = game.fused
  P, S = q.shape[0], q.shape[1]
  member = torch.arange(B, device='cuda') // n
  flat = q.view(-1)
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  ones = torch.ones((B,), device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    greedy = q[member, s].argmax(1)
    explore = torch.rand((B,), device='cuda') < EPSILON
    a = torch.where(explore, torch.randint(0, 5, (B,), device='cuda'), greedy)
    _, reward, discount = game.play(a.to(torch.int8))
    r = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    b = q[member, f.state.long()].max(1).values
    target = r + (GAMMA * discount) * b            # (a frame that ends the episode reports discount 0)
    at = (member * S + s) * 5 + a
    delta = target - flat[at]
    total = torch.zeros((P * S * 5,), device='cuda').index_put_((at,), delta, accumulate=True)
    count = torch.zeros((P * S * 5,), device='cuda').index_put_((at,), ones, accumulate=True)
    flat.add_(ALPHA * total / count.clamp_(min=1.0))


def row(name, n, path):
  """One row, in this process: prints it; exit status GATE_MISSED when the gate is missed."""
  import torch
  from campx_amd import _hip
  game = build(name)
  f = game.fused
  S, P = f.n_states, B // n
  plan = (ctypes.c_int64 * 6)()
  if _hip.lib.campx_wide_shared_plan(S, int(f.has_perf), B, P, _hip.config_get('wide_lds_max'), path,
                                     plan) != 0:
    print('%-10s S=%-4d n=%-4d P=%-5d  path %d does not apply (not one learner fits the LDS)'
          % (name, S, n, P, path))
    return SKIPPED
  q = torch.zeros((P, S, 5), device='cuda')
  hyper = [torch.full((P,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  out = game.shared_learner_buffers(P, T, 100, path)
  launch = lambda: game.learn_shared(T, q, *hyper, seed=1, window=100, out=out, path=path)
  for _ in range(WARM):
    launch()
  torch.cuda.synchronize()
  ours = timed_ms(launch, RUNS)
  q.zero_()
  torch_frames(game, q, n, LOOP_WARM_FRAMES)
  torch.cuda.synchronize()
  loop = timed_ms(lambda: torch_frames(game, q, n, T), LOOP_RUNS)
  del q, out
  # for information: a table per environment, the same B and T
  q_each = torch.zeros((B, S, 5), device='cuda')
  each = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  bufs = game.learner_buffers(T, 100)
  alone = lambda: game.learn_tabular(T, q_each, *each, seed=1, window=100, out=bufs)
  for _ in range(WARM):
    alone()
  torch.cuda.synchronize()
  tabular = timed_ms(alone, RUNS)
  ok = ours <= loop
  print('%-10s S=%-4d n=%-4d P=%-5d  path %d (G %d, %d threads, %6d B LDS, entries %s)   learn_shared() %.3f ms '
        '= %.2f us / frame   torch loop %.1f ms = %.1f us / frame (x%.0f)   learn_tabular() %.3f ms%s'
        % (name, S, n, P, plan[0], plan[1], plan[2], plan[3], 'in LDS' if plan[4] else 'through L1 / L2',
           ours, ours * 1000 / T, loop, loop * 1000 / T, loop / ours, tabular, '' if ok else '   GATE MISSED'))
  return 0 if ok else GATE_MISSED


def main():
  if len(sys.argv) == 5 and sys.argv[1] == '--row':
    return row(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
  import torch
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'r19_shared.txt')
  lines = ['# tools/bench_shared.py: B = %d, T = %d; a process per row; event pairs, the median of %d '
           'launches after %d warm-up launches and of %d torch loops after %d warm-up frames; %s'
           % (B, T, RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, torch.cuda.get_device_name(0))]
  ok, broke = True, False
  for name, n, forced in ROWS:
    try:
      done = subprocess.run([sys.executable, os.path.abspath(__file__), '--row', name, str(n), str(forced)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            timeout=ROW_SECONDS)
    except subprocess.TimeoutExpired as late:
      lines.append('%s n %d path %d  ROW TIMED OUT after %d s\n%s'
                   % (name, n, forced, ROW_SECONDS, (late.stderr or '')[-2000:]))
      ok, broke = False, True
      break                      # nothing more is started on the device after a failure
    lines.append(done.stdout.rstrip('\n'))
    if done.returncode not in (0, GATE_MISSED, SKIPPED):
      lines.append('  ROW FAILED (exit status %d)\n%s' % (done.returncode, done.stderr.rstrip('\n')))
      ok, broke = False, True
      break                      # nothing more is started on the device after a failure
    if done.returncode == GATE_MISSED:
      ok = False
    print(lines[-1], flush=True)
  if broke:
    lines.append('the run ended at the row above; the rows after it were not started')
  lines.append('gate (learn_shared() no slower than the torch loop of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 2 if broke else (0 if ok else 1)


if __name__ == '__main__':
  sys.exit(main())
