#!/usr/bin/env python3
"""`rollout_population()` measured: P policies over one batch in ONE launch, beside what a user
pays for the same today.

Boat race on its state table and the 16x16 maze, T = 100, B = 65 536, P = 1, 16, 256, 65 536
(n = B / P = 65 536 ... 1 environments per member).  Beside each row, in the same process and the
same loop (the three alternate, so that a drifting clock meets them alike):

  (a) one `rollout_policy()` at the same B and T: the same walk under one table;
  (b) one `rollout_policy()` on a game of n environments, times P: P launches on P small games,
      which is what a population costs without this call.

GATE: population time <= (b) for every P >= 16 (exit status 1 otherwise): the one-launch claim is
the feature.  A row that fails or outlasts its time limit ends the run (exit status 2): nothing
more is started on the device, and what was collected is written.  The ratio to (a) is reported, with the path each row took (1 = table and thresholds
in LDS, 2 = through L1 / L2) and the members one workgroup stages, and is not gated.

A fresh process per row; settled clocks (warm-up launches first), event pairs, median of 25.

    python tools/bench_population.py [out.txt]      # default: profiles/r14_population.txt
"""
import ctypes
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RUNS, WARM, T, B = 25, 10, 100, 65536
MEMBERS = (1, 16, 256, 65536)
GAMES = ('boat_race', 'maze16')
GATE_MISSED = 3            # exit status of a row that ran and missed the gate
ROW_SECONDS = 300          # a row builds two games and times 35 rounds of three launches: seconds


def build(name, batch):
  from campx_amd.games import boat_race, maze
  if name == 'boat_race':
    game = boat_race.build(batch, 'cuda')
    game.use_state_table()
  else:
    game = maze.build(16, 16, batch=batch, device='cuda')
  game.its_showtime()
  game.fused.validate_actions = False
  return game


def medians_ms(fns):
  """The median time of each of `fns`, run in turn: every round times each once."""
  import torch
  for _ in range(WARM):
    for fn in fns:
      fn()
  torch.cuda.synchronize()
  times = [[] for _ in fns]
  for _ in range(RUNS):
    for i, fn in enumerate(fns):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      times[i].append(e0.elapsed_time(e1))
  return [statistics.median(t) for t in times]


def row(name, P):
  """One row, in this process: prints it; exit status GATE_MISSED when the gate is missed."""
  import torch
  from campx_amd import _hip
  big, small = build(name, B).fused, build(name, B // P).fused
  S = big.n_states
  gen = torch.Generator(device='cuda').manual_seed(1)
  policies = torch.rand((P, S, 5), generator=gen, device='cuda') + 0.05
  one = policies[0].contiguous()
  plan = (ctypes.c_int64 * 4)()
  _hip.check(_hip.lib.campx_wide_population_plan(S, int(big.has_perf), B, P,
                                                 _hip.config_get('wide_lds_max'), 0, plan),
             'campx_wide_population_plan')
  pop_bufs, big_bufs = big.rollout_population_buffers(T), big.rollout_policy_buffers(T)
  small_bufs = small.rollout_policy_buffers(T)
  pop, same_b, one_member = medians_ms([
      lambda: big.rollout_population(policies, T, seed=1, reset_first=True, out=pop_bufs),
      lambda: big.rollout_policy(one, T, seed=1, reset_first=True, out=big_bufs),
      lambda: small.rollout_policy(one, T, seed=1, reset_first=True, out=small_bufs)])
  today = one_member * P
  ok = P < 16 or pop <= today
  print('%-10s S=%-4d B=%d T=%d  P=%-6d n=%-6d path %d, %3d members staged (%6d B LDS)   '
        'rollout_population() %.4f ms   (a) rollout_policy() at B %.4f ms (x%.2f)   '
        '(b) P x rollout_policy() at n: %d x %.4f = %.3f ms (x%.1f)%s'
        % (name, S, B, T, P, B // P, plan[0], plan[3], plan[1], pop, same_b, pop / same_b, P,
           one_member, today, today / pop, '' if ok else '   GATE MISSED'))
  return 0 if ok else GATE_MISSED


def main():
  if len(sys.argv) == 4 and sys.argv[1] == '--row':
    return row(sys.argv[2], int(sys.argv[3]))
  import torch
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'r14_population.txt')
  lines = ['# tools/bench_population.py: a process per row; median of %d event pairs after %d warm-up '
           'rounds, the three calls of a row alternating; %s' % (RUNS, WARM, torch.cuda.get_device_name(0))]
  ok, broke = True, False
  for name, P in [(name, P) for name in GAMES for P in MEMBERS]:
    try:
      done = subprocess.run([sys.executable, os.path.abspath(__file__), '--row', name, str(P)],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            timeout=ROW_SECONDS)
    except subprocess.TimeoutExpired as late:
      lines.append('%s P=%d  ROW TIMED OUT after %d s\n%s' % (name, P, ROW_SECONDS, (late.stderr or '')[-2000:]))
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
  lines.append('gate (rollout_population() no slower than P launches of rollout_policy() on n environments, '
               'every P >= 16): %s' % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 2 if broke else (0 if ok else 1)


if __name__ == '__main__':
  sys.exit(main())
