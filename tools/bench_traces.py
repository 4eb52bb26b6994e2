#!/usr/bin/env python3
"""`learn_traces()` measured: T frames of Q(lambda) for B independent learners in ONE launch, beside
`learn_tabular()` on the same game and beside what a user pays for the same frames without it.

T = 1 000, B = 65 536, the boat race (8 states) and the 16x16 maze (159 states).  Per game:
  - the torch restatement on the same device: per frame an epsilon-greedy action from `q`, one
    `play()`, the TD error, and the DENSE update `q += step * z; z *= c` over [B, S * 5] (with the
    Watkins cut and the bump as a `scatter_`).  It draws torch's random numbers: the comparator for
    the time, not for the bits (tests/test_trace_learner.py has those);
  - `learn_tabular()`, planned: the ratio a trace costs is recorded, not gated on;
  - `learn_traces()` planned, and with every (path, team) forced that fits, team in TEAMS
    (`--teams all`: every power of two up to 256).

GATE: every `learn_traces()` row is no slower than its game's torch loop (exit status 1 otherwise).
A row that fails or outlasts its time limit ends the run (exit status 2): nothing more is started
on the device, and what was collected is written.

A fresh process per row; warm-up first, event pairs, the median of 15 launches and of 3 torch
loops.  A row whose first launch takes more than SLOW_MS is timed as the median of 3 launches and
says so.

    python tools/bench_traces.py [out.txt] [--teams all] [--games boat_race,maze16]
                                                # default: profiles/r21_traces.txt
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
SLOW_MS, SLOW_RUNS = 300.0, 3
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 50     # torch loops of T frames
GAMES = ('boat_race', 'maze16')
TEAMS = (1, 2, 8, 64, 256)
ALL_TEAMS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
ROW_SECONDS = 300
ALPHA, GAMMA, EPSILON, LAM = 0.1, 0.9, 0.1, 0.9


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


def plan_of(f, path, team):
  from campx_amd import _hip
  plan = (ctypes.c_int64 * 5)()
  code = _hip.lib.campx_wide_traces_plan(f.n_states, int(f.has_perf), B, _hip.config_get('wide_lds_max'),
                                         path, team, plan)
  return code, list(plan)


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


def torch_frames(game, q, z, frames):
  """`frames` frames of Watkins's Q(lambda), accumulating traces, a learner per environment, in
  torch ops and one `play()` per frame; the sweep and the decay are dense over [B, S * 5]."""
  import torch
  f = game.fused
  lanes = torch.arange(B, device='cuda')
  flat_q, flat_z = q.view(B, -1), z.view(B, -1)
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    row = q[lanes, s]
    greedy = row.argmax(1)
    explore = torch.rand((B,), device='cuda') < EPSILON
    a = torch.where(explore, torch.randint(0, 5, (B,), device='cuda'), greedy)
    old = row.gather(1, a[:, None])
    flat_z.mul_((old == row.max(1, keepdim=True).values).float())            # the cut
    _, reward, discount = game.play(a.to(torch.int8))
    r = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    b = q[lanes, f.state.long()].max(1).values
    target = r + (GAMMA * discount) * b            # (a frame that ends the episode reports discount 0)
    at = (s * 5 + a)[:, None]
    flat_z.scatter_add_(1, at, torch.ones((B, 1), device='cuda'))
    step = ALPHA * (target[:, None] - old)
    flat_q.addcmul_(step, flat_z)
    flat_z.mul_(((GAMMA * LAM) * discount)[:, None])


def row(name, what, path, team):
  """One row, in this process: prints 'ms<TAB>text'."""
  import torch
  game = build(name)
  f = game.fused
  S = f.n_states
  q = torch.zeros((B, S, 5), device='cuda')
  z = torch.zeros((B, S, 5), device='cuda')
  head = '%-10s S=%-4d B=%d T=%d  ' % (name, S, B, T)
  if what == 'torch':
    torch_frames(game, q, z, LOOP_WARM_FRAMES)
    torch.cuda.synchronize()
    ms = timed_ms(lambda: torch_frames(game, q, z, T), LOOP_RUNS)
    print('%.6f\t%storch restatement (play() + dense q += step * z; z *= c per frame)   %.1f ms = %.1f us / frame'
          % (ms, head, ms, ms * 1000 / T))
    return 0
  hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  out = game.learner_buffers(T, 100)
  if what == 'tabular':
    launch = lambda: game.learn_tabular(T, q, *hyper, seed=1, window=100, out=out)
    label = 'learn_tabular() planned'
  else:
    lam = torch.full((B,), LAM, device='cuda')
    launch = lambda: game.learn_traces(T, q, z, lam, 'accumulating', *hyper, seed=1, window=100, out=out,
                                       path=path, team=team)
    plan = plan_of(f, path, team)[1]
    label = 'learn_traces() %s -> path %d team %-3d (%6d B LDS)' % (
        'planned        ' if (path, team) == (0, 0) else 'path=%d team=%-3d' % (path, team),
        plan[0], plan[1], plan[2])
  first = timed_ms(launch, 1)
  runs, warm = (RUNS, WARM) if first <= SLOW_MS else (SLOW_RUNS, 0)
  for _ in range(warm):
    launch()
  torch.cuda.synchronize()
  ms = timed_ms(launch, runs)
  print('%.6f\t%s%s   %.3f ms = %.2f us / frame%s'
        % (ms, head, label, ms, ms * 1000 / T, '' if runs == RUNS else '   (median of %d: slow row)' % runs))
  return 0


def rows_of(name, teams):
  """The rows of a game; a forced shape is listed only if the plan takes it (host arithmetic)."""
  from campx_amd import _hip
  S, perf = {'boat_race': (8, 1), 'maze16': (159, 0)}[name]
  rows = [('torch', 0, 0), ('tabular', 0, 0), ('traces', 0, 0)]
  plan = (ctypes.c_int64 * 5)()
  for path in (1, 2):
    for team in teams:
      if _hip.lib.campx_wide_traces_plan(S, perf, B, _hip.config_get('wide_lds_max'), path, team, plan) == 0:
        rows.append(('traces', path, team))
  return rows


def main():
  args = sys.argv[1:]
  if len(args) == 5 and args[0] == '--row':
    return row(args[1], args[2], int(args[3]), int(args[4]))
  import torch
  teams, games = TEAMS, GAMES
  if '--teams' in args:
    i = args.index('--teams')
    teams = ALL_TEAMS if args[i + 1] == 'all' else tuple(int(x) for x in args[i + 1].split(','))
    del args[i:i + 2]
  if '--games' in args:
    i = args.index('--games')
    games = tuple(args[i + 1].split(','))
    del args[i:i + 2]
  path = args[0] if args else os.path.join(REPO, 'profiles', 'r21_traces.txt')
  lines = ['# tools/bench_traces.py: a process per row; event pairs, the median of %d launches after %d '
           'warm-up launches and of %d torch loops after %d warm-up frames; lam %.2f, accumulating, rule q; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, LAM, torch.cuda.get_device_name(0))]
  ok, broke = True, False
  for name in games:
    loop = tabular = None
    best = None
    planned = None
    for what, forced, team in rows_of(name, teams):
      cmd = [sys.executable, os.path.abspath(__file__), '--row', name, what, str(forced), str(team)]
      try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              timeout=ROW_SECONDS)
      except subprocess.TimeoutExpired as late:
        lines.append('%s %s path %d team %d  ROW TIMED OUT after %d s\n%s'
                     % (name, what, forced, team, ROW_SECONDS, (late.stderr or '')[-2000:]))
        ok, broke = False, True
        break                      # nothing more is started on the device after a failure
      if done.returncode != 0 or '\t' not in done.stdout:
        lines.append('%s %s path %d team %d  ROW FAILED (exit status %d)\n%s'
                     % (name, what, forced, team, done.returncode, done.stderr.rstrip('\n')))
        ok, broke = False, True
        break                      # nothing more is started on the device after a failure
      ms, text = done.stdout.rstrip('\n').split('\t', 1)
      ms = float(ms)
      if what == 'torch':
        loop = ms
      elif what == 'tabular':
        tabular = ms
      else:
        text += '   x%.1f learn_tabular(), torch / this = x%.1f' % (ms / tabular, loop / ms)
        if ms > loop:
          text += '   GATE MISSED'
          ok = False
        if (forced, team) == (0, 0):
          planned = ms
        elif best is None or ms < best[0]:
          best = (ms, forced, team)
      lines.append(text)
      print(text, flush=True)
    if broke:
      break
    if best is not None and planned is not None:
      lines.append('%s: fastest forced shape path %d team %d at %.3f ms; planned %.3f ms (%s)'
                   % (name, best[1], best[2], best[0], planned,
                      'the planned shape is not the fastest' if best[0] < 0.95 * planned
                      else 'within 5% of the fastest'))
  if broke:
    lines.append('the run ended at the row above; the rows after it were not started')
  lines.append('gate (learn_traces() no slower than the torch restatement of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 2 if broke else (0 if ok else 1)


if __name__ == '__main__':
  sys.exit(main())
