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

GATE: every `learn_traces()` row is no slower than its game's torch loop.  Rows, failures and exit
statuses: tools/benchlib.py.

Warm-up first, event pairs, the median of 15 launches and of 3 torch loops.  A row whose first
launch takes more than SLOW_MS is timed as the median of 3 launches and says so.

    python tools/bench_traces.py [out.txt] [--teams all] [--games boat_race,maze16]
                                                # default: profiles/r21_traces.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
SLOW_MS, SLOW_RUNS = 300.0, 3
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 50     # torch loops of T frames
GAMES = ('boat_race', 'maze16')
TEAMS = (1, 2, 8, 64, 256)
ALL_TEAMS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
ROW_SECONDS = 300
ALPHA, GAMMA, EPSILON, LAM = 0.1, 0.9, 0.1, 0.9


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
  """One row, in this process: `name`, `S`, `what` ('torch', 'tabular' or 'traces'), the forced
  `path` and `team` (0, 0: planned), the median `ms` of `runs` calls, `device`; for 'traces' also
  `plan` (path, team, LDS bytes, ...)."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, B)
  f = game.fused
  S = f.n_states
  q = torch.zeros((B, S, 5), device='cuda')
  z = torch.zeros((B, S, 5), device='cuda')
  res = {'name': name, 'S': S, 'what': what, 'path': path, 'team': team, 'device': torch.cuda.get_device_name(0)}
  if what == 'torch':
    torch_frames(game, q, z, LOOP_WARM_FRAMES)
    return dict(res, runs=LOOP_RUNS, ms=benchlib.median_ms(lambda: torch_frames(game, q, z, T), LOOP_RUNS))
  hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  out = game.learner_buffers(T, 100)
  if what == 'tabular':
    launch = lambda: game.learn_tabular(T, q, *hyper, seed=1, window=100, out=out)
  else:
    lam = torch.full((B,), LAM, device='cuda')
    launch = lambda: game.learn_traces(T, q, z, lam, 'accumulating', *hyper, seed=1, window=100, out=out,
                                       path=path, team=team)
    plan = (ctypes.c_int64 * 5)()
    _hip.lib.campx_wide_traces_plan(S, int(f.has_perf), B, _hip.config_get('wide_lds_max'), path, team, plan)
    res['plan'] = list(plan)
  runs, warm = (RUNS, WARM) if benchlib.event_ms(launch) <= SLOW_MS else (SLOW_RUNS, 0)
  return dict(res, runs=runs, ms=benchlib.median_ms(launch, runs, warm))


def rows_of(name, teams):
  """The rows of a game; a forced shape is listed only if the plan takes it (host arithmetic)."""
  from campx_amd import _hip
  S, perf = {'boat_race': (8, 1), 'maze16': (159, 0)}[name]
  rows = [(name, 'torch', 0, 0), (name, 'tabular', 0, 0), (name, 'traces', 0, 0)]
  plan = (ctypes.c_int64 * 5)()
  for path in (1, 2):
    for team in teams:
      if _hip.lib.campx_wide_traces_plan(S, perf, B, _hip.config_get('wide_lds_max'), path, team, plan) == 0:
        rows.append((name, 'traces', path, team))
  return rows


def report(records):
  """A game's 'torch' and 'tabular' records come before its 'traces' ones, as `rows_of()` lists them."""
  lines = ['# tools/bench_traces.py: a process per row; event pairs, the median of %d launches after %d '
           'warm-up launches and of %d torch loops after %d warm-up frames; lam %.2f, accumulating, rule q; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, LAM, benchlib.device_of(records))]
  ok = True
  for name in dict.fromkeys(r['name'] for r in records):
    loop = tabular = best = planned = None
    for r in (r for r in records if r['name'] == name):
      ms = r['ms']
      head = '%-10s S=%-4d B=%d T=%d  ' % (name, r['S'], B, T)
      if r['what'] == 'torch':
        loop = ms
        lines.append('%storch restatement (play() + dense q += step * z; z *= c per frame)   %.1f ms = %.1f us / frame'
                     % (head, ms, ms * 1000 / T))
        continue
      if r['what'] == 'tabular':
        tabular = ms
        label = 'learn_tabular() planned'
      else:
        shape = (r['path'], r['team'])
        label = 'learn_traces() %s -> path %d team %-3d (%6d B LDS)' % (
            'planned        ' if shape == (0, 0) else 'path=%d team=%-3d' % shape, *r['plan'][:3])
      text = '%s%s   %.3f ms = %.2f us / frame%s' % (
          head, label, ms, ms * 1000 / T, '' if r['runs'] == RUNS else '   (median of %d: slow row)' % r['runs'])
      if r['what'] == 'traces':
        text += '   x%.1f learn_tabular(), torch / this = x%.1f' % (ms / tabular, loop / ms)
        if ms > loop:
          text += '   GATE MISSED'
          ok = False
        if shape == (0, 0):
          planned = ms
        elif best is None or ms < best[0]:
          best = (ms,) + shape
      lines.append(text)
    if best is not None and planned is not None:
      lines.append('%s: fastest forced shape path %d team %d at %.3f ms; planned %.3f ms (%s)'
                   % (name, best[1], best[2], best[0], planned,
                      'the planned shape is not the fastest' if best[0] < 0.95 * planned
                      else 'within 5% of the fastest'))
  lines.append('gate (learn_traces() no slower than the torch restatement of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  args, teams, games = list(argv), TEAMS, GAMES
  if '--teams' in args:
    i = args.index('--teams')
    teams = ALL_TEAMS if args[i + 1] == 'all' else tuple(int(x) for x in args[i + 1].split(','))
    del args[i:i + 2]
  if '--games' in args:
    i = args.index('--games')
    games = tuple(args[i + 1].split(','))
    del args[i:i + 2]
  records, broke = benchlib.run_rows(__file__, [r for name in games for r in rows_of(name, teams)], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(args, 'r21_traces.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
