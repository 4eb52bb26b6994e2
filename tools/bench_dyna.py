#!/usr/bin/env python3
"""`learn_dyna()` measured: T frames of Dyna-Q - a real step and n planning updates a frame - for B
independent learners in ONE launch, beside `learn_tabular()` on the same game and beside what a
user pays for the same frames without it.

T = 1 000, B = 65 536, the boat race (8 states) and the 16x16 maze (159 states), planning 0 / 5 / 50.
Per game:
  - `learn_tabular()`, planned: the ratio to `learn_dyna()` at planning 0, and its time per frame
    beside `learn_dyna()`'s time per UPDATE, ms / (T * (1 + n)), are recorded, not gated on;
  - per planning setting, the torch restatement on the same device: per frame an epsilon-greedy
    action from `q`, one `play()`, gather / `scatter_` on `q`, the pair marked in a dense mask
    [B, S * 5]; per planning step a draw from that mask (`multinomial`), gathers from the decoded
    table and from `q`, one `scatter_`.  It draws torch's random numbers: the comparator for the
    time, not for the bits (tests/test_dyna_learner.py has those);
  - `learn_dyna()` planned, and with each path forced where the plan takes it.

GATE: every `learn_dyna()` row is no slower than the torch loop of its game and planning setting.
Rows, failures and exit statuses: tools/benchlib.py.

Warm-up first, event pairs, the median of 15 launches and of 3 torch loops.  A row whose first
launch takes more than SLOW_MS is timed as the median of 3 launches, a torch loop that takes more
than SLOW_LOOP_MS is timed once, and both say so.

    python tools/bench_dyna.py [out.txt] [--games boat_race,maze16]     # default: profiles/r23_dyna.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
SLOW_MS, SLOW_RUNS = 300.0, 3
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 20     # torch loops of T frames
SLOW_LOOP_MS = 10000.0             # a torch loop beyond this is timed once
GAMES = ('boat_race', 'maze16')
PLANNINGS = (0, 5, 50)
ROW_SECONDS = 300
ALPHA, GAMMA, EPSILON = 0.1, 0.9, 0.1


def torch_frames(game, q, mask, frames, n):
  """`frames` frames of Dyna-Q with `n` planning updates each, a learner per environment, in torch
  ops and one `play()` per frame; `mask` float32 [B, S * 5] holds 1 for the pairs a learner has met."""
  import torch
  f = game.fused
  table = f.table_arrays()
  t_next = table['next_state'].reshape(-1).long()
  t_reward = torch.nan_to_num(table['reward'].reshape(-1))
  t_c = GAMMA * table['discount'].reshape(-1) * (table['done'].reshape(-1) == 0)
  lanes = torch.arange(B, device='cuda')
  flat_q = q.view(B, -1)
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  one = torch.ones((B, 1), device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    row = q[lanes, s]
    explore = torch.rand((B,), device='cuda') < EPSILON
    a = torch.where(explore, torch.randint(0, 5, (B,), device='cuda'), row.argmax(1))
    old = row.gather(1, a[:, None])
    _, reward, discount = game.play(a.to(torch.int8))
    r = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    b = q[lanes, f.state.long()].max(1).values
    target = r + (GAMMA * discount) * b            # (a frame that ends the episode reports discount 0)
    at = (s * 5 + a)[:, None]
    flat_q.scatter_(1, at, old + ALPHA * (target[:, None] - old))
    mask.scatter_(1, at, one)
    for _ in range(n):
      i = torch.multinomial(mask, 1)
      pair = i[:, 0]
      b = q[lanes, t_next[pair]].max(1).values
      old = flat_q.gather(1, i)
      flat_q.scatter_(1, i, old + ALPHA * ((t_reward[pair] + t_c[pair] * b)[:, None] - old))


def row(name, what, path, n):
  """One row, in this process: `name`, `S`, `what` ('torch', 'tabular' or 'dyna'), the forced `path`
  (0: planned), the planning updates `n`, the median `ms` of `runs` calls, `device`; for 'dyna' also
  `plan` (path, LDS bytes, ...)."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, B)
  f = game.fused
  S = f.n_states
  q = torch.zeros((B, S, 5), device='cuda')
  res = {'name': name, 'S': S, 'what': what, 'path': path, 'n': n, 'device': torch.cuda.get_device_name(0)}
  if what == 'torch':
    mask = torch.zeros((B, S * 5), device='cuda')
    torch_frames(game, q, mask, LOOP_WARM_FRAMES, n)
    loop = lambda: torch_frames(game, q, mask, T, n)
    first = benchlib.event_ms(loop)
    if first > SLOW_LOOP_MS:
      return dict(res, runs=1, ms=first)
    return dict(res, runs=LOOP_RUNS, ms=benchlib.median_ms(loop, LOOP_RUNS))
  hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  if what == 'tabular':
    out = game.learner_buffers(T, 100)
    launch = lambda: game.learn_tabular(T, q, *hyper, seed=1, window=100, out=out)
  else:
    out = game.dyna_buffers(T, 100, path)
    model = {'seen': torch.zeros((B, S * 5), dtype=torch.int32, device='cuda'),
             'n_seen': torch.zeros((B,), dtype=torch.int32, device='cuda')}
    planning = torch.full((B,), n, dtype=torch.int32, device='cuda')
    launch = lambda: game.learn_dyna(T, q, model, planning, *hyper, seed=1, window=100, out=out, path=path)
    plan = (ctypes.c_int64 * 5)()
    _hip.lib.campx_wide_dyna_plan(S, int(f.has_perf), B, _hip.config_get('wide_lds_max'), path, plan)
    res['plan'] = list(plan)
  runs, warm = (RUNS, WARM) if benchlib.event_ms(launch) <= SLOW_MS else (SLOW_RUNS, 0)
  return dict(res, runs=runs, ms=benchlib.median_ms(launch, runs, warm))


def rows_of(name):
  """The rows of a game; a forced path is listed only if the plan takes it (host arithmetic)."""
  from campx_amd import _hip
  S, perf = {'boat_race': (8, 1), 'maze16': (159, 0)}[name]
  plan = (ctypes.c_int64 * 5)()
  paths = [0] + [path for path in (1, 2) if _hip.lib.campx_wide_dyna_plan(
      S, perf, B, _hip.config_get('wide_lds_max'), path, plan) == 0]
  rows = [(name, 'tabular', 0, 0)]
  for n in PLANNINGS:
    rows.append((name, 'torch', 0, n))
    rows += [(name, 'dyna', path, n) for path in paths]
  return rows


def report(records):
  """A game's 'tabular' record comes first and a setting's 'torch' record before its 'dyna' ones, as
  `rows_of()` lists them."""
  lines = ['# tools/bench_dyna.py: a process per row; event pairs, the median of %d launches after %d '
           'warm-up launches and of %d torch loops after %d warm-up frames; rule q; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, benchlib.device_of(records))]
  ok = True
  for name in dict.fromkeys(r['name'] for r in records):
    loop = tabular = None
    for r in (r for r in records if r['name'] == name):
      ms, n = r['ms'], r['n']
      head = '%-10s S=%-4d B=%d T=%d  ' % (name, r['S'], B, T)
      if r['what'] == 'torch':
        loop = ms
        lines.append('%storch restatement, planning %-2d (play() + gather / scatter_ a frame; multinomial + '
                     'gather / scatter_ a planning step)   %.1f ms = %.1f us / frame%s'
                     % (head, n, ms, ms * 1000 / T, '' if r['runs'] == LOOP_RUNS else '   (one loop: slow row)'))
        continue
      if r['what'] == 'tabular':
        tabular = ms
        lines.append('%slearn_tabular() planned   %.3f ms = %.3f us / frame' % (head, ms, ms * 1000 / T))
        continue
      text = '%slearn_dyna() planning %-2d %s -> path %d (%6d B LDS)   %.3f ms = %.3f us / update%s' % (
          head, n, 'planned' if r['path'] == 0 else 'path=%d ' % r['path'], r['plan'][0], r['plan'][1], ms,
          ms * 1000 / (T * (1 + n)), '' if r['runs'] == RUNS else '   (median of %d: slow row)' % r['runs'])
      if tabular is not None:
        text += '   x%.2f learn_tabular()' % (ms / tabular)
      if loop is not None:
        text += ', torch / this = x%.1f' % (loop / ms)
        if ms > loop:
          text += '   GATE MISSED'
          ok = False
      lines.append(text)
  lines.append('gate (learn_dyna() no slower than the torch restatement of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  args, games = list(argv), GAMES
  if '--games' in args:
    i = args.index('--games')
    games = tuple(args[i + 1].split(','))
    del args[i:i + 2]
  records, broke = benchlib.run_rows(__file__, [r for name in games for r in rows_of(name)], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(args, 'r23_dyna.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
