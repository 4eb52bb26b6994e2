#!/usr/bin/env python3
"""Exact state visitation on a state table measured, per frame: `WideGame.state_visitation()`
(csrc/k_visit.hip) with each path forced (1 = all frames in one launch from LDS, where the table
fits; 2 = one launch per frame, 64-bit global atomic adds) and chosen by the library (0), against
the same frame restated in torch on the same device in the same run:

    x = (d >> 24)[:, None] * N + (((d & 0xffffff)[:, None] * N) >> 24);  x[:, 1:] -= x[:, :-1].clone()
    visits += x;  finished[t] = x[done].sum()
    d = zeros(S).index_add_(0, next[~done], x[~done]);  d[0] += finished[t]

(int64 throughout: the restatement gives the same numbers, and is checked to; it is the yardstick
for time, tests/visitation_reference.py the one for bits).

Sizes: the boat race on its state table (8 states); synthetic tables of 1 940 states and of
4 400 000 states, the size of the 16x16 two-box sokoban's enumerated table - every state reachable,
next states uniform over the table, a tenth of the entries ending the episode.  The start is uniform
over the states, so that every state has mass at every frame: a frame of the global path is then
S * 5 atomic adds less the entries that end the episode - also printed as atomic adds per second,
global (path 2 at 4.4 M states) and LDS (path 1 at 1 940).

GATE: path 0 is no slower per frame than the torch restatement at every size (exit status 1
otherwise; the table says where it is missed).

Settled clocks (warm-up runs first), event pairs around FRAMES frames, median of 15 runs.  Rows,
failures and exit statuses: tools/benchlib.py.

    python tools/bench_visitation.py [out.txt]        # default: profiles/r12_visitation.txt
"""
import sys
import types

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, FRAMES = 15, 5, 32
ROWS = (('boat_race', 8), ('synthetic', 1940), ('synthetic', 4400000))
ROW_SECONDS = 900


def row(kind, S):
  """One row, in this process: `kind`, `S`, `alive` (entries that do not end the episode), `same`
  (the torch restatement gives the same numbers), `plan`, `device`, and `torch`, `path0` .. `path2`
  (None where the path does not fit): medians in ms PER FRAME."""
  import ctypes
  import torch
  from campx_amd import _hip
  if kind == 'boat_race':
    from campx_amd.games import boat_race
    engine = boat_race.build(1, 'cuda')
    engine.use_state_table()
    engine.its_showtime()
    game = engine.fused
  else:
    from bench_planning import synthetic_table
    from campx_amd import wide
    game = wide.WideGame(types.SimpleNamespace(rows=4, cols=4), 1, 'cuda', synthetic_table(S))
  assert game.n_states == S
  tabs = game.table_arrays()
  nxt, done = tabs['next_state'].long(), tabs['done'] != 0
  alive = ~done
  nxt_alive = nxt[alive]
  w = torch.rand((S, 5), device='cuda').add_(0.5)
  unit = 1 << 38
  start = torch.full((S,), unit // S, dtype=torch.int64, device='cuda')
  out = game.visitation_buffers(FRAMES)
  call = lambda path: game.state_visitation(w, FRAMES, start=start, out=out, path=path)
  N = call(0)['counts'].long().cumsum(1)

  def torch_frames():
    d = start.clone()
    visits = torch.zeros((S, 5), dtype=torch.int64, device='cuda')
    finished = torch.zeros((FRAMES,), dtype=torch.int64, device='cuda')
    for t in range(FRAMES):
      x = (d >> 24)[:, None] * N + (((d & 0xffffff)[:, None] * N) >> 24)
      x[:, 1:] -= x[:, :-1].clone()
      visits += x
      finished[t] = x[done].sum()
      d = torch.zeros((S,), dtype=torch.int64, device='cuda').index_add_(0, nxt_alive, x[alive])
      d[0] += finished[t]
    return visits, finished, d

  res = {'kind': kind, 'S': S, 'alive': int(alive.sum())}
  want = torch_frames()
  got = call(0)
  res['same'] = bool(torch.equal(got['visits'], want[0]) and torch.equal(got['finished'], want[1])
                     and torch.equal(got['final'], want[2]))
  res['torch'] = benchlib.median_ms(torch_frames, RUNS, WARM) / FRAMES
  plan = (ctypes.c_int64 * 4)()
  _hip.check(_hip.lib.campx_wide_visit_plan(S, _hip.config_get('wide_lds_max'), 0, plan),
             'campx_wide_visit_plan')
  res['plan'] = int(plan[0])
  for path in (0, 1, 2):
    fits = _hip.lib.campx_wide_visit_plan(S, _hip.config_get('wide_lds_max'), path, plan) == 0
    res['path%d' % path] = benchlib.median_ms(lambda: call(path), RUNS, WARM) / FRAMES if fits else None
  game.check_actions()
  res['device'] = torch.cuda.get_device_name(0)
  return res


def fmt(v):
  return '    n/a   ' if v is None else '%10.5f' % v


def report(rows):
  lines = ['# tools/bench_visitation.py: ms PER FRAME (%d frames a call, uniform start); median of %d event '
           'pairs after %d warm-up runs, a fresh process per row, %s'
           % (FRAMES, RUNS, WARM, benchlib.device_of(rows)),
           '%-10s %8s | %10s | %10s %10s %10s | %4s | %8s | %s'
           % ('table', 'S', 'torch', 'path 0', 'LDS (1)', 'global (2)', 'auto', 'torch/0', 'same numbers')]
  ok = True
  for r in rows:
    t0, tt = r['path0'], r['torch']
    met = t0 <= tt and r['same']
    ok = ok and met
    lines.append('%-10s %8d | %10.5f | %s %s %s | %4s | %8.2f | %s%s'
                 % (r['kind'], r['S'], tt, fmt(t0), fmt(r['path1']), fmt(r['path2']),
                    'LDS' if r['plan'] == 1 else 'glb', tt / t0, 'yes' if r['same'] else 'NO',
                    '' if met else '   GATE MISSED: path 0 is slower than torch, or differs'))
    for name, key in (('LDS', 'path1'), ('global', 'path2')):
      if r[key]:
        lines.append('#   64-bit %s atomic adds: %d a frame, %.3g per second (everything else of the frame '
                     'included)' % (name, r['alive'], r['alive'] / (r[key] * 1e-3)))
  lines.append('gate (path 0 no slower per frame than the torch restatement at every size, same numbers): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r12_visitation.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
