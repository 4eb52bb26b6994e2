#!/usr/bin/env python3
"""The exact visitation of a population of policies measured: ONE `WideGame.visit_population()`
call (csrc/k_visit.hip) for P policies - as the library chooses (path 0) and with the
one-launch-per-frame path forced (2) - against the loop it replaces: P calls of
`state_visitation()`, a counts launch and one workgroup each, timed in the same run.

Games: the boat race on its state table (8 states) and the 16x16 maze (159 states); 32 frames a
call; P = 1, 16, 256, 4 096.

GATE: at P = 16 on the boat race the one launch (path 0) takes less time than the loop of 16
`state_visitation()` calls (exit status 1 otherwise).  Every other figure is recorded, not gated:
P = 1 beside `state_visitation()` - it may cost more -, and every forced path 2, which says whether
"LDS whenever a member fits" holds at that size.

Settled clocks (warm-up runs first), an event pair around each call, the three ALTERNATING in each
of 25 rounds, median and spread (min .. max) of the 25 (rows, failures and exit statuses:
tools/benchlib.py).  Every call
writes into buffers made once (`out=`), starts from `start=None` and so reads nothing back; the
times are what a caller waits for, host launch cost included.

    python tools/bench_visit_population.py [out.txt]     # default: profiles/r17_visit_population.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, FRAMES = 25, 5, 32
GAMES = ('boat_race', 'maze16')
MEMBERS = (1, 16, 256, 4096)
ROW_SECONDS = 600


def row(name, P):
  """One row, in this process: `game`, `S`, `P`, `plan`, `device`, `same_bits`, and `path0`, `loop`,
  `path2`: (median, min, max) in ms per call of FRAMES frames for all P members."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, 1).fused
  S = game.n_states
  torch.manual_seed(P)
  policies = torch.rand((P, S, 5), device='cuda').add_(0.5)
  out = game.visit_population_buffers(P, FRAMES)
  single = game.visitation_buffers(FRAMES)
  res = {'game': name, 'S': S, 'P': P, 'device': torch.cuda.get_device_name(0)}
  plan = (ctypes.c_int64 * 5)()
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  _hip.check(_hip.lib.campx_wide_visit_population_plan(S, P, _hip.config_get('wide_lds_max'), cus, 0, plan),
             'campx_wide_visit_population_plan')
  res['plan'] = list(plan)

  def loop():
    for m in range(P):
      game.state_visitation(policies[m], FRAMES, out=single)

  res.update(benchlib.alternating_ms({
      'path0': lambda: game.visit_population(policies, FRAMES, out=out, path=0),
      'loop': loop,
      'path2': lambda: game.visit_population(policies, FRAMES, out=out, path=2)}, RUNS, WARM))
  # the three agree: the last member of the loop against the population's, on either path
  same = True
  for path in (0, 2):
    got = game.visit_population(policies, FRAMES, out=out, path=path)
    loop()
    same = same and all(bool(torch.equal(got[k][P - 1], single[k])) for k in ('visits', 'final', 'counts'))
    same = same and bool(torch.equal(got['finished'][:, P - 1], single['finished']))
  res['same_bits'] = same
  return res


def fmt(v):
  return '%9.4f (%8.4f .. %9.4f)' % tuple(v)


def report(rows):
  lines = ['# tools/bench_visit_population.py: ms PER CALL of %d frames, P policies a call; median (min .. max) of %d '
           'event pairs after %d warm-up rounds, the three alternating in each round, a fresh process per row, %s'
           % (FRAMES, RUNS, WARM, benchlib.device_of(rows)),
           '# loop: P calls of state_visitation(); path 2: visit_population() with one launch per frame forced',
           '%-10s %4s %5s | %-32s | %-32s | %-32s | %4s %3s %6s | %8s %8s'
           % ('game', 'S', 'P', 'visit_population(), path 0', 'loop of state_visitation()', 'path 2 forced',
              'auto', 'G', 'grid', 'loop / 0', '2 / 0')]
  ok = True
  for r in rows:
    gated = r['game'] == 'boat_race' and r['P'] == 16
    met = not gated or r['path0'][0] < r['loop'][0]
    ok = ok and met and r['same_bits']
    lines.append('%-10s %4d %5d | %s | %s | %s | %4s %3d %6d | %8.2f %8.2f%s%s'
                 % (r['game'], r['S'], r['P'], fmt(r['path0']), fmt(r['loop']), fmt(r['path2']),
                    'LDS' if r['plan'][0] == 1 else 'glb', r['plan'][4], r['plan'][3],
                    r['loop'][0] / r['path0'][0], r['path2'][0] / r['path0'][0],
                    '' if met else '   GATE MISSED: the one launch is not faster than the loop',
                    '' if r['same_bits'] else '   THE LOOP AND THE LAUNCH DIFFER'))
  lines.append('gate (boat race, P = 16: the one launch takes less time than the loop of 16 state_visitation() '
               'calls): %s' % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, [(name, P) for name in GAMES for P in MEMBERS], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r17_visit_population.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
