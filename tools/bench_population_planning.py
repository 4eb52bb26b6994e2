#!/usr/bin/env python3
"""The exact evaluation of a population of policies measured: ONE
`WideGame.evaluate_population()` call (csrc/k_plan.hip) for P policies - each path forced (1 = a
workgroup holds several members in LDS and runs all sweeps in one launch; 2 = one launch per sweep
for all members) and chosen by the library (0) - against the loop it replaces: P calls of
`evaluate_policy()`, one launch by one workgroup each, timed in the same run.

Games: the boat race on its state table (8 states) and the 16x16 maze (159 states); 64 sweeps a
call.  P = 1, 16, 256, 4 096, 65 536 for the one launch; P = 1, 16, 256 for the loop - the loop is
timed where it is quoted and not extrapolated beyond.

GATE: at P = 16 on the boat race the one launch (path 0) takes no longer than the loop of 16
`evaluate_policy()` calls (exit status 1 otherwise).  Sixteen launches against one leave no doubt
about the direction, so there is no margin.  Every other figure is recorded, not gated.

Settled clocks (warm-up runs first), an event pair around each call, median of 25.  Rows, failures
and exit statuses: tools/benchlib.py.

    python tools/bench_population_planning.py [out.txt]     # default: profiles/r16_population_planning.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, SWEEPS, GAMMA = 25, 5, 64, 0.99
GAMES = ('boat_race', 'maze16')
MEMBERS = (1, 16, 256, 4096, 65536)
LOOP_UP_TO = 256
ROW_SECONDS = 600


def row(name, P):
  """One row, in this process: `game`, `S`, `P`, `plan`, `device`, and medians in ms per call of
  SWEEPS sweeps: `path0` .. `path2` (None where the path does not fit) and `loop` (None above
  LOOP_UP_TO, else with `same_bits`: its last member agrees with the launch's)."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, 1).fused
  S = game.n_states
  torch.manual_seed(P)
  policies = torch.rand((P, S, 5), device='cuda').add_(0.5)
  out = game.population_sweep_buffers(P, SWEEPS)
  res = {'game': name, 'S': S, 'P': P, 'device': torch.cuda.get_device_name(0)}
  plan = (ctypes.c_int64 * 5)()
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  lds_max = _hip.config_get('wide_lds_max')
  _hip.check(_hip.lib.campx_wide_population_sweeps_plan(S, P, 0, lds_max, cus, 0, plan),
             'campx_wide_population_sweeps_plan')
  res['plan'] = list(plan)
  for path in (0, 1, 2):
    fits = _hip.lib.campx_wide_population_sweeps_plan(S, P, 0, lds_max, cus, path, plan) == 0
    launch = lambda: game.evaluate_population(policies, GAMMA, SWEEPS, out=out, path=path)
    res['path%d' % path] = benchlib.median_ms(launch, RUNS, WARM) if fits else None
  res['loop'] = None
  if P <= LOOP_UP_TO:
    single = game.sweep_buffers(SWEEPS, want_q=False, greedy=False)

    def loop():
      for m in range(P):
        game.evaluate_policy(policies[m], GAMMA, SWEEPS, want_q=False, out=single)

    res['loop'] = benchlib.median_ms(loop, RUNS, WARM)
    # the two agree: the last member of the loop against the population's
    got = game.evaluate_population(policies, GAMMA, SWEEPS, out=out)['values'][P - 1]
    res['same_bits'] = bool(torch.equal(got.view(torch.int32), single['values'].view(torch.int32)))
  return res


def fmt(v):
  return '      n/a' if v is None else '%9.4f' % v


def report(rows):
  lines = ['# tools/bench_population_planning.py: ms PER CALL of %d sweeps (gamma %.2f), P policies a call; median '
           'of %d event pairs after %d warm-up runs, a fresh process per row, %s'
           % (SWEEPS, GAMMA, RUNS, WARM, benchlib.device_of(rows)),
           '# loop: P calls of evaluate_policy(), timed for P <= %d and not extrapolated beyond' % LOOP_UP_TO,
           '%-10s %5s %6s | %9s %9s %9s | %4s %5s %8s | %9s %9s'
           % ('game', 'S', 'P', 'path 0', 'LDS (1)', 'global(2)', 'auto', 'G', 'grid', 'loop', 'loop / 0')]
  ok = True
  for r in rows:
    gated = r['game'] == 'boat_race' and r['P'] == 16
    met = not gated or r['path0'] <= r['loop']
    ok = ok and met and r.get('same_bits', True)
    ratio = '%9.1f' % (r['loop'] / r['path0']) if r['loop'] is not None else '      n/a'
    lines.append('%-10s %5d %6d | %s %s %s | %4s %5d %8d | %s %s%s%s'
                 % (r['game'], r['S'], r['P'], fmt(r['path0']), fmt(r['path1']), fmt(r['path2']),
                    'LDS' if r['plan'][0] == 1 else 'glb', r['plan'][4], r['plan'][3], fmt(r['loop']), ratio,
                    '' if met else '   GATE MISSED: one launch is slower than the loop',
                    '' if r.get('same_bits', True) else '   THE LOOP AND THE LAUNCH DIFFER'))
  lines.append('gate (boat race, P = 16: the one launch no slower than the loop of 16 evaluate_policy() calls): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, [(name, P) for name in GAMES for P in MEMBERS], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r16_population_planning.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
