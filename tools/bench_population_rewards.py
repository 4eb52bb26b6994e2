#!/usr/bin/env python3
"""A population of rewards measured: ONE `WideGame.value_iteration_population(rewards=...)` call
and ONE `WideGame.evaluate_population(rewards=...)` call (csrc/k_plan.hip,
`campx::wide_population_solve`) for P reward tables - on the planned path (0) and with each path
forced (1 = a workgroup holds several members and their rewards in LDS and runs all sweeps in one
launch; 2 = one launch per sweep for all members) - against the loop each replaces: P calls of
`value_iteration(reward=rewards[m])`, or of `evaluate_policy(policies[m], reward=rewards[m])`, one
launch by one workgroup each, timed in the same run.

Games: the boat race on its state table (8 states) and the 16x16 maze (159 states); 64 sweeps a
call; P = 1, 16, 256, 4 096, the loop timed at every one of them.

GATE: at every P >= 16, for both forms and both games, the one launch (path 0) takes no longer than
the loop timed in the same run (exit status 1 otherwise).  The loop is what the call replaces, so
there is no other yardstick and no margin.  At P = 1 the ratio is recorded and not gated: the
members instance is expected to cost a little more than the single call there.  Nothing here tunes
the members to a workgroup or the choice of path; the forced paths are recorded beside the planned
one and no crossover is claimed.

Settled clocks (warm-up runs first), an event pair around each call, median of 25, the timed
alternatives taking turns within every one of the 25 rounds.  Rows, failures and exit statuses:
tools/benchlib.py.

    python tools/bench_population_rewards.py [out.txt]      # default: profiles/r20_population_rewards.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, SWEEPS, GAMMA = 25, 3, 64, 0.99
GAMES = ('boat_race', 'maze16')
MEMBERS = (1, 16, 256, 4096)
FORMS = ('greedy', 'policy')
ROW_SECONDS = 900


def row(name, P):
  """One row, in this process: `game`, `S`, `P`, `device`, and per form ('greedy', 'policy') a dict
  of `plan`, `same_bits` and medians in ms per call of SWEEPS sweeps: `loop`, `path0`, and `path1`,
  `path2` where they fit."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, 1).fused
  S = game.n_states
  torch.manual_seed(P)
  policies = torch.rand((P, S, 5), device='cuda').add_(0.5)
  rewards = torch.rand((P, S, 5), device='cuda').mul_(2).sub_(1)
  rewards[0] = game.table_arrays()['reward']
  out = game.population_sweep_buffers(P, SWEEPS, greedy=True)
  single = game.sweep_buffers(SWEEPS, want_q=False, greedy=True)
  res = {'game': name, 'S': S, 'P': P, 'device': torch.cuda.get_device_name(0)}
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  lds_max = _hip.config_get('wide_lds_max')
  for form in FORMS:
    policy = 1 if form == 'policy' else 0
    plan = (ctypes.c_int64 * 5)()
    _hip.check(_hip.lib.campx_wide_population_solve_plan(S, P, policy, 1, lds_max, cus, 0, plan),
               'campx_wide_population_solve_plan')
    r = {'plan': list(plan)}
    if policy:
      launch = lambda path: game.evaluate_population(policies, GAMMA, SWEEPS, rewards=rewards, out=out, path=path)

      def loop():
        for m in range(P):
          game.evaluate_policy(policies[m], GAMMA, SWEEPS, reward=rewards[m], want_q=False, out=single)
    else:
      launch = lambda path: game.value_iteration_population(GAMMA, SWEEPS, rewards=rewards, out=out, path=path)

      def loop():
        for m in range(P):
          game.value_iteration(GAMMA, SWEEPS, reward=rewards[m], want_q=False, out=single)

    alternatives = {'loop': loop}
    for path in (0, 1, 2):
      if _hip.lib.campx_wide_population_solve_plan(S, P, policy, 1, lds_max, cus, path, plan) == 0:
        alternatives['path%d' % path] = (lambda path: lambda: launch(path))(path)
    r.update((key, ms[0]) for key, ms in benchlib.alternating_ms(alternatives, RUNS, WARM).items())
    # the two agree: the last member of the loop against the population's
    loop()
    got = launch(0)['values'][P - 1]
    r['same_bits'] = bool(torch.equal(got.view(torch.int32), single['values'].view(torch.int32)))
    res[form] = r
  return res


def fmt(v):
  return '      n/a' if v is None else '%9.4f' % v


def report(rows):
  lines = ['# tools/bench_population_rewards.py: ms PER CALL of %d sweeps (gamma %.2f), P reward tables a call; '
           'median of %d event pairs after %d warm-up rounds, the alternatives taking turns within a round, '
           'a fresh process per row, %s' % (SWEEPS, GAMMA, RUNS, WARM, benchlib.device_of(rows)),
           '# greedy: value_iteration_population(rewards=) against P calls of value_iteration(reward=); '
           'policy: evaluate_population(rewards=) against P calls of evaluate_policy(reward=)',
           '# gated: path 0 <= loop at P >= 16.  Not measured: other table sizes, other sweep counts, the '
           'crossover between the paths, any other members to a workgroup than the rule gives',
           '%-10s %-6s %5s %6s | %9s %9s %9s | %4s %5s %8s | %9s %9s'
           % ('game', 'form', 'S', 'P', 'path 0', 'LDS (1)', 'global(2)', 'auto', 'G', 'grid', 'loop', 'loop / 0')]
  ok = True
  for r in rows:
    for form in FORMS:
      f = r[form]
      gated = r['P'] >= 16
      met = not gated or f['path0'] <= f['loop']
      ok = ok and met and f['same_bits']
      lines.append('%-10s %-6s %5d %6d | %s %s %s | %4s %5d %8d | %s %9.2f%s%s'
                   % (r['game'], form, r['S'], r['P'], fmt(f['path0']), fmt(f.get('path1')), fmt(f.get('path2')),
                      'LDS' if f['plan'][0] == 1 else 'glb', f['plan'][4], f['plan'][3], fmt(f['loop']),
                      f['loop'] / f['path0'],
                      '' if met else '   GATE MISSED: one launch is slower than the loop',
                      '' if f['same_bits'] else '   THE LOOP AND THE LAUNCH DIFFER'))
  lines.append('gate (P >= 16, both forms, both games: the one launch no slower than the loop it replaces): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, [(name, P) for name in GAMES for P in MEMBERS], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r20_population_rewards.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
