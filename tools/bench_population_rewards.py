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
alternatives taking turns within every one of the 25 rounds, a fresh process per row.

    python tools/bench_population_rewards.py [out.txt]      # default: profiles/r20_population_rewards.txt
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RUNS, WARM, SWEEPS, GAMMA = 25, 3, 64, 0.99
GAMES = ('boat_race', 'maze16')
MEMBERS = (1, 16, 256, 4096)
FORMS = ('greedy', 'policy')


def medians_ms(alternatives):
  """{name: median ms} of the callables of `alternatives`, which take turns within each round."""
  import torch
  for _ in range(WARM):
    for fn in alternatives.values():
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in alternatives}
  for _ in range(RUNS):
    for name, fn in alternatives.items():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      times[name].append(e0.elapsed_time(e1))
  return {name: statistics.median(t) for name, t in times.items()}


def build(name):
  from campx_amd.games import boat_race, maze
  if name == 'boat_race':
    game = boat_race.build(1, 'cuda')
    game.use_state_table()
  else:
    game = maze.build(16, 16, batch=1, device='cuda')
  game.its_showtime()
  game.fused.validate_actions = False
  return game.fused


def row(name, P):
  """One row, in this process: per form, medians in ms per call of SWEEPS sweeps."""
  import torch
  from campx_amd import _hip
  game = build(name)
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
    r.update(medians_ms(alternatives))
    # the two agree: the last member of the loop against the population's
    loop()
    got = launch(0)['values'][P - 1]
    r['same_bits'] = bool(torch.equal(got.view(torch.int32), single['values'].view(torch.int32)))
    res[form] = r
  return res


def fmt(v):
  return '      n/a' if v is None else '%9.4f' % v


def main():
  if len(sys.argv) > 1 and sys.argv[1] == '--row':
    print('ROW ' + json.dumps(row(sys.argv[2], int(sys.argv[3]))))
    return 0
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'r20_population_rewards.txt')
  rows = []
  for name in GAMES:
    for P in MEMBERS:                      # a fresh process per row, one at a time
      done = subprocess.run([sys.executable, os.path.abspath(__file__), '--row', name, str(P)],
                            stdout=subprocess.PIPE, text=True, timeout=900)
      if done.returncode != 0:
        print('row %s P=%d failed with status %d' % (name, P, done.returncode))
        return 2
      rows.append(json.loads([l for l in done.stdout.splitlines() if l.startswith('ROW ')][-1][4:]))
      print('row %s P=%d done' % (name, P), flush=True)
  lines = ['# tools/bench_population_rewards.py: ms PER CALL of %d sweeps (gamma %.2f), P reward tables a call; '
           'median of %d event pairs after %d warm-up rounds, the alternatives taking turns within a round, '
           'a fresh process per row, %s' % (SWEEPS, GAMMA, RUNS, WARM, rows[0]['device']),
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
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
