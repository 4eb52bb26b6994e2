#!/usr/bin/env python3
"""`rollout_population()` measured: P policies over one batch in ONE launch, beside what a user
pays for the same today.

Boat race on its state table and the 16x16 maze, T = 100, B = 65 536, P = 1, 16, 256, 65 536
(n = B / P = 65 536 ... 1 environments per member).  Beside each row, in the same process and the
same loop (the three alternate, so that a drifting clock meets them alike):

  (a) one `rollout_policy()` at the same B and T: the same walk under one table;
  (b) one `rollout_policy()` on a game of n environments, times P: P launches on P small games,
      which is what a population costs without this call.

GATE: population time <= (b) for every P >= 16: the one-launch claim is the feature.  The ratio to
(a) is reported, with the path each row took (1 = table and thresholds in LDS, 2 = through L1 / L2)
and the members one workgroup stages, and is not gated.  Rows, failures and exit statuses:
tools/benchlib.py.

Settled clocks (warm-up launches first), event pairs, median of 25.

    python tools/bench_population.py [out.txt]      # default: profiles/r14_population.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, T, B = 25, 10, 100, 65536
MEMBERS = (1, 16, 256, 65536)
GAMES = ('boat_race', 'maze16')
ROW_SECONDS = 300          # a row builds two games and times 35 rounds of three launches: seconds


def row(name, P):
  """One row, in this process: `name`, `S`, `P`, `plan` (path, LDS bytes, -, members staged), the
  medians `pop`, `same_b` (a) and `one_member` (one launch of (b)) in ms, `device`; the outcome is
  the row's gate."""
  import torch
  from campx_amd import _hip
  big, small = benchlib.state_table_game(name, B).fused, benchlib.state_table_game(name, B // P).fused
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
  ms = benchlib.alternating_ms({
      'pop': lambda: big.rollout_population(policies, T, seed=1, reset_first=True, out=pop_bufs),
      'same_b': lambda: big.rollout_policy(one, T, seed=1, reset_first=True, out=big_bufs),
      'one_member': lambda: small.rollout_policy(one, T, seed=1, reset_first=True, out=small_bufs)}, RUNS, WARM)
  res = {'name': name, 'S': S, 'P': P, 'plan': list(plan), 'device': torch.cuda.get_device_name(0)}
  res.update((key, ms[key][0]) for key in ms)
  res['outcome'] = 'ok' if P < 16 or res['pop'] <= res['one_member'] * P else 'gate_missed'
  return res


def report(records):
  lines = ['# tools/bench_population.py: a process per row; median of %d event pairs after %d warm-up '
           'rounds, the three calls of a row alternating; %s' % (RUNS, WARM, benchlib.device_of(records))]
  ok = True
  for r in records:
    met = r['outcome'] == 'ok'
    ok = ok and met
    P, plan, pop = r['P'], r['plan'], r['pop']
    today = r['one_member'] * P
    lines.append('%-10s S=%-4d B=%d T=%d  P=%-6d n=%-6d path %d, %3d members staged (%6d B LDS)   '
                 'rollout_population() %.4f ms   (a) rollout_policy() at B %.4f ms (x%.2f)   '
                 '(b) P x rollout_policy() at n: %d x %.4f = %.3f ms (x%.1f)%s'
                 % (r['name'], r['S'], B, T, P, B // P, plan[0], plan[3], plan[1], pop, r['same_b'],
                    pop / r['same_b'], P, r['one_member'], today, today / pop, '' if met else '   GATE MISSED'))
  lines.append('gate (rollout_population() no slower than P launches of rollout_policy() on n environments, '
               'every P >= 16): %s' % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, [(name, P) for name in GAMES for P in MEMBERS], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r14_population.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
