#!/usr/bin/env python3
"""`vtrace_returns()` measured beside what it must beat or match.

T = 100 at B = 4 096 and 65 536, on the padded buffers of `rollout_population_buffers()` /
`rollout_policy_buffers()` filled by a rollout of uniform policies:

  * ratio mode;
  * table mode with path 1 (tables in LDS) and path 2 (through the caches) forced: the boat race
    with P = 1 (8 + 8 states) and P = 16 (8 + 128), the 16x16 maze (159 + 159);
  * baseline (a): `discounted_returns(values=...)` on the same buffers - the on-policy kernel of the
    same shape.  Only the ratio is reported (by bytes ratio mode moves 25 per environment-frame
    against 21);
  * baseline (b): the rule restated in torch on the same device - everything that does not depend
    on the frame after as whole-tensor operations, the recursion as a reversed loop of T steps -
    with its ratio built by two `table_lookup()` calls and a division (given, in ratio mode).
  GATE: the kernel is faster than (b) at every size and in every mode measured (exit status 1
  otherwise).

Settled clocks (warm-up runs first), event pairs, median of 25 runs.  Rows, failures and exit
statuses: tools/benchlib.py.

    python tools/bench_vtrace.py [out.txt]        # default: profiles/r18_vtrace.txt
"""
import functools
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, T = 25, 10, 100
GAMMA, LAM, BARS = 0.99, 0.95, (1.0, 1.0, 1.0)
ROWS = [(kind, B) for B in (4096, 65536) for kind in ('ratio', 'boat_race_p1', 'boat_race_p16', 'maze16')]
ROW_SECONDS = 120
median = functools.partial(benchlib.median_ms, runs=RUNS, warm=WARM)


def torch_vtrace(reward, done, discount, values, bootstrap, w):
  """Baseline (b) behind its ratio: the rule in torch, the recursion a reversed loop."""
  import torch
  over = done.bool()
  r = torch.nan_to_num(reward, nan=0.0)
  c = GAMMA * discount
  w = torch.where(w > 0, w, torch.zeros_like(w))
  rho, cs, rpg = (w.clamp(max=bar) for bar in BARS)
  v_next = torch.cat([values[1:], bootstrap[None]])
  delta = rho * (torch.where(over, r, r + c * v_next) - values)
  k = (c * LAM) * cs
  D, rows = torch.zeros_like(bootstrap), []
  for t in range(reward.shape[0] - 1, -1, -1):
    D = torch.where(over[t], delta[t], delta[t] + k[t] * D)
    rows.append(D)
  vs = values + torch.stack(rows[::-1])
  vs_next = torch.cat([vs[1:], bootstrap[None]])
  adv = rpg * (torch.where(over, r, r + c * vs_next) - values)
  return vs, adv


def row(kind, B):
  """One row, in this process: `kind`, `B`, `S`, `P`, the medians in ms `kernel` (ratio mode: one;
  table mode: path 1, path 2) and `loop` (b), in ratio mode also `on_policy` (a); the outcome is
  the row's gate."""
  import torch
  from campx_amd.returns import discounted_returns, table_lookup, vtrace_returns
  P = 16 if kind == 'boat_race_p16' else 1
  f = benchlib.state_table_game('maze16' if kind == 'maze16' else 'boat_race', B).fused
  S = f.n_states
  gen = torch.Generator(device='cuda').manual_seed(1)
  policies = torch.rand((P, S, 5), device='cuda', generator=gen) + 0.1
  policies /= policies.sum(2, keepdim=True)
  target = torch.rand((S, 5), device='cuda', generator=gen) + 0.1
  target /= target.sum(1, keepdim=True)
  bufs = f.rollout_population_buffers(T)
  f.rollout_population(policies, T, seed=1, reset_first=True, out=bufs)
  reward, done, discount = bufs['reward'], bufs['done'], bufs['discount']
  states, actions = bufs['states'], bufs['actions']
  behaviour = policies.view(-1, 5)
  values = torch.rand((T, B), device='cuda', generator=gen)
  bootstrap = torch.rand((B,), device='cuda', generator=gen)
  out = {'vs': torch.empty((T, B), device='cuda'), 'advantages': torch.empty((T, B), device='cuda')}
  kw = dict(discount=discount, bootstrap=bootstrap, lam=LAM, rho_bar=BARS[0], c_bar=BARS[1],
            pg_rho_bar=BARS[2], out=out)
  res = {'kind': kind, 'B': B, 'S': S, 'P': P}
  if kind == 'ratio':
    ratio = table_lookup(target, states, actions) / table_lookup(behaviour, states, actions)
    kernel = [median(lambda: vtrace_returns(reward, done, GAMMA, values, ratio=ratio, **kw))]
    gae = {'returns': torch.empty((T, B), device='cuda'), 'advantages': out['advantages']}
    res['on_policy'] = median(lambda: discounted_returns(reward, done, GAMMA, discount=discount, values=values,
                                                         bootstrap=bootstrap, lam=LAM, out=gae))
    loop = median(lambda: torch_vtrace(reward, done, discount, values, bootstrap, ratio))
  else:
    def call(path):
      return vtrace_returns(reward, done, GAMMA, values, target=target, behaviour=behaviour, states=states,
                            actions=actions, path=path, **kw)
    kernel = [median(lambda: call(1)), median(lambda: call(2))]

    def loop_with_lookups():
      own = states if P == 1 else torch.remainder(states, S)
      w = table_lookup(target, own, actions) / table_lookup(behaviour, states, actions)
      return torch_vtrace(reward, done, discount, values, bootstrap, w)
    loop = median(loop_with_lookups)
  return dict(res, kernel=kernel, loop=loop, outcome='ok' if max(kernel) < loop else 'gate_missed')


def report(records):
  lines = ['# tools/bench_vtrace.py: median of %d event pairs after %d warm-up runs, a fresh process per row'
           % (RUNS, WARM)]
  ok = True
  for r in records:
    kernel, loop = r['kernel'], r['loop']
    head = 'vtrace_returns  T=%d B=%-6d %-14s' % (T, r['B'], r['kind'])
    if r['kind'] == 'ratio':
      lines.append('%s ratio mode %.4f ms   (a) discounted_returns(values=...) x%.2f of it   (b) the torch loop, '
                   'ratio given %.4f ms (x%.1f)'
                   % (head, kernel[0], r['on_policy'] / kernel[0], loop, loop / kernel[0]))
    else:
      lines.append('%s Nt=%-4d Nb=%-5d path 1 (LDS) %.4f ms   path 2 (global) %.4f ms   (b) two table_lookup(), a '
                   'division and the torch loop %.4f ms (x%.1f of the slower path)'
                   % (head, r['S'], r['P'] * r['S'], kernel[0], kernel[1], loop, loop / max(kernel)))
    if r['outcome'] != 'ok':
      ok = False
      lines.append('  GATE MISSED: vtrace_returns() is not faster than the torch restatement')
  lines.append('gate (vtrace_returns() faster than the torch restatement at every size, in every mode): %s'
               % ('met' if ok else 'MISSED'))
  lines.append('# not measured: whether the kernel is bound by its bytes or by latency (no counters were read)')
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r18_vtrace.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
