#!/usr/bin/env python3
"""The learner's step measured: `[T, B]` streams -> the gradient of the tabular policy-gradient
loss  -(log p[s_t, a_t] * w_t).sum(0).mean()  with respect to the table `p`, three ways:

  (1) as examples/reinforce_tabular.py does it: `.long()` twice, an advanced index, `log`,
      multiply, sum, `backward()` (whose index_put_ accumulates 6.5 M values into S x 5 addresses);
  (2) the same with `table_lookup(p, states, actions)` for the index;
  (3) `sum_by_state(states, actions, (w,))` and the loss over `[S, 5]`:
      -(log p * sums).sum() / B, `backward()`.

and, beside them, `sum_by_state()` alone with each accumulation path forced (1 = LDS where the
accumulators fit, 2 = global) and chosen by the library (0), and `table_lookup()` alone.

Sizes, T = 100: the boat race on its state table (8 states; the streams of a real
`rollout_policy()` under a uniform policy) at B = 4 096 and 65 536; synthetic uniform states and
actions over S = 1 940 and S = 4 400 000 at B = 65 536.

GATE: form (3) is no slower than form (1) at every size (exit status 1 otherwise; the table says
where it is missed).  Form (1) is measured in the same run.

Settled clocks (warm-up runs first), event pairs, median of 25 runs.  Rows, failures and exit
statuses: tools/benchlib.py.

    python tools/bench_learner.py [out.txt]        # default: profiles/r10_learner.txt
"""
import functools
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, T = 25, 10, 100
ROWS = (('boat_race', 8, 4096), ('boat_race', 8, 65536), ('uniform', 1940, 65536),
        ('uniform', 4400000, 65536))
ROW_SECONDS = 900
median = functools.partial(benchlib.median_ms, runs=RUNS, warm=WARM)


def row(kind, S, B):
  """One row, in this process: `kind`, `S`, `B`, `plan`, `device`, `max_diff_2`, `max_diff_3`, and
  the medians in ms `form1` .. `form3`, `sums_path0` .. `sums_path2` (None where the path does not
  fit), `sums_k0` and `lookup`."""
  import ctypes
  import torch
  from campx_amd import _hip
  from campx_amd.returns import sum_by_state, table_lookup
  if kind == 'boat_race':
    from campx_amd.games import boat_race
    game = boat_race.build(B, 'cuda')
    game.use_state_table()
    game.its_showtime()
    assert game.fused.n_states == S
    bufs = game.rollout_policy_buffers(T)
    game.rollout_policy(torch.ones((S, 5), device='cuda'), T, seed=1, reset_first=True, out=bufs)
    states, actions = bufs['states'], bufs['actions']            # padded rows, as the rollout wrote them
  else:
    gen = torch.Generator(device='cuda').manual_seed(S)
    states = torch.randint(0, S, (T, B), generator=gen, device='cuda', dtype=torch.int32)
    actions = torch.randint(0, 5, (T, B), generator=gen, device='cuda').to(torch.int8)
  w = torch.randn((T, B), device='cuda')
  p = torch.rand((S, 5), device='cuda').add_(0.5).requires_grad_()

  def form1():
    p.grad = None
    log_probs = torch.log(p[states.long(), actions.long()])
    (-(log_probs * w).sum(0).mean()).backward()

  def form2():
    p.grad = None
    log_probs = torch.log(table_lookup(p, states, actions))
    (-(log_probs * w).sum(0).mean()).backward()

  K = 1
  out = {'raw': torch.empty((K + 1, S, 5), dtype=torch.int64, device='cuda'),
         'skipped': torch.empty((1,), dtype=torch.int64, device='cuda'),
         'clamped': torch.empty((1,), dtype=torch.int64, device='cuda')}

  def form3():
    p.grad = None
    sums = sum_by_state(states, actions, (w,), n_states=S, out=out)
    (-(torch.log(p) * sums['sums'][0].float()).sum() / B).backward()

  res = {'kind': kind, 'S': S, 'B': B}
  form1()
  g1 = p.grad.clone()
  form2()
  g2 = p.grad.clone()
  form3()
  g3 = p.grad.clone()
  scale = float(g1.abs().max())
  res['max_diff_2'] = float((g2 - g1).abs().max()) / scale
  res['max_diff_3'] = float((g3 - g1).abs().max()) / scale
  res['form1'] = median(form1)
  res['form2'] = median(form2)
  res['form3'] = median(form3)
  plan = (ctypes.c_int64 * 8)()
  _hip.check(_hip.lib.campx_state_sums_plan(S, 5, K, B, T, 24, 0, plan), 'campx_state_sums_plan')
  res['plan'] = [int(v) for v in plan]
  for path in (0, 1, 2):
    if path == 1 and S * 5 * (K + 1) * 8 > _hip.SUMS_LDS_BUDGET:
      res['sums_path1'] = None
      continue
    res['sums_path%d' % path] = median(
        lambda: _hip.ops.state_sums(states, actions, [w], S, 5, 24, False, path, out['raw'],
                                    out['skipped'], out['clamped']))
  res['sums_k0'] = median(
      lambda: _hip.ops.state_sums(states, actions, [], S, 5, 24, False, 0, out['raw'][:1],
                                  out['skipped'], out['clamped']))
  x = torch.empty((T, B), device='cuda')
  pd = p.detach()
  res['lookup'] = median(lambda: _hip.ops.table_lookup(pd, states, actions, x, None))
  res['device'] = torch.cuda.get_device_name(0)
  return res


def fmt(v):
  return '   n/a  ' if v is None else '%8.4f' % v


def report(rows):
  lines = ['# tools/bench_learner.py: [T, B] streams -> gradient of the tabular loss, T = %d; median ms '
           'of %d event pairs after %d warm-up runs, a fresh process per row, %s'
           % (T, RUNS, WARM, benchlib.device_of(rows)),
           '# (1) .long() + advanced index + backward   (2) table_lookup() + backward   '
           '(3) sum_by_state() + loss over [S, 5] + backward',
           '%-10s %9s %6s | %8s %8s %8s | %7s | %-24s | %8s %8s %8s %8s | %8s'
           % ('streams', 'S', 'B', '(1)', '(2)', '(3)', '(1)/(3)', 'plan: path copies LDS B',
              'sums 0', 'sums LDS', 'sums glb', 'K=0', 'lookup')]
  ok = True
  for r in rows:
    met = r['form3'] <= r['form1']
    ok = ok and met
    lines.append('%-10s %9d %6d | %8.4f %8.4f %8.4f | %7.2f | %-24s | %s %s %s %s | %s%s'
                 % (r['kind'], r['S'], r['B'], r['form1'], r['form2'], r['form3'],
                    r['form1'] / r['form3'],
                    '%s x%d %d' % ('LDS' if r['plan'][0] == 1 else 'global', r['plan'][1], r['plan'][5]),
                    fmt(r['sums_path0']), fmt(r['sums_path1']), fmt(r['sums_path2']), fmt(r['sums_k0']),
                    fmt(r['lookup']), '' if met else '   GATE MISSED: (3) is slower than (1)'))
    lines.append('#   gradients against (1), largest difference / largest |gradient|: (2) %.2e  (3) %.2e'
                 % (r['max_diff_2'], r['max_diff_3']))
  lines.append('gate (form (3) no slower than form (1) at every size): %s' % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r10_learner.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
