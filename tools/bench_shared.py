#!/usr/bin/env python3
"""`learn_shared()` measured: T frames of online Q-learning for P shared learners of n actors each
in ONE launch, beside what a user pays for the same frames today.

T = 1 000, B = 65 536.  Rows: the boat race and the 16x16 maze on their state tables, n = 1, 16, 256
and 1 024 actors per learner (P = B / n learners), each path forced where the plan allows it
(1 = tables and accumulators in LDS, 2 = in global memory).  Two baselines in the same process:
  * a torch restatement of the same T frames on the same device and game: per frame an
    epsilon-greedy action from `q[member]` (gather, argmax, rand), one `play()`, the TD errors, and
    their mean per (learner, state, action) through two `index_put_(accumulate=True)` - floats
    added in arrival order, so it does not repeat; it is the comparator for the time, not for the
    bits (tests/test_shared_learner.py has those);
  * `learn_tabular()` at the same B and T - a table per environment - for information only.

GATE: the launch is no slower than the torch loop, every row.  Rows, failures and exit statuses:
tools/benchlib.py.

Warm-up first, event pairs, the median of 15 launches and of 3 torch loops.

    python tools/bench_shared.py [out.txt]      # default: profiles/r19_shared.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 50     # torch loops of T frames
ACTORS = (1, 16, 256, 1024)
ROWS = tuple((name, n, path) for name in ('boat_race', 'maze16') for n in ACTORS for path in (1, 2))
ROW_SECONDS = 240          # a row builds one game and runs 36 launches and 3 050 torch frames: seconds
ALPHA, GAMMA, EPSILON = 0.1, 0.9, 0.1


def torch_frames(game, q, n, frames):
  """`frames` frames of synchronous epsilon-greedy Q-learning on `q` [P, S, 5], n environments per
  learner, in torch ops and one `play()` per frame."""
  import torch
  f = game.fused
  P, S = q.shape[0], q.shape[1]
  member = torch.arange(B, device='cuda') // n
  flat = q.view(-1)
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  ones = torch.ones((B,), device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    greedy = q[member, s].argmax(1)
    explore = torch.rand((B,), device='cuda') < EPSILON
    a = torch.where(explore, torch.randint(0, 5, (B,), device='cuda'), greedy)
    _, reward, discount = game.play(a.to(torch.int8))
    r = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    b = q[member, f.state.long()].max(1).values
    target = r + (GAMMA * discount) * b            # (a frame that ends the episode reports discount 0)
    at = (member * S + s) * 5 + a
    delta = target - flat[at]
    total = torch.zeros((P * S * 5,), device='cuda').index_put_((at,), delta, accumulate=True)
    count = torch.zeros((P * S * 5,), device='cuda').index_put_((at,), ones, accumulate=True)
    flat.add_(ALPHA * total / count.clamp_(min=1.0))


def row(name, n, path):
  """One row, in this process: `name`, `S`, `n`, `P`, `path`, `device`; skipped where the plan
  refuses the forced path, else `plan` (path, G, threads, LDS bytes, entries in LDS) and the medians
  `ours`, `loop` and `tabular` in ms, the outcome being the row's gate."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, B)
  f = game.fused
  S, P = f.n_states, B // n
  res = {'name': name, 'S': S, 'n': n, 'P': P, 'path': path, 'device': torch.cuda.get_device_name(0)}
  plan = (ctypes.c_int64 * 6)()
  if _hip.lib.campx_wide_shared_plan(S, int(f.has_perf), B, P, _hip.config_get('wide_lds_max'), path,
                                     plan) != 0:
    return dict(res, outcome='skipped')
  q = torch.zeros((P, S, 5), device='cuda')
  hyper = [torch.full((P,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  out = game.shared_learner_buffers(P, T, 100, path)
  ours = benchlib.median_ms(lambda: game.learn_shared(T, q, *hyper, seed=1, window=100, out=out, path=path),
                            RUNS, WARM)
  q.zero_()
  torch_frames(game, q, n, LOOP_WARM_FRAMES)
  loop = benchlib.median_ms(lambda: torch_frames(game, q, n, T), LOOP_RUNS)
  del q, out
  # for information: a table per environment, the same B and T
  q_each = torch.zeros((B, S, 5), device='cuda')
  each = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  bufs = game.learner_buffers(T, 100)
  tabular = benchlib.median_ms(lambda: game.learn_tabular(T, q_each, *each, seed=1, window=100, out=bufs),
                               RUNS, WARM)
  return dict(res, plan=list(plan), ours=ours, loop=loop, tabular=tabular,
              outcome='ok' if ours <= loop else 'gate_missed')


def report(records):
  lines = ['# tools/bench_shared.py: B = %d, T = %d; a process per row; event pairs, the median of %d '
           'launches after %d warm-up launches and of %d torch loops after %d warm-up frames; %s'
           % (B, T, RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, benchlib.device_of(records))]
  ok = True
  for r in records:
    if r['outcome'] == 'skipped':
      lines.append('%-10s S=%-4d n=%-4d P=%-5d  path %d does not apply (not one learner fits the LDS)'
                   % (r['name'], r['S'], r['n'], r['P'], r['path']))
      continue
    met = r['outcome'] == 'ok'
    ok = ok and met
    plan, ours, loop = r['plan'], r['ours'], r['loop']
    lines.append('%-10s S=%-4d n=%-4d P=%-5d  path %d (G %d, %d threads, %6d B LDS, entries %s)   learn_shared() %.3f ms '
                 '= %.2f us / frame   torch loop %.1f ms = %.1f us / frame (x%.0f)   learn_tabular() %.3f ms%s'
                 % (r['name'], r['S'], r['n'], r['P'], plan[0], plan[1], plan[2], plan[3],
                    'in LDS' if plan[4] else 'through L1 / L2', ours, ours * 1000 / T, loop, loop * 1000 / T,
                    loop / ours, r['tabular'], '' if met else '   GATE MISSED'))
  lines.append('gate (learn_shared() no slower than the torch loop of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r19_shared.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
