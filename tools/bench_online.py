#!/usr/bin/env python3
"""`learn_tabular()` measured: T frames of online Q-learning for B independent learners in ONE
launch, beside what a user pays for the same frames today.

T = 1 000, B = 65 536.  Rows: the boat race on its state table with both paths forced (1 = the
learners' tables in LDS, 2 = through L1 / L2) and the 16x16 maze on the global path (its 159 states
do not fit path 1).  The comparator of every row is a torch restatement of the same T frames on the
same device and the same game: per frame an epsilon-greedy action from `q` (gather, argmax, rand),
one `play()`, and the update through gather / `scatter_` on `q` - a handful of torch ops and one
launch of the engine per frame.  It draws torch's random numbers, not the kernel's: it is the
comparator for the time, not for the bits (tests/test_learner.py has those).

GATE: the launch is no slower than the torch loop, every row.  Rows, failures and exit statuses:
tools/benchlib.py.

Warm-up first, event pairs, the median of 15 launches and of 3 torch loops.

    python tools/bench_online.py [out.txt]      # default: profiles/r15_online.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 50     # torch loops of T frames
ROWS = (('boat_race', 1), ('boat_race', 2), ('maze16', 2))
ROW_SECONDS = 240          # a row builds one game and runs 18 launches and 3 050 torch frames: seconds
ALPHA, GAMMA, EPSILON = 0.1, 0.9, 0.1


def torch_frames(game, q, frames):
  """`frames` frames of epsilon-greedy Q-learning on `q` [B, S, 5], a learner per environment, in
  torch ops and one `play()` per frame."""
  import torch
  f = game.fused
  lanes = torch.arange(B, device='cuda')
  flat = q.view(B, -1)
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    greedy = q[lanes, s].argmax(1)
    explore = torch.rand((B,), device='cuda') < EPSILON
    a = torch.where(explore, torch.randint(0, 5, (B,), device='cuda'), greedy)
    _, reward, discount = game.play(a.to(torch.int8))
    r = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    b = q[lanes, f.state.long()].max(1).values
    target = r + (GAMMA * discount) * b            # (a frame that ends the episode reports discount 0)
    at = (s * 5 + a)[:, None]
    old = flat.gather(1, at)
    flat.scatter_(1, at, old + ALPHA * (target[:, None] - old))


def row(name, path):
  """One row, in this process: `name`, `S`, `plan` (path, LDS bytes, -, entries in LDS), the medians
  `ours` and `loop` in ms, `device`; the outcome is the row's gate."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, B)
  f = game.fused
  S = f.n_states
  plan = (ctypes.c_int64 * 4)()
  _hip.check(_hip.lib.campx_wide_learn_plan(S, int(f.has_perf), B, _hip.config_get('wide_lds_max'),
                                            path, plan), 'campx_wide_learn_plan')
  q = torch.zeros((B, S, 5), device='cuda')
  hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA, GAMMA, EPSILON)]
  out = game.learner_buffers(T, 100)
  ours = benchlib.median_ms(lambda: game.learn_tabular(T, q, *hyper, seed=1, window=100, out=out, path=path),
                            RUNS, WARM)
  q.zero_()
  torch_frames(game, q, LOOP_WARM_FRAMES)
  loop = benchlib.median_ms(lambda: torch_frames(game, q, T), LOOP_RUNS)
  return {'name': name, 'S': S, 'plan': list(plan), 'ours': ours, 'loop': loop,
          'device': torch.cuda.get_device_name(0), 'outcome': 'ok' if ours <= loop else 'gate_missed'}


def report(records):
  lines = ['# tools/bench_online.py: a process per row; event pairs, the median of %d launches after %d '
           'warm-up launches and of %d torch loops after %d warm-up frames; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, benchlib.device_of(records))]
  ok = True
  for r in records:
    met = r['outcome'] == 'ok'
    ok = ok and met
    plan, ours, loop = r['plan'], r['ours'], r['loop']
    lines.append('%-10s S=%-4d B=%d T=%d  path %d (%6d B LDS, entries %s)   learn_tabular() %.3f ms = %.2f us / frame   '
                 'torch loop %.1f ms = %.1f us / frame (x%.0f)%s'
                 % (r['name'], r['S'], B, T, plan[0], plan[1], 'in LDS' if plan[3] else 'through L1 / L2', ours,
                    ours * 1000 / T, loop, loop * 1000 / T, loop / ours, '' if met else '   GATE MISSED'))
  lines.append('gate (learn_tabular() no slower than the torch loop of the same frames, every row): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r15_online.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
