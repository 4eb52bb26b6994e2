#!/usr/bin/env python3
"""Sweeps of policy evaluation and value iteration on a state table measured, per sweep:
`WideGame.evaluate_policy()` / `value_iteration()` (csrc/k_plan.hip) with each path forced
(1 = all sweeps in one launch from LDS, where the table fits; 2 = one launch per sweep) and chosen
by the library (0), against the same sweep restated in torch on the same device in the same run:

    q = where(done, r, r + c * V[next.long()])        c = gamma * discount
    V = (w * q).sum(1) / w.sum(1)      or      V = q.max(1).values

(the restatement reorders the sums: it is the yardstick for time, tests/planning_reference.py the
one for bits).

Sizes: the boat race on its state table (8 states); synthetic tables of 1 940 states and of
4 400 000 states, the size of the 16x16 two-box sokoban's enumerated table - every state reachable,
next states uniform over the table, so the gathers of a sweep are as scattered as a table's can be.

GATE: path 0 is no slower per sweep than the torch restatement at every size, for both reductions
(exit status 1 otherwise; the table says where it is missed).  Also printed, for the record: the
bytes a sweep of the global path has to move (40 per state of entries, 20 of weights for a policy,
4 read and 4 written of values, 20 gathered) over its time, against a `fill_()` of 256 MiB.

Settled clocks (warm-up runs first), event pairs around SWEEPS sweeps, median of 15 runs.  Rows,
failures and exit statuses: tools/benchlib.py.

    python tools/bench_planning.py [out.txt]        # default: profiles/r11_planning.txt
"""
import sys
import types

import benchlib

sys.path.insert(0, benchlib.REPO)

RUNS, WARM, SWEEPS, GAMMA = 15, 5, 32, 0.99
ROWS = (('boat_race', 8), ('synthetic', 1940), ('synthetic', 4400000))
ROW_SECONDS = 900


def synthetic_table(S, seed=0):
  """A legal state table of S states with the attributes of a `tabulate.TracedGame` that the
  state-table tier reads: one hidden thing on a 4 x 4 board, state s reachable from state 0 through
  its parent (s - 1) // 5, every other entry uniform over the table, a tenth of those ending the
  episode."""
  import numpy as np
  rng = np.random.RandomState(seed)
  g = types.SimpleNamespace()
  g.rows, g.cols, g.n_states = 4, 4, S
  g.chars = [' ', '#']
  g.any_reward, g.has_perf = True, False
  board = np.full((4, 4), ord(' '), np.uint8)
  board[0, :] = ord('#')
  g.variants, g.backdrop = [board], board
  g.model_board = lambda cells, movers=True, variant=0: board.copy()
  g.mode_orders = g.variant_masks = None
  g.statics, g.pieces_as_mask = (), True
  g.movers, g.piece_cell, g.z_order = ['#'], [None], list(g.chars)
  g.st_variant = np.zeros(S, np.uint16)
  g.st_cells = rng.randint(0, 16, size=(S, 1)).astype(np.uint16)
  g.st_shows = np.zeros((S, 1), np.uint8)
  g.st_present = np.ones((S, 1), bool)
  g.init_cells = (int(g.st_cells[0, 0]),)
  nxt = rng.randint(0, S, size=S * 5)
  children = np.arange(1, S)
  nxt[children - 1] = children                  # entry (s - 1) of the flat table leads to s
  tree = np.zeros(S * 5, bool)
  tree[children - 1] = True
  g.st_next = nxt.reshape(S, 5).astype(np.int32)
  g.st_done = ((rng.rand(S * 5) < 0.1) & ~tree).reshape(S, 5).astype(np.uint8)
  g.st_reward = rng.choice(np.array([np.nan, 0.0, 1.0, -1.0, 0.1], np.float32), size=(S, 5))
  g.discount_list = [1.0] * 16
  g.st_dcode = np.zeros((S, 5), np.uint8)
  g.st_discount = np.where(g.st_done != 0, np.float32(0), np.float32(1)).astype(np.float32)
  g.st_perf = np.zeros((S, 5), np.int8)
  g.st_reached = np.ones((S, 5), bool)
  g.done_bytes = lambda: (g.st_done | (g.st_dcode << 4)).astype(np.uint8)
  return g


def row(kind, S):
  """One row, in this process: `kind`, `S`, `fill_gbs`, `device`, and for each reduction ('policy',
  'greedy') `<name>_torch`, `<name>_path0` .. `_path2` (None where the path does not fit) - medians
  in ms PER SWEEP -, `<name>_plan` and `<name>_max_diff`."""
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
    from campx_amd import wide
    game = wide.WideGame(types.SimpleNamespace(rows=4, cols=4), 1, 'cuda', synthetic_table(S))
  assert game.n_states == S
  tabs = game.table_arrays()
  nxt, done = tabs['next_state'].long(), tabs['done'] != 0
  r = torch.nan_to_num(tabs['reward'], nan=0.0)
  c = GAMMA * tabs['discount']
  w = torch.rand((S, 5), device='cuda').add_(0.5)
  total = w.sum(1)

  def torch_sweeps(policy):
    v = torch.zeros((S,), device='cuda')
    for _ in range(SWEEPS):
      q = torch.where(done, r, r + c * v[nxt])
      v = (w * q).sum(1) / total if policy else q.max(1).values
    return v

  res = {'kind': kind, 'S': S}
  for name, policy in (('policy', True), ('greedy', False)):
    out = game.sweep_buffers(SWEEPS, greedy=not policy)
    call = ((lambda path: game.evaluate_policy(w, GAMMA, SWEEPS, out=out, path=path)) if policy else
            (lambda path: game.value_iteration(GAMMA, SWEEPS, out=out, path=path)))
    want = torch_sweeps(policy)
    got = call(0)['values']
    res[name + '_max_diff'] = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
    res[name + '_torch'] = benchlib.median_ms(lambda: torch_sweeps(policy), RUNS, WARM) / SWEEPS
    plan = (ctypes.c_int64 * 4)()
    _hip.check(_hip.lib.campx_wide_sweeps_plan(S, 1 if policy else 0, 0, _hip.config_get('wide_lds_max'),
                                               0, plan), 'campx_wide_sweeps_plan')
    res[name + '_plan'] = int(plan[0])
    for path in (0, 1, 2):
      fits = _hip.lib.campx_wide_sweeps_plan(S, 1 if policy else 0, 0, _hip.config_get('wide_lds_max'),
                                             path, plan) == 0
      res['%s_path%d' % (name, path)] = (benchlib.median_ms(lambda: call(path), RUNS, WARM) / SWEEPS
                                         if fits else None)
  game.check_actions()
  big = torch.empty((256 << 20,), dtype=torch.uint8, device='cuda')
  res['fill_gbs'] = big.numel() / (benchlib.median_ms(lambda: big.fill_(1), RUNS, WARM) * 1e-3) / 1e9
  res['device'] = torch.cuda.get_device_name(0)
  return res


def fmt(v):
  return '    n/a   ' if v is None else '%10.5f' % v


def report(rows):
  lines = ['# tools/bench_planning.py: ms PER SWEEP (%d sweeps a call, gamma %.2f); median of %d event pairs '
           'after %d warm-up runs, a fresh process per row, %s'
           % (SWEEPS, GAMMA, RUNS, WARM, benchlib.device_of(rows)),
           '%-10s %8s %-7s | %10s | %10s %10s %10s | %4s | %8s | %9s %9s'
           % ('table', 'S', 'reduce', 'torch', 'path 0', 'LDS (1)', 'global (2)', 'auto', 'torch/0',
              'glb GB/s', 'fill GB/s')]
  ok = True
  for r in rows:
    for name, per_state in (('policy', 88), ('greedy', 68)):
      t0, tt = r[name + '_path0'], r[name + '_torch']
      met = t0 <= tt
      ok = ok and met
      gbs = r['S'] * per_state / (r[name + '_path2'] * 1e-3) / 1e9
      lines.append('%-10s %8d %-7s | %10.5f | %s %s %s | %4s | %8.2f | %9.1f %9.1f%s'
                   % (r['kind'], r['S'], name, tt, fmt(t0), fmt(r[name + '_path1']), fmt(r[name + '_path2']),
                      'LDS' if r[name + '_plan'] == 1 else 'glb', tt / t0, gbs, r['fill_gbs'],
                      '' if met else '   GATE MISSED: path 0 is slower than torch'))
      lines.append('#   values against the torch restatement, largest difference / largest |value|: %.2e'
                   % r[name + '_max_diff'])
  lines.append('gate (path 0 no slower per sweep than the torch restatement at every size): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r11_planning.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
