#!/usr/bin/env python3
"""Observation windows measured beside the only other way to get the same tensor.

`render_frame_windows()` of N sampled (frame, environment) pairs of a 100-frame trace of 4 096
environments - the 16x16 maze with a 7x7 and a 5x5 egocentric window (wall-padded), the boat race
on its state table with 3x3 - at N = 4 096 and 1 048 576, int8; and `render_state_windows()` of
all states of the maze.  Each beside

  * `render_frames()` / `render_states()` of the full observations followed by the torch pad and
    slice of tests/windows_reference.py, on the same indices: what a caller does without the window
    kernel.  Bytes written, microseconds and TB/s are reported for both (the baseline's bytes are
    the full observations it has to write first; its pad and slice traffic comes on top).

GATE: at N = 1 048 576 the window call is no slower than that baseline for both maze windows
(exit status 1 otherwise).  N = 4 096 and the state rows are launch-bound: there to be read.

Settled clocks (warm-up runs first), event pairs, median of 25 runs.  Rows, failures and exit
statuses: tools/benchlib.py.

    python tools/bench_windows.py [out.txt]        # default: profiles/r13_windows.txt
"""
import os
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)
sys.path.insert(0, os.path.join(benchlib.REPO, 'tests'))

RUNS, WARM, T, B = 25, 10, 100, 4096
ROWS = [('maze16', 7, 7, 4096), ('maze16', 7, 7, 1048576), ('maze16', 5, 5, 4096),
        ('maze16', 5, 5, 1048576), ('boat_race', 3, 3, 4096), ('boat_race', 3, 3, 1048576),
        ('maze16', 7, 7, 0), ('maze16', 5, 5, 0)]          # N = 0: all states
GATED = {('maze16', 7, 7, 1048576), ('maze16', 5, 5, 1048576)}
ROW_SECONDS = 300


def row(name, h, w, N):
  """One row, in this process: `name`, `h`, `w`, `N` (pairs, or the states where 0 was asked for),
  `states` (a row of all states), the bytes `mine` and `theirs` and the medians `ours` and `baseline`
  in MICROSECONDS; a GATED row whose window call is the slower one answers gate_missed."""
  import torch
  import windows_reference as ref
  from campx_amd.windows import Window
  gated = (name, h, w, N) in GATED
  f = benchlib.state_table_game(name, B).fused
  L, H, W = f.n_layers, f.rows, f.cols
  thing = f.chars[int(f.spec.dyn_layer[0])]
  pad = f.chars[int(f.spec.static_top_layer[0])]
  win = Window(h, w, thing, pad=pad)
  where = win.resolve(f.chars, f.spec)
  if N:
    weights = torch.ones((f.n_states, 5), device='cuda')
    trace = f.rollout_policy(weights, T, seed=1, reset_first=True)['trace']
    gen = torch.Generator().manual_seed(N)
    t = torch.randint(0, T, (N,), generator=gen).cuda()
    e = torch.randint(0, B, (N,), generator=gen).cuda()
    out = torch.empty((N, L, h, w), dtype=torch.int8, device='cuda')
    full = torch.empty((N, L, H, W), dtype=torch.int8, device='cuda')
    entries = trace[where.thing]

    def ours():
      f.render_frame_windows(trace, t, e, win, out=out)

    def baseline():
      f.render_frames(trace, t, e, out=full)
      r0, c0 = ref.centres(entries[t, e], W, H * W, h, w)
      return ref.crop(full, r0, c0, h, w, where.pad_layer)
    states = False
  else:
    N = f.n_states
    out = torch.empty((N, L, h, w), dtype=torch.int8, device='cuda')
    full = torch.empty((N, L, H, W), dtype=torch.int8, device='cuda')
    off = (N * 5 * 8 + 15) // 16 * 16
    entries = f._tables[off:off + N * 16].view(torch.int16).view(N, 8)[:, where.thing]

    def ours():
      f.render_state_windows(win, out=out)

    def baseline():
      f.render_states(out=full)
      r0, c0 = ref.centres(entries, W, H * W, h, w)
      return ref.crop(full, r0, c0, h, w, where.pad_layer)
    states = True
  ours()
  assert torch.equal(out, baseline())          # the same tensor, or the row means nothing
  a = benchlib.median_ms(ours, RUNS, WARM) * 1e3
  b = benchlib.median_ms(baseline, RUNS, WARM) * 1e3
  return {'name': name, 'h': h, 'w': w, 'N': N, 'states': states, 'mine': N * L * h * w,
          'theirs': N * L * H * W, 'ours': a, 'baseline': b,
          'outcome': 'gate_missed' if gated and a > b else 'ok'}


def report(records):
  lines = ['# tools/bench_windows.py: one process per row, median of %d event pairs after %d warm-up '
           'runs; int8, traces of %d frames x %d environments' % (RUNS, WARM, T, B)]
  ok = True
  for r in records:
    what = ('render_state_windows S=%-7d' if r['states'] else 'render_frame_windows N=%-8d') % r['N']
    mine, theirs, a, b = r['mine'], r['theirs'], r['ours'], r['baseline']
    lines.append('%s %-9s %dx%d  window %10.3f MB %10.1f us (%.3f TB/s)   full + pad + slice %10.3f MB '
                 '%10.1f us (%.3f TB/s)   baseline / window %.2f'
                 % (what, r['name'], r['h'], r['w'], mine / 1e6, a, mine / a / 1e6, theirs / 1e6, b,
                    theirs / b / 1e6, b / a))
    if r['outcome'] != 'ok':
      lines.append('  GATE MISSED: the window call is slower than render_frames() + pad + slice')
      ok = False
  lines.append('gate (window call no slower than the baseline at N = 1 048 576, both maze windows): %s'
               % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  records, broke = benchlib.run_rows(__file__, ROWS, ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(argv, 'r13_windows.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
