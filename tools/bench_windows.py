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

One fresh process per row; settled clocks (warm-up runs first), event pairs, median of 25 runs.

    python tools/bench_windows.py [out.txt]        # default: profiles/r13_windows.txt
"""
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

RUNS, WARM, T, B = 25, 10, 100, 4096
ROWS = [('maze16', 7, 7, 4096), ('maze16', 7, 7, 1048576), ('maze16', 5, 5, 4096),
        ('maze16', 5, 5, 1048576), ('boat_race', 3, 3, 4096), ('boat_race', 3, 3, 1048576),
        ('maze16', 7, 7, 0), ('maze16', 5, 5, 0)]          # N = 0: all states
GATED = {('maze16', 7, 7, 1048576), ('maze16', 5, 5, 1048576)}


def median_us(torch, fn):
  for _ in range(WARM):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(RUNS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
  return statistics.median(times)


def row(name, h, w, N):
  import torch
  import windows_reference as ref
  from campx_amd.games import boat_race, maze
  from campx_amd.windows import Window
  if name == 'boat_race':
    game = boat_race.build(B, 'cuda')
    game.use_state_table()
  else:
    game = maze.build(16, 16, batch=B, device='cuda')
  game.its_showtime()
  f = game.fused
  f.validate_actions = False
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
    what = 'render_frame_windows N=%-8d' % N
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
    what = 'render_state_windows S=%-7d' % N
  ours()
  assert torch.equal(out, baseline())          # the same tensor, or the row means nothing
  a = median_us(torch, ours)
  b = median_us(torch, baseline)
  mine, theirs = N * L * h * w, N * L * H * W
  print('%s %-9s %dx%d  window %10.3f MB %10.1f us (%.3f TB/s)   full + pad + slice %10.3f MB '
        '%10.1f us (%.3f TB/s)   baseline / window %.2f'
        % (what, name, h, w, mine / 1e6, a, mine / a / 1e6, theirs / 1e6, b, theirs / b / 1e6, b / a))
  return a <= b


def main():
  if len(sys.argv) > 1 and sys.argv[1] == '--row':
    name, h, w, N = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    return 0 if row(name, h, w, N) else 3
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'r13_windows.txt')
  lines = ['# tools/bench_windows.py: one process per row, median of %d event pairs after %d warm-up '
           'runs; int8, traces of %d frames x %d environments' % (RUNS, WARM, T, B)]
  ok = True
  for name, h, w, N in ROWS:
    done = subprocess.run([sys.executable, os.path.abspath(__file__), '--row', name, str(h), str(w), str(N)],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    lines.append(done.stdout.rstrip())
    if done.returncode not in (0, 3):
      lines.append('  ROW FAILED (exit status %d)' % done.returncode)
      lines.append(done.stderr.rstrip())
      ok = False
      break                      # nothing more is started on the device after a failure
    if done.returncode == 3 and (name, h, w, N) in GATED:
      lines.append('  GATE MISSED: the window call is slower than render_frames() + pad + slice')
      ok = False
  lines.append('gate (window call no slower than the baseline at N = 1 048 576, both maze windows): %s'
               % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
