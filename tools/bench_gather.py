#!/usr/bin/env python3
"""Trace-only rollouts and the gather render, measured (numbers are recorded, not gated).

  * `rollout_trace()` beside `rollout()`, ms per 100 frames: boat race B = 65 536, sokoban B = 131 072.
  * `render_frames()` at N = 4 096 / 65 536 / 1 048 576 random (frame, environment) pairs of the
    boat race, int8 and bf16, plain and streaming stores, beside what a user can do without it -
    `obs.view(T * B, -1).index_select(0, flat)` from a materialised observation buffer - and
    beside `fill_` of the same output bytes (the store ceiling of a plain torch kernel).

Settled clocks (warm-up launches first), event pairs, median of 25 runs.

    python tools/bench_gather.py [out.txt]        # default: profiles/r07_gather.txt
"""
import functools
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)
import torch  # noqa: E402

from campx_amd import fused  # noqa: E402
from campx_amd.games import boat_race, sokoban  # noqa: E402

RUNS, WARM = 25, 10
median = functools.partial(benchlib.median_ms, runs=RUNS, warm=WARM)


def rollouts(lines):
  for name, build, B in (('boat_race', boat_race.build, 65536), ('sokoban', sokoban.build, 131072)):
    game = build(batch=B, device='cuda')
    game.its_showtime()
    f = game.fused
    f.validate_actions = False
    T = 100
    acts = torch.randint(0, 5, (T, B), dtype=torch.int8, device='cuda')
    full, lean = f.rollout_buffers(T), f.rollout_trace_buffers(T)
    a = median(lambda: f.rollout(acts, out=full, reset_first=True))
    b = median(lambda: f.rollout_trace(acts, out=lean, reset_first=True))
    row = f.n_layers * f.rows * f.cols
    lines.append('%-10s B=%-7d T=100  rollout() %.4f ms (%.1f MB obs)   rollout_trace() %.4f ms (%.1f MB trace)' % (
        name, B, a, row * B * T / 1e6, b, f.n_dyn * B * T / 1e6))
    del full, lean, game
    torch.cuda.empty_cache()


def gathers(lines):
  B, T = 65536, 100
  game = boat_race.build(batch=B, device='cuda')
  game.its_showtime()
  f = game.fused
  f.validate_actions = False
  acts = torch.randint(0, 5, (T, B), dtype=torch.int8, device='cuda')
  out = f.rollout(acts, reset_first=True)
  row = f.n_layers * f.rows * f.cols
  for dtype in (torch.int8, torch.bfloat16):
    obs = out['obs'] if dtype == torch.int8 else out['obs'].to(dtype)
    flat_obs = obs.view(T * B, row)
    for N in (4096, 65536, 1048576):
      t = torch.randint(0, T, (N,), device='cuda')
      e = torch.randint(0, B, (N,), device='cuda')
      flat = t * B + e
      dst = torch.empty((N, f.n_layers, f.rows, f.cols), dtype=dtype, device='cuda')
      sel = torch.empty((N, row), dtype=dtype, device='cuda')
      got, shipped = {}, fused.GATHER_STREAMING
      try:
        for streaming in (False, True):
          fused.GATHER_STREAMING = streaming
          got[streaming] = median(lambda: f.render_frames(out['trace'], t, e, out=dst))
      finally:
        fused.GATHER_STREAMING = shipped
      assert torch.equal(dst.view(N, row), flat_obs.index_select(0, flat))
      sel_ms = median(lambda: torch.index_select(flat_obs, 0, flat, out=sel))
      fill_ms = median(lambda: dst.fill_(1))
      nbytes = N * row * dst.element_size()
      lines.append('boat_race %-8s N=%-8d %7.1f MB  render_frames plain %.4f ms (%.2f TB/s)  streaming %.4f ms (%.2f TB/s)'
                   '  index_select %.4f ms (%.2f TB/s)  fill_ %.4f ms (%.2f TB/s)' % (
                       str(dtype).replace('torch.', ''), N, nbytes / 1e6, got[False], nbytes / got[False] / 1e9,
                       got[True], nbytes / got[True] / 1e9, sel_ms, nbytes / sel_ms / 1e9, fill_ms,
                       nbytes / fill_ms / 1e9))
    del obs, flat_obs


def main():
  path = benchlib.out_path(sys.argv[1:], 'r07_gather.txt')
  lines = ['# tools/bench_gather.py on %s: median of %d runs after %d warm-up ones, event pairs' % (
      torch.cuda.get_device_name(0), RUNS, WARM)]
  rollouts(lines)
  gathers(lines)
  text = '\n'.join(lines) + '\n'
  with open(path, 'w') as f:
    f.write(text)
  print(text)


if __name__ == '__main__':
  main()
