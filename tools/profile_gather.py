#!/usr/bin/env python3
"""The program behind profiles/r07_gather_rocprofv3.txt: 60 x `render_frames()` and 60 x
`index_select` from the materialised observations, at 4 096 and 65 536 random (frame, environment)
pairs of a 100-frame boat-race trace of 65 536 environments.

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/profile_gather.py
    python tools/rocpd_summary.py DIR > profiles/r07_gather_rocprofv3.txt
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from campx_amd.games import boat_race  # noqa: E402


def main():
  B, T = 65536, 100
  game = boat_race.build(batch=B, device='cuda')
  game.its_showtime()
  f = game.fused
  f.validate_actions = False
  out = f.rollout(torch.randint(0, 5, (T, B), dtype=torch.int8, device='cuda'), reset_first=True)
  row = f.n_layers * f.rows * f.cols
  flat_obs = out['obs'].view(T * B, row)
  for N in (4096, 65536):
    t = torch.randint(0, T, (N,), device='cuda')
    e = torch.randint(0, B, (N,), device='cuda')
    flat = t * B + e
    dst = torch.empty((N, f.n_layers, f.rows, f.cols), dtype=torch.int8, device='cuda')
    sel = torch.empty((N, row), dtype=torch.int8, device='cuda')
    for _ in range(60):
      f.render_frames(out['trace'], t, e, out=dst)
    for _ in range(60):
      torch.index_select(flat_obs, 0, flat, out=sel)
    torch.cuda.synchronize()


if __name__ == '__main__':
  main()
