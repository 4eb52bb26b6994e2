#!/usr/bin/env python3
"""`render_states()` and `discounted_returns()` measured, each beside what it must beat or match.

`render_states()` - all states of the boat race on its state table (8), of the 16x16 maze (159)
and of the 16x16 two-box sokoban (4.4 M), int8 and bf16, into one buffer allocated once:

  * against `fill_` of the same buffer: the render kernel behind it reaches 0.93-0.99 of a fill in
    rollouts, so the ratio says what the one-frame trace in front of it and the shape (one frame
    of N rows) cost.  The two small games are launch-bound: their ratio is one of launch counts
    (the rows kernel + the render against one fill), reported as it comes.

`discounted_returns()` - T = 100 at B = 4 096 and 65 536, on the padded buffers of
`rollout_policy_buffers()`, with and without `values`:

  * against the reversed torch loop of examples/reinforce_tabular.py:47-51 on the same buffers
    (returns only: it has no episode ends, no NaN rewards and no advantages).
  GATE: the kernel is faster at every size measured (exit status 1 otherwise).

Settled clocks (warm-up runs first), event pairs, median of 25 runs.

    python tools/bench_states.py [out.txt]        # default: profiles/r09_states.txt
"""
import functools
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)
import torch  # noqa: E402

from campx_amd.games import sokoban  # noqa: E402
from campx_amd.returns import discounted_returns  # noqa: E402

RUNS, WARM, T = 25, 10, 100
median = functools.partial(benchlib.median_ms, runs=RUNS, warm=WARM)


def build(name, B):
  if name != 'sokoban16':
    return benchlib.state_table_game(name, B)
  game = sokoban.build(batch=B, device='cuda', level=3)
  game.its_showtime()
  game.fused.validate_actions = False
  return game


def states_point(name, lines):
  game = build(name, 64)
  f = game.fused
  S, R = f.n_states, f.n_layers * f.rows * f.cols
  for dtype in (torch.int8, torch.bfloat16):
    out = torch.empty((S, f.n_layers, f.rows, f.cols), dtype=dtype, device='cuda')
    render = median(lambda: f.render_states(obs_dtype=dtype, out=out))
    fill = median(lambda: out.fill_(1))
    nbytes = S * R * out.element_size()
    lines.append('render_states  %-10s S=%-8d %-8s %9.3f MB  %.4f ms (%.2f TB/s)   fill_ %.4f ms   '
                 'fill_ / render_states %.2f'
                 % (name, S, str(dtype).replace('torch.', ''), nbytes / 1e6, render,
                    nbytes / render / 1e9, fill, fill / render))
    del out
  del game
  torch.cuda.empty_cache()


def returns_point(B, lines):
  game = build('boat_race', B)
  f = game.fused
  weights = torch.ones((f.n_states, 5), device='cuda')
  bufs = f.rollout_policy_buffers(T)
  f.rollout_policy(weights, T, seed=1, reset_first=True, out=bufs)
  reward, done, discount = bufs['reward'], bufs['done'], bufs['discount']
  values = torch.rand((T, B), device='cuda')
  bootstrap = torch.rand((B,), device='cuda')
  out = {'returns': torch.empty((T, B), device='cuda'), 'advantages': torch.empty((T, B), device='cuda')}
  plain = median(lambda: discounted_returns(reward, done, 0.99, out={'returns': out['returns']}))
  full = median(lambda: discounted_returns(reward, done, 0.99, discount=discount, values=values,
                                              bootstrap=bootstrap, lam=0.95, out=out))

  def loop():
    returns, running = [], torch.zeros(B, device='cuda')
    for r in reversed(list(reward)):
      running = r + 0.99 * running
      returns.append(running)
    return torch.stack(returns[::-1])
  host = median(loop)
  lines.append('discounted_returns  T=%d B=%-6d  returns %.4f ms   with discount, values, bootstrap '
               '%.4f ms   the reversed torch loop %.4f ms (x%.1f)'
               % (T, B, plain, full, host, host / plain))
  del game, bufs
  torch.cuda.empty_cache()
  return max(plain, full) < host


def main():
  path = benchlib.out_path(sys.argv[1:], 'r09_states.txt')
  lines = ['# tools/bench_states.py: median of %d event pairs after %d warm-up runs, %s'
           % (RUNS, WARM, torch.cuda.get_device_name(0))]
  for name in ('boat_race', 'maze16', 'sokoban16'):
    states_point(name, lines)
  ok = True
  for B in (4096, 65536):
    if not returns_point(B, lines):
      ok = False
      lines.append('  GATE MISSED: discounted_returns() is not faster than the torch loop')
  lines.append('gate (discounted_returns() faster than the reversed torch loop at every size): %s'
               % ('met' if ok else 'MISSED'))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
