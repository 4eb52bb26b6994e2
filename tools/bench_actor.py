#!/usr/bin/env python3
"""`learn_actor_critic()` measured: T frames of one-step actor-critic - a softmax policy and a
critic per learner - for B independent learners in ONE launch, beside `learn_tabular()` on the same
game and beside what a user pays for the same frames without it.

T = 1 000, B = 65 536, the boat race (8 states) and the 16x16 maze (159 states).  Per game:
  - `learn_tabular()`, planned, for scale: the ratio is what the five exponent rules, the five
    divisions and the second table of a frame cost over the value-based frame - recorded, not gated;
  - the torch restatement on the same device: per frame `softmax_weights()` of the states' rows, the
    threshold compare on a uniform draw, one `play()`, gather / `scatter_` on `values`, and a
    gather / `scatter_` of the whole row on `prefs`.  It draws torch's random numbers: the comparator
    for the time, not for the bits (tests/test_actor_critic.py has those);
  - `learn_actor_critic()` planned, and with each path forced where the plan takes it.

GATE: every `learn_actor_critic()` row is no slower than the torch loop of its game.  Rows, failures
and exit statuses: tools/benchlib.py.

Warm-up first, event pairs, the median of 15 launches and of 3 torch loops.

    python tools/bench_actor.py [out.txt] [--games boat_race,maze16]     # default: profiles/r24_actor.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 20     # torch loops of T frames
GAMES = ('boat_race', 'maze16')
ROW_SECONDS = 300
ALPHA_ACTOR, ALPHA_CRITIC, GAMMA, EPSILON = 0.1, 0.1, 0.9, 0.1


def torch_frames(game, prefs, values, frames):
  """`frames` frames of one-step actor-critic, a learner per environment, in torch ops and one
  `play()` per frame."""
  import torch
  from campx_amd.returns import softmax_weights
  f = game.fused
  lanes = torch.arange(B, device='cuda')
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    h = prefs[lanes, s]
    w = softmax_weights(h)
    c = w.cumsum(1)
    r = torch.rand((B, 1), device='cuda') * c[:, 4:]
    a = (r >= c[:, :4]).sum(1)
    v_s = values.gather(1, s[:, None])
    _, reward, discount = game.play(a.to(torch.int8))
    rew = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    v_n = values.gather(1, f.state.long()[:, None])[:, 0]
    delta = (rew + (GAMMA * discount) * v_n)[:, None] - v_s      # (an episode's last frame reports discount 0)
    values.scatter_(1, s[:, None], v_s + ALPHA_CRITIC * delta)
    grad = torch.nn.functional.one_hot(a, 5) - w / c[:, 4:]
    prefs[lanes, s] = h + (ALPHA_ACTOR * delta) * grad


def row(name, what, path):
  """One row, in this process: `name`, `S`, `what` ('torch', 'tabular' or 'actor'), the forced `path`
  (0: planned), the median `ms` of `runs` calls, `device`; for 'actor' also `plan`."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, B)
  f = game.fused
  S = f.n_states
  res = {'name': name, 'S': S, 'what': what, 'path': path, 'device': torch.cuda.get_device_name(0)}
  prefs = torch.zeros((B, S, 5), device='cuda')
  values = torch.zeros((B, S), device='cuda')
  if what == 'torch':
    torch_frames(game, prefs, values, LOOP_WARM_FRAMES)
    loop = lambda: torch_frames(game, prefs, values, T)
    return dict(res, runs=LOOP_RUNS, ms=benchlib.median_ms(loop, LOOP_RUNS))
  out = game.learner_buffers(T, 100)
  if what == 'tabular':
    hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA_ACTOR, GAMMA, EPSILON)]
    launch = lambda: game.learn_tabular(T, prefs, *hyper, seed=1, window=100, out=out)
  else:
    hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA_ACTOR, ALPHA_CRITIC, GAMMA)]
    launch = lambda: game.learn_actor_critic(T, prefs, values, *hyper, seed=1, window=100, out=out,
                                             path=path)
    plan = (ctypes.c_int64 * 4)()
    _hip.lib.campx_wide_actor_plan(S, int(f.has_perf), B, _hip.config_get('wide_lds_max'), path, plan)
    res['plan'] = list(plan)
  return dict(res, runs=RUNS, ms=benchlib.median_ms(launch, RUNS, WARM))


def rows_of(name):
  """The rows of a game; a forced path is listed only if the plan takes it (host arithmetic)."""
  from campx_amd import _hip
  S, perf = {'boat_race': (8, 1), 'maze16': (159, 0)}[name]
  plan = (ctypes.c_int64 * 4)()
  paths = [0] + [path for path in (1, 2) if _hip.lib.campx_wide_actor_plan(
      S, perf, B, _hip.config_get('wide_lds_max'), path, plan) == 0]
  return [(name, 'tabular', 0), (name, 'torch', 0)] + [(name, 'actor', path) for path in paths]


def report(records):
  """A game's 'tabular' and 'torch' records come before its 'actor' ones, as `rows_of()` lists them."""
  lines = ['# tools/bench_actor.py: a process per row; event pairs, the median of %d launches after %d '
           'warm-up launches and of %d torch loops after %d warm-up frames; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, benchlib.device_of(records))]
  ok = True
  for name in dict.fromkeys(r['name'] for r in records):
    loop = tabular = None
    for r in (r for r in records if r['name'] == name):
      ms = r['ms']
      head = '%-10s S=%-4d B=%d T=%d  ' % (name, r['S'], B, T)
      if r['what'] == 'torch':
        loop = ms
        lines.append('%storch restatement (softmax_weights() + threshold compare + play() + gather / '
                     'scatter_ on both tables a frame)   %.1f ms = %.1f us / frame' % (head, ms, ms * 1000 / T))
        continue
      if r['what'] == 'tabular':
        tabular = ms
        lines.append('%slearn_tabular() planned   %.3f ms = %.3f us / frame' % (head, ms, ms * 1000 / T))
        continue
      text = '%slearn_actor_critic() %s -> path %d (%6d B LDS)   %.3f ms = %.3f us / frame' % (
          head, 'planned' if r['path'] == 0 else 'path=%d ' % r['path'], r['plan'][0], r['plan'][1], ms,
          ms * 1000 / T)
      if tabular is not None:
        text += '   x%.2f learn_tabular()' % (ms / tabular)
      if loop is not None:
        text += ', torch / this = x%.1f' % (loop / ms)
        if ms > loop:
          text += '   GATE MISSED'
          ok = False
      lines.append(text)
  lines.append('gate (learn_actor_critic() no slower than the torch restatement of the same frames, every '
               'row): %s' % ('met' if ok else 'MISSED'))
  return lines, ok


def main(argv):
  if argv[:1] == ['--row']:
    return benchlib.row_main(row, argv[1:])
  args, games = list(argv), GAMES
  if '--games' in args:
    i = args.index('--games')
    games = tuple(args[i + 1].split(','))
    del args[i:i + 2]
  records, broke = benchlib.run_rows(__file__, [r for name in games for r in rows_of(name)], ROW_SECONDS)
  lines, ok = report(records)
  return benchlib.finish(benchlib.out_path(args, 'r24_actor.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
