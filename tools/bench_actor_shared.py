#!/usr/bin/env python3
"""`learn_actor_critic_shared()` measured: T frames of synchronous advantage actor-critic - P
learners, each one softmax policy and one critic fed by n = B / P actors - in ONE launch, beside
`learn_shared()` at the same (n, P), `learn_actor_critic()` at the same B, and what a user pays for
the same frames without it.

T = 1 000, B = 65 536; the boat race (8 states) at n = 1, 16, 256 and 1 024 and the 16x16 maze (159
states) at n = 16, 256 and 1 024.  Per game `learn_actor_critic()` planned, once; per (game, n):
  - `learn_shared()`, planned, for scale: the ratio is what the softmax, the five sums of a state
    and the six divisions of its owner cost over the value-based shared frame - recorded, not gated;
  - the torch restatement on the same device: per frame `softmax_weights()` of the actors' rows, the
    threshold compare on a uniform draw, one `play()`, gathers on both tables and
    `index_put_(accumulate=True)` of the visitor counts and of both tables' updates.  It draws
    torch's random numbers and sums floats: the comparator for the time, not for the bits
    (tests/test_shared_actor.py has those);
  - `learn_actor_critic_shared()` planned, and with each path forced where the plan takes it.

GATE: every `learn_actor_critic_shared()` row is no slower than the torch loop of its (game, n).
Rows, failures and exit statuses: tools/benchlib.py.

Warm-up first, event pairs, the median of 15 launches and of 3 torch loops.

    python tools/bench_actor_shared.py [out.txt] [--games boat_race,maze16]
                                                        # default: profiles/r25_actor_shared.txt
"""
import ctypes
import sys

import benchlib

sys.path.insert(0, benchlib.REPO)

T, B = 1000, 65536
RUNS, WARM = 15, 3                 # launches
LOOP_RUNS, LOOP_WARM_FRAMES = 3, 20     # torch loops of T frames
GAMES = ('boat_race', 'maze16')
ACTORS = {'boat_race': (1, 16, 256, 1024), 'maze16': (16, 256, 1024)}
TABLES = {'boat_race': (8, 1), 'maze16': (159, 0)}        # states, hidden performance
ROW_SECONDS = 300
ALPHA_ACTOR, ALPHA_CRITIC, GAMMA, EPSILON = 0.1, 0.1, 0.9, 0.1


def torch_frames(game, prefs, values, n, frames):
  """`frames` frames of the shared rule - every visited state moves by the step size times the
  mean update of its visitors - in torch ops and one `play()` per frame."""
  import torch
  from campx_amd.returns import softmax_weights
  f = game.fused
  P, S = values.shape
  m = torch.arange(B, device='cuda') // n
  zero = torch.zeros((), dtype=torch.int64, device='cuda')
  one = torch.ones((B,), device='cuda')
  for _ in range(frames):
    s = torch.where(f.done != 0, zero, f.state.long())
    w = softmax_weights(prefs[m, s])
    c = w.cumsum(1)
    r = torch.rand((B, 1), device='cuda') * c[:, 4:]
    a = (r >= c[:, :4]).sum(1)
    v_s = values[m, s]
    _, reward, discount = game.play(a.to(torch.int8))
    rew = torch.zeros((B,), device='cuda') if reward is None else torch.nan_to_num(reward)
    v_n = values[m, f.state.long()]
    delta = rew + (GAMMA * discount) * v_n - v_s          # (an episode's last frame reports discount 0)
    visitors = torch.zeros((P, S), device='cuda').index_put_((m, s), one, accumulate=True).clamp_(min=1)
    grad = delta[:, None] * (torch.nn.functional.one_hot(a, 5) - w / c[:, 4:])
    values += ALPHA_CRITIC * torch.zeros((P, S), device='cuda').index_put_(
        (m, s), delta, accumulate=True) / visitors
    prefs += ALPHA_ACTOR * torch.zeros((P, S, 5), device='cuda').index_put_(
        (m, s), grad, accumulate=True) / visitors[:, :, None]


def row(name, what, n, path):
  """One row, in this process: `name`, `S`, `what` ('torch', 'actor', 'shared' or 'a2c'), `n`, the
  forced `path` (0: planned), the median `ms` of `runs` calls, `device`; for 'a2c' also `plan`."""
  import torch
  from campx_amd import _hip
  game = benchlib.state_table_game(name, B)
  f = game.fused
  S = f.n_states
  P = B // n
  res = {'name': name, 'S': S, 'what': what, 'n': n, 'path': path,
         'device': torch.cuda.get_device_name(0)}
  prefs = torch.zeros((P, S, 5), device='cuda')
  values = torch.zeros((P, S), device='cuda')
  if what == 'torch':
    torch_frames(game, prefs, values, n, LOOP_WARM_FRAMES)
    loop = lambda: torch_frames(game, prefs, values, n, T)
    return dict(res, runs=LOOP_RUNS, ms=benchlib.median_ms(loop, LOOP_RUNS))
  if what == 'actor':
    out = game.learner_buffers(T, 100)
    hyper = [torch.full((B,), x, device='cuda') for x in (ALPHA_ACTOR, ALPHA_CRITIC, GAMMA)]
    launch = lambda: game.learn_actor_critic(T, prefs, values, *hyper, seed=1, window=100, out=out)
  elif what == 'shared':
    out = game.shared_learner_buffers(P, T, 100)
    hyper = [torch.full((P,), x, device='cuda') for x in (ALPHA_ACTOR, GAMMA, EPSILON)]
    launch = lambda: game.learn_shared(T, prefs, *hyper, seed=1, window=100, out=out)
  else:
    out = game.shared_actor_buffers(P, T, 100, path)
    hyper = [torch.full((P,), x, device='cuda') for x in (ALPHA_ACTOR, ALPHA_CRITIC, GAMMA)]
    launch = lambda: game.learn_actor_critic_shared(T, prefs, values, *hyper, seed=1, window=100,
                                                    out=out, path=path)
    plan = (ctypes.c_int64 * 6)()
    _hip.lib.campx_wide_actor_shared_plan(S, int(f.has_perf), B, P, _hip.config_get('wide_lds_max'),
                                          path, plan)
    res['plan'] = list(plan)
  return dict(res, runs=RUNS, ms=benchlib.median_ms(launch, RUNS, WARM))


def rows_of(name):
  """The rows of a game; a forced path is listed only if the plan takes it (host arithmetic)."""
  from campx_amd import _hip
  S, perf = TABLES[name]
  plan = (ctypes.c_int64 * 6)()
  rows = [(name, 'actor', 1, 0)]
  for n in ACTORS[name]:
    paths = [0] + [path for path in (1, 2) if _hip.lib.campx_wide_actor_shared_plan(
        S, perf, B, B // n, _hip.config_get('wide_lds_max'), path, plan) == 0]
    rows += [(name, 'shared', n, 0), (name, 'torch', n, 0)] + [(name, 'a2c', n, path) for path in paths]
  return rows


def report(records):
  """A game's 'actor' record comes first, and an n's 'shared' and 'torch' records before its 'a2c'
  ones, as `rows_of()` lists them."""
  lines = ['# tools/bench_actor_shared.py: a process per row; event pairs, the median of %d launches '
           'after %d warm-up launches and of %d torch loops after %d warm-up frames; %s'
           % (RUNS, WARM, LOOP_RUNS, LOOP_WARM_FRAMES, benchlib.device_of(records))]
  ok = True
  for name in dict.fromkeys(r['name'] for r in records):
    alone = loop = shared = None
    for r in (r for r in records if r['name'] == name):
      ms = r['ms']
      head = '%-10s S=%-4d B=%d T=%d  ' % (name, r['S'], B, T)
      if r['what'] == 'actor':
        alone = ms
        lines.append('%slearn_actor_critic() planned (a learner per environment)   %.3f ms = %.3f us / frame'
                     % (head, ms, ms * 1000 / T))
        continue
      head += 'n=%-4d P=%-5d ' % (r['n'], B // r['n'])
      if r['what'] == 'torch':
        loop = ms
        lines.append('%storch restatement (softmax_weights() + threshold compare + play() + gathers + '
                     'index_put_(accumulate=True) on both tables a frame)   %.1f ms = %.1f us / frame'
                     % (head, ms, ms * 1000 / T))
        continue
      if r['what'] == 'shared':
        shared, loop = ms, None
        lines.append('%slearn_shared() planned   %.3f ms = %.3f us / frame' % (head, ms, ms * 1000 / T))
        continue
      text = '%slearn_actor_critic_shared() %s -> path %d, G=%d (%6d B LDS)   %.3f ms = %.3f us / frame' % (
          head, 'planned' if r['path'] == 0 else 'path=%d ' % r['path'], r['plan'][0], r['plan'][1],
          r['plan'][3], ms, ms * 1000 / T)
      if shared is not None:
        text += '   x%.2f learn_shared()' % (ms / shared)
      if alone is not None:
        text += ', x%.2f learn_actor_critic()' % (ms / alone)
      if loop is not None:
        text += ', torch / this = x%.1f' % (loop / ms)
        if ms > loop:
          text += '   GATE MISSED'
          ok = False
      lines.append(text)
  lines.append('gate (learn_actor_critic_shared() no slower than the torch restatement of the same '
               'frames, every row): %s' % ('met' if ok else 'MISSED'))
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
  return benchlib.finish(benchlib.out_path(args, 'r25_actor_shared.txt'), lines, ok, broke)


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
