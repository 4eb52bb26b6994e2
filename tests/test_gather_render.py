"""Trace-only rollouts and on-demand rendering of sampled frames, on the GPU.

`rollout_trace()` must leave exactly what `rollout()` leaves, minus the observations; and
`render_frames(trace, t, e)` must give, bit for bit, `rollout()`'s `obs[t, e]` - for every game
kind the gather kernel covers (one to four movers of the one-cell tier, a state-table game,
pieces in a mask, a scenery in variants), for batches that are and are not a multiple of 16, in
int8 / bf16 / f16 and with int32 / int64 indices.  All comparisons are exact."""

import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# frames per rollout: the maze's shortest way to its goal is 26 moves
FRAMES = {'maze_16x16': 40}
BATCHES = (1000, 4097)
GAMES = ('boat_race', 'sokoban', 'sokoban_l2', 'wall_world', 'maze_16x16', 'pieces', 'variants')
DTYPES = (torch.int8, torch.bfloat16, torch.float16)
CASES = [(g, b) for g in GAMES for b in BATCHES]
CASE_IDS = ['{}-{}'.format(g, b) for g, b in CASES]


def _builder(name):
  from games_under_test import FUSED_GAMES, WIDE_GAMES
  import random_pickups
  if name in FUSED_GAMES:
    return FUSED_GAMES[name]
  if name in WIDE_GAMES:
    return WIDE_GAMES[name]
  defs = random_pickups.definitions()
  # tests/test_random_pickups.py's routes: seven coins travel as a piece mask, the tide as variants
  return random_pickups.builder(defs[{'pieces': 3, 'variants': 12}[name]])


def _game(name, B):
  game = _builder(name)(batch=B, device='cuda')
  game.its_showtime()
  f = game.fused
  if name == 'pieces':
    assert f.spec.n_pieces > 0
  if name == 'variants':
    assert f.spec.n_variants > 1
  if name == 'sokoban_l2':
    assert f.n_dyn == 4          # the agent and three boxes
  if name == 'sokoban':
    assert f.n_dyn == 2
  return game


def _frames(name):
  return FRAMES.get(name, 24)


def _maze_way():
  """Action ids of a shortest way from 'A' to 'G' of the 16x16 maze (breadth first over its art)."""
  from campx_amd.games import maze
  art = maze.maze_art(16, 16)
  find = lambda ch: next((r, row.index(ch)) for r, row in enumerate(art) if ch in row)
  start, goal = find('A'), find('G')
  moves = {0: (0, -1), 1: (0, 1), 2: (-1, 0), 3: (1, 0)}
  came, queue = {start: None}, [start]
  for at in queue:
    for a, (dr, dc) in moves.items():
      to = (at[0] + dr, at[1] + dc)
      if art[to[0]][to[1]] != '#' and to not in came:
        came[to] = (at, a)
        queue.append(to)
  way, at = [], goal
  while came[at] is not None:
    at, a = came[at]
    way.append(a)
  return way[::-1]


def _actions(name, B, call):
  """Seeded random action streams.  They end episodes by themselves in the sokobans and the two
  pickup games (hundreds of times in 24 frames); no random walk reaches the maze's goal, so every
  third environment of the maze's first rollout walks a shortest way there and goes on at random."""
  T = _frames(name)
  gen = torch.Generator().manual_seed(1000 * call + B + len(name))
  acts = torch.randint(0, 5, (T, B), generator=gen, dtype=torch.int8)
  if name == 'maze_16x16' and call == 0:
    way = torch.tensor(_maze_way(), dtype=torch.int8)
    assert len(way) < T - 1
    acts[:len(way), ::3] = way[:, None]
  return acts.cuda()


@functools.lru_cache(maxsize=None)
def _rolled(name, B):
  """(game, [three consecutive rollouts' dicts]) - full rollouts, the reference of every check.
  No test advances the cached game any further."""
  game = _game(name, B)
  outs = [game.rollout(_actions(name, B, i), reset_first=(i == 0)) for i in range(3)]
  torch.cuda.synchronize()
  return game, outs


def _bits(x):
  return x.view(torch.int16) if x.element_size() == 2 else x


def _expect(obs, t, e, dtype):
  return obs[t.long(), e.long()].to(dtype)


def _state(f):
  return f.state if f.pos is None else f.pos


@pytest.mark.parametrize('name,B', CASES, ids=CASE_IDS)
def test_rollout_trace_leaves_what_rollout_leaves(name, B):
  a, outs = _rolled(name, B)
  T = _frames(name)
  b = _game(name, B)
  assert set(b.rollout_trace_buffers(T)) == {'trace', 'reward', 'discount', 'done', 'perf'}
  bufs = b.rollout_trace_buffers(T)
  for i in range(2):
    got = b.rollout_trace(_actions(name, B, i), reset_first=(i == 0), out=bufs if i else None)
    assert 'obs' not in got and 'board' not in got
    for k in ('trace', 'reward', 'discount', 'done', 'perf'):
      want = outs[i][k]
      if want is None:
        assert got[k] is None, k
        continue
      assert got[k].shape == want.shape and got[k].dtype == want.dtype, k
      assert got[k].stride() == want.stride(), k                # the same row padding
      assert torch.equal(got[k].view(torch.uint8) if got[k].dtype == torch.float32 else got[k],
                         want.view(torch.uint8) if want.dtype == torch.float32 else want), (i, k)
    # ... and the frames render from a trace that only rollout_trace() ever wrote
    gen = torch.Generator().manual_seed(i)
    t = torch.randint(0, T, (2000,), generator=gen).cuda()
    e = torch.randint(0, B, (2000,), generator=gen).cuda()
    assert torch.equal(b.render_frames(got['trace'], t, e), outs[i]['obs'][t, e])
  # a third call (the cached game has made it too): both carried on from the same state
  want = outs[2]
  got = b.rollout_trace(_actions(name, B, 2))
  assert torch.equal(got['trace'], want['trace']) and torch.equal(got['done'], want['done'])
  assert torch.equal(_state(a.fused), _state(b.fused))
  assert torch.equal(a.fused.done, b.fused.done)
  assert torch.equal(a.fused.ret.view(torch.int32), b.fused.ret.view(torch.int32))
  assert a.fused.frame == b.fused.frame
  b.fused.check_actions()


def _index_sets(T, B, done):
  """name -> (t, e) int64 CPU tensors."""
  gen = torch.Generator().manual_seed(B)
  tt, ee = torch.meshgrid(torch.arange(T), torch.arange(B), indexing='ij')
  tt, ee = tt.reshape(-1), ee.reshape(-1)
  perm = torch.randperm(T * B, generator=gen)
  dup = torch.randint(0, T * B, (3001,), generator=gen) % 97     # many repeats of a few pairs
  sets = {
      'in_order': (tt, ee),
      'permutation': (tt[perm], ee[perm]),
      'duplicates': (tt[dup], ee[dup]),
      'one': (torch.tensor([T // 2]), torch.tensor([B // 3])),
      'odd_n': (tt[perm[:1237]], ee[perm[:1237]]),                # 1 237 rows: N * R is odd for odd R
      'corners': (torch.tensor([0, 0, T - 1, T - 1]), torch.tensor([0, B - 1, 0, B - 1])),
  }
  ended = done.nonzero()
  if len(ended):
    # the frame an episode ended on and the one after it (the rebuilt environment's first)
    t_end, e_end = ended[:, 0].cpu(), ended[:, 1].cpu()
    keep = t_end < T - 1
    t_end, e_end = t_end[keep][:500], e_end[keep][:500]
    sets['episode_ends'] = (torch.cat([t_end, t_end + 1]), torch.cat([e_end, e_end]))
  return sets


# Games that cannot end an episode, and why: their action streams hold no game-over because no
# stream could.  Every other game's stream must (and the test says so if it does not).
NEVER_ENDS = {
    'boat_race': 'none of its entities calls terminate_episode() (examples/boat_race.py: the race goes on)',
    'wall_world': 'an AgentDrape and three FixedDrapes: no goal, nothing that terminates',
}


@pytest.mark.parametrize('name,B', CASES, ids=CASE_IDS)
def test_render_frames_gives_the_rollouts_frames(name, B):
  game, outs = _rolled(name, B)
  out = outs[0]
  T = _frames(name)
  obs, trace = out['obs'], out['trace']
  sets = _index_sets(T, B, out['done'])
  if name in NEVER_ENDS:
    assert not any(bool(o['done'].any()) for o in outs), NEVER_ENDS[name]
  else:
    assert 'episode_ends' in sets, 'no episode ended: the action stream must hold game-overs'
    t_end, e_end = sets['episode_ends']
    half = len(t_end) // 2
    assert half >= 10
    assert bool(out['done'][t_end[:half].cuda(), e_end[:half].cuda()].all())     # the frame it ended on ...
    assert torch.equal(t_end[half:], t_end[:half] + 1)                           # ... and the one after
  n = 0
  for what, (t, e) in sets.items():
    for dtype in DTYPES:
      for idx in (torch.int64, torch.int32):
        td, ed = t.to(idx).cuda(), e.to(idx).cuda()
        got = game.render_frames(trace, td, ed, obs_dtype=dtype)
        assert got.shape == (len(t),) + obs.shape[2:] and got.dtype == dtype
        assert torch.equal(_bits(got), _bits(_expect(obs, td, ed, dtype))), (what, dtype, idx)
        n += 1
  game.fused.check_actions()      # nothing was out of range
  assert n == len(sets) * 6          # every set in every dtype with both index types


@pytest.mark.parametrize('name,B', CASES, ids=CASE_IDS)
def test_a_ring_of_three_rollouts_renders_frames_of_all_three(name, B):
  game, outs = _rolled(name, B)
  T = _frames(name)
  ring = torch.cat([o['trace'] for o in outs], dim=1)            # [planes, 3 T, B], rows back to back
  obs = torch.cat([o['obs'] for o in outs], dim=0)
  gen = torch.Generator().manual_seed(5)
  t = torch.randint(0, 3 * T, (5000,), generator=gen)
  e = torch.randint(0, B, (5000,), generator=gen)
  t[:3] = torch.tensor([0, T, 3 * T - 1])
  for i in range(3):
    assert ((t >= i * T) & (t < (i + 1) * T)).any()
  for dtype in (torch.int8, torch.bfloat16):
    got = game.render_frames(ring, t.cuda(), e.cuda(), obs_dtype=dtype)
    assert torch.equal(_bits(got), _bits(_expect(obs, t.cuda(), e.cuda(), dtype)))


@pytest.mark.parametrize('name,B', CASES, ids=CASE_IDS)
def test_indices_out_of_range_are_clamped_and_counted(name, B):
  game, outs = _rolled(name, B)
  T = _frames(name)
  obs, trace = outs[0]['obs'], outs[0]['trace']
  gen = torch.Generator().manual_seed(9)
  t = torch.randint(0, T, (700,), generator=gen)
  e = torch.randint(0, B, (700,), generator=gen)
  bad = {3: (-1, 0), 64: (T, 5), 200: (2, -7), 699: (1, B), 350: (T + 10 ** 6, B + 10 ** 6)}
  for i, (ti, ei) in bad.items():
    t[i], e[i] = ti, ei
  good = torch.ones(700, dtype=torch.bool)
  good[list(bad)] = False
  f = game.fused
  f.check_actions()
  f.validate_actions = False             # (the lazy look at the flag may or may not see this call's)
  try:
    for idx in (torch.int64, torch.int32):
      got = game.render_frames(trace, t.to(idx).cuda(), e.to(idx).cuda())       # returns
      want = obs[t.clamp(0, T - 1).cuda(), e.clamp(0, B - 1).cuda()]
      assert torch.equal(got[good.cuda()], want[good.cuda()])
      assert torch.equal(got, want)      # the others show the nearest frame inside
      with pytest.raises(ValueError, match=r'\b{} rows of render_frames'.format(len(bad))):
        f.check_actions()
      f.check_actions()                  # counted once, then cleared
  finally:
    f.validate_actions = True


@pytest.mark.parametrize('name,B', [('boat_race', 1000), ('pieces', 4097)])
def test_bad_indices_surface_lazily_and_beside_bad_actions(name, B):
  """validate_actions=True, the default: no call synchronises; the pinned flag a launch raised is
  seen by the first render_frames() or rollout after the GPU got there.  And when bad actions and
  bad indices are both up, ONE error names both counts - neither is lost."""
  T = _frames(name)
  game = _game(name, B)                  # (a game of its own: it is advanced and left with flags)
  f = game.fused
  assert f.validate_actions is True
  trace = game.rollout_trace(_actions(name, B, 0), reset_first=True)['trace']
  want = _rolled(name, B)[1][0]['obs']
  ok_t, ok_e = torch.tensor([0, 1, 2]).cuda(), torch.tensor([0, 1, 2]).cuda()
  bad_t, bad_e = torch.tensor([0, T, -1]).cuda(), torch.tensor([0, 1, B]).cuda()
  bufs = game.rollout_trace_buffers(T)

  def later_calls():
    yield lambda: game.render_frames(trace, ok_t, ok_e)
    yield lambda: game.rollout_trace(_actions(name, B, 1), out=bufs)
  for later in later_calls():
    seen = None
    try:
      game.render_frames(trace, bad_t, bad_e)
    except ValueError as err:            # (allowed: the launch's flag was visible already)
      seen = str(err)
    torch.cuda.synchronize()
    if seen is None:
      with pytest.raises(ValueError) as err:
        later()
      seen = str(err.value)
    assert '2 rows of render_frames' in seen and 'action ids' not in seen
    f.check_actions()                    # raised once, then clean
    assert torch.equal(game.render_frames(trace, ok_t, ok_e), want[ok_t, ok_e])
  # both kinds at once: the index flag is up (and nobody has looked) when a play() with bad ids
  # comes by - its look at the flags reads BOTH counters before it clears either
  acts = torch.randint(0, 5, (B,), dtype=torch.int8)
  acts[4], acts[7], acts[9] = 9, -2, 77
  f.validate_actions = False
  try:
    game.render_frames(trace, bad_t, bad_e)
  finally:
    f.validate_actions = True
  torch.cuda.synchronize()
  with pytest.raises(ValueError) as both:
    game.play(acts.cuda())
  assert '3 action ids' in str(both.value) and '2 rows of render_frames' in str(both.value)
  f.check_actions()                      # nothing left behind


@pytest.mark.parametrize('name,B', [('boat_race', 4097), ('sokoban_l2', 1000), ('pieces', 1000),
                                    ('variants', 4097)])
def test_render_frames_is_capturable_in_a_hip_graph(name, B):
  game, outs = _rolled(name, B)
  T = _frames(name)
  obs, trace = outs[0]['obs'], outs[0]['trace']
  gen = torch.Generator().manual_seed(2)
  N = 2049
  t = torch.randint(0, T, (N,), generator=gen).cuda()
  e = torch.randint(0, B, (N,), generator=gen).cuda()
  dst = torch.empty((N,) + obs.shape[2:], dtype=torch.bfloat16, device='cuda')
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    game.render_frames(trace, t, e, out=dst)       # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    game.render_frames(trace, t, e, out=dst)
  for seed in (3, 4):
    gen = torch.Generator().manual_seed(seed)
    t.copy_(torch.randint(0, T, (N,), generator=gen))
    e.copy_(torch.randint(0, B, (N,), generator=gen))
    dst.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(_expect(obs, t, e, torch.bfloat16)))


def test_the_shape_tier_refuses_both_by_name():
  from games_under_test import SHAPE_GAMES
  game = SHAPE_GAMES['hello_world'](batch=64, device='cuda')
  game.its_showtime()
  acts = torch.zeros((4, 64), dtype=torch.int8, device='cuda')
  with pytest.raises(NotImplementedError, match='rollout_trace'):
    game.rollout_trace(acts)
  with pytest.raises(NotImplementedError, match='render_frames'):
    game.render_frames(torch.zeros((1, 4, 64), dtype=torch.uint8, device='cuda'),
                       torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))


def test_games_without_a_tabulated_update_pass_say_so(monkeypatch):
  from campx_amd import fused
  from campx_amd.games import sokoban
  monkeypatch.setattr(fused, 'COMPILE_TABLE', False)
  game = sokoban.build(batch=64, device='cuda')
  game.its_showtime()
  with pytest.raises(ValueError, match='not tabulated'):
    game.rollout_trace(torch.zeros((4, 64), dtype=torch.int8, device='cuda'))


def test_replay_minibatches_example_runs():
  """examples/replay_minibatches.py: a ring of traces filled by rollout_trace(), minibatches of
  sampled transitions rendered in bf16 for the reference driver's MLP."""
  repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, os.path.join(repo, 'examples'))
  import replay_minibatches
  got = replay_minibatches.run(batch=512, frames=20, episodes=3, minibatches=2, n=300)
  assert got['ring'].shape == (1, 60, 512) and got['minibatch'].shape == (300, 7, 5, 5)
  assert got['minibatch'].dtype == torch.bfloat16 and len(got['values']) == 2
  assert all(v == v for v in got['values'])
  again = got['game'].render_frames(got['ring'], got['last_t'], got['last_e'])
  assert torch.equal(again.to(torch.bfloat16).view(torch.int16), got['minibatch'].view(torch.int16))
  assert int(again.sum()) == 300 * 25          # every cell of a frame shows exactly one character
