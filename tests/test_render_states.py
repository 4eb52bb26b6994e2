"""`render_states()` on the GPU (csrc/k_states.hip, `campx::wide_render_states`): the observation of
a state of the table, bit for bit what the engine shows for an environment in that state.

The games (each set up once, 257 environments):
  * maze, boat_race, pickups, porter   tests/test_policy_rollout.py's: the 16x16 maze, the boat
                race on its state table, seven coins as a piece MASK (the trace's second plane,
                episodes that end), and the two-plane porter whose table is past the LDS bound;
  * maze_15x17  rows of 1 530 bytes: no whole number of 16-byte chunks;
  * variants    a `random_pickups` definition whose scenery comes in several VARIANTS.
Every comparison is `torch.equal` on bits, in int8, float16 and bfloat16."""

import functools

import pytest
import torch

from test_policy_rollout import _engine, _policy

pytestmark = pytest.mark.gpu

GAMES = ['maze', 'boat_race', 'pickups', 'porter', 'maze_15x17', 'variants']
DTYPES = (torch.int8, torch.float16, torch.bfloat16)
B, T = 257, 24


@functools.lru_cache(maxsize=None)
def _game(name):
  from campx_amd import wide
  if name == 'maze_15x17':
    from campx_amd.games import maze
    game = maze.build(15, 17, batch=B, device='cuda')
  elif name == 'variants':
    import random_pickups
    defs = random_pickups.definitions()
    game = None
    for i in [12] + [i for i in range(len(defs)) if i != 12]:     # (12: test_gather_render.py's)
      game = random_pickups.builder(defs[i])(batch=B, device='cuda')
      game.its_showtime()
      if isinstance(game.fused, wide.WideGame) and game.fused.spec.n_variants > 1:
        break
  else:
    game = _engine(name, B)
  if name != 'variants':
    game.its_showtime()
  f = game.fused
  assert isinstance(f, wide.WideGame), type(f)
  if name == 'variants':
    assert f.spec.n_variants > 1
  if name == 'pickups':
    assert f.spec.n_pieces > 0 and f._n_planes == f.n_dyn + 1
  if name == 'porter':
    assert f._n_planes == 2
  if name == 'maze_15x17':
    assert f.n_layers * f.rows * f.cols == 1530
  return game


def _bits(x):
  return x.view(torch.int16) if x.element_size() == 2 else x


def _same(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _all_states(name, dtype):
  """render_states() of every state, computed once and left unchanged."""
  out = _game(name).render_states(obs_dtype=dtype)
  torch.cuda.synchronize()
  return out


@pytest.mark.parametrize('name', GAMES)
def test_state_zero_is_the_showtime_frame(name):
  game = _game(name)
  f = game.fused
  first = f.showtime()[0].layered_board[0].clone()
  assert first.dtype == torch.int8
  for dtype in DTYPES:
    for idx in (torch.int64, torch.int32):
      got = game.render_states(torch.zeros(1, dtype=idx, device='cuda'), obs_dtype=dtype)
      assert got.shape == (1, f.n_layers, f.rows, f.cols) and got.dtype == dtype
      assert _same(got[0], first.to(dtype)), (dtype, idx)
    assert _same(_all_states(name, dtype)[0], first.to(dtype))
  f.check_actions()


@pytest.mark.parametrize('name', GAMES)
def test_states_of_a_policy_rollout_against_its_rendered_trace(name):
  """`out['states'][t + 1]` is the state frame t reached - `trace[t]` - or, behind an episode end,
  the reset state; `fused.state` is the state the last frame reached."""
  game = _game(name)
  f = game.fused
  S = f.n_states
  shared = name in ('maze', 'boat_race', 'pickups', 'porter')       # test_policy_rollout.py's games
  w = torch.from_numpy(_policy(name, S) if shared else _weights(S)).cuda()
  first = f.showtime()[0].layered_board[0].clone()
  out = game.rollout_policy(w, T, seed=11, reset_first=True)
  trace, done = out['trace'], out['done']
  if name == 'pickups':
    assert bool(done[:T - 1].any())                       # episodes end inside the rollout
  env = torch.arange(B, device='cuda')
  tt = torch.arange(T - 1, device='cuda').repeat_interleave(B)
  ee = env.repeat(T - 1)
  ids = out['states'][1:].reshape(-1)
  over = done[:T - 1].reshape(-1).bool()
  assert ids.shape == (B * (T - 1),) and bool((ids[over] == 0).all())
  for dtype in DTYPES:
    last = game.render_frames(trace, torch.full((B,), T - 1, device='cuda'), env, obs_dtype=dtype)
    assert _same(game.render_states(f.state, obs_dtype=dtype), last), dtype
    want = game.render_frames(trace, tt, ee, obs_dtype=dtype)
    want[over] = first.to(dtype)
    assert _same(game.render_states(ids, obs_dtype=dtype), want), dtype
    # frame 0 samples from the reset state: the observation render_frames() never yields
    assert _same(game.render_states(out['states'][0], obs_dtype=dtype),
                 first.to(dtype).expand(B, -1, -1, -1).contiguous()), dtype
  f.check_actions()


def _weights(S):
  import numpy as np
  return np.random.RandomState(S).uniform(0.05, 1.0, size=(S, 5)).astype(np.float32)


@pytest.mark.parametrize('name', GAMES)
def test_all_states_equal_the_calls_on_their_parts(name):
  """Ranges split at 1, 15, 16, 17 and 4 097: the edges of a 16-row group and of a 256-lane
  block of wide_state_rows_kernel, and starts that are not whole render windows."""
  game = _game(name)
  f = game.fused
  S = f.n_states
  cuts = [0] + [c for c in (1, 15, 16, 17, 4097) if c < S] + [S]
  for dtype in DTYPES:
    whole = _all_states(name, dtype)
    assert whole.shape == (S, f.n_layers, f.rows, f.cols) and whole.dtype == dtype
    parts = [game.render_states(torch.arange(a, b, device='cuda', dtype=torch.int32), obs_dtype=dtype)
             for a, b in zip(cuts[:-1], cuts[1:])]
    assert _same(torch.cat(parts), whole), dtype
    assert len(torch.unique(_bits(whole).reshape(S, -1), dim=0)) > 1      # (not one picture S times)
  f.check_actions()


@pytest.mark.parametrize('N', [1, 63, 4099])
@pytest.mark.parametrize('name', GAMES)
def test_repeated_ids(name, N):
  game = _game(name)
  S = game.fused.n_states
  gen = torch.Generator().manual_seed(N + S)
  ids = torch.randint(0, S, (N,), generator=gen)
  ids[N // 2:] = ids[:N - N // 2].flip(0)          # every id of the second half is a repeat
  for dtype in DTYPES:
    for idx in (torch.int64, torch.int32):
      got = game.render_states(ids.to(idx).cuda(), obs_dtype=dtype)
      assert _same(got, _all_states(name, dtype)[ids.cuda()]), (dtype, idx)
  game.fused.check_actions()


@pytest.mark.parametrize('name', ['boat_race', 'pickups', 'variants'])
def test_bad_ids_render_as_state_zero_and_are_counted(name):
  game = _game(name)
  f = game.fused
  S = f.n_states
  gen = torch.Generator().manual_seed(S)
  ids = torch.randint(0, S, (300,), generator=gen)
  bad = {3: -1, 64: S, 255: 2 ** 31 - 1, 256: -2 ** 31, 299: S + 10 ** 6}
  for i, v in bad.items():
    ids[i] = v
  good = torch.ones(300, dtype=torch.bool)
  good[list(bad)] = False
  f.check_actions()
  f.validate_actions = False             # (the lazy look at the flag may or may not see this call's)
  try:
    for idx in (torch.int64, torch.int32):
      for dtype in DTYPES:
        whole = _all_states(name, dtype)
        got = game.render_states(ids.to(idx).cuda(), obs_dtype=dtype)          # returns
        assert _same(got[good.cuda()], whole[ids[good].cuda()]), (idx, dtype)
        assert _same(got[(~good).cuda()], whole[:1].expand(len(bad), -1, -1, -1).contiguous())
      with pytest.raises(ValueError, match=r'\b{} state ids'.format(3 * len(bad))):
        f.check_actions()
      f.check_actions()                  # counted once, then cleared
      assert int(f._bad_state_ids.item()) == 0
    # int64 ids past 32 bits are bad ids, not ids modulo 2^32
    far = torch.tensor([1, 2 ** 32, 2 ** 32 + 1, -2 ** 40], dtype=torch.int64, device='cuda')
    got = game.render_states(far)
    whole = _all_states(name, torch.int8)
    assert _same(got, whole[torch.tensor([1, 0, 0, 0], device='cuda')])
    with pytest.raises(ValueError, match=r'\b3 state ids'):
      f.check_actions()
  finally:
    f.validate_actions = True
  # 'sync' raises at once
  f.validate_actions = 'sync'
  try:
    with pytest.raises(ValueError, match=r'\b1 state ids'):
      game.render_states(torch.tensor([S], device='cuda'))
  finally:
    f.validate_actions = True
  f.check_actions()


@pytest.mark.parametrize('name', ['boat_race', 'maze_15x17', 'pickups', 'variants'])
def test_render_states_is_capturable_in_a_hip_graph(name):
  game = _game(name)
  f = game.fused
  S, N = f.n_states, 1031
  gen = torch.Generator().manual_seed(2)
  ids = torch.randint(0, S, (N,), generator=gen).cuda()
  dst = torch.empty((N, f.n_layers, f.rows, f.cols), dtype=torch.bfloat16, device='cuda')
  whole = _all_states(name, torch.bfloat16)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    game.render_states(ids, out=dst)             # warm up outside the capture (and size the scratch)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                  # one stream, no parallel branches
    assert game.render_states(ids, out=dst) is dst
  for seed in (3, 4):
    gen = torch.Generator().manual_seed(seed)
    ids.copy_(torch.randint(0, S, (N,), generator=gen))
    dst.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(dst, whole[ids])
    assert _same(game.render_states(ids, obs_dtype=torch.bfloat16), whole[ids])      # eager
  f.check_actions()


def test_more_rows_than_one_render_launch_addresses():
  """N x row bytes past 2^32 - 65536: the rows go as several render launches.  The 16x16 maze's
  rows are 1 536 bytes, so 2 800 243 rows (4.3 GB of int8) cross the bound by 4 099 rows."""
  game = _game('maze')
  f = game.fused
  S, R = f.n_states, f.n_layers * f.rows * f.cols
  assert R == 1536
  most = ((2 ** 32 - 65536 - 1) // R) // 16 * 16
  N = most + 4099
  ids = torch.arange(N, device='cuda', dtype=torch.int32) % S
  got = game.render_states(ids)
  whole = _all_states('maze', torch.int8)
  for a, b in ((0, 64), (most - 64, most + 64), (N - 64, N)):
    assert torch.equal(got[a:b], whole[ids[a:b].long()]), (a, b)
  assert torch.equal(got[::4099], whole[ids[::4099].long()])
  # and every row, by its sum
  sums = whole.view(S, -1).sum(1, dtype=torch.int32)
  assert torch.equal(got.view(N, -1).sum(1, dtype=torch.int32), sums[ids.long()])
  del got
  f.check_actions()


def test_argument_errors_and_the_other_tiers():
  game = _game('boat_race')
  f = game.fused
  with pytest.raises(ValueError, match='state_ids'):
    game.render_states(torch.zeros(3, dtype=torch.int16, device='cuda'))
  with pytest.raises(ValueError, match='state_ids'):
    game.render_states(torch.zeros((3, 1), dtype=torch.int64, device='cuda'))
  with pytest.raises(ValueError, match='state_ids'):
    game.render_states(torch.zeros(0, dtype=torch.int64, device='cuda'))
  with pytest.raises(ValueError, match='state_ids'):
    game.render_states(torch.zeros(3, dtype=torch.int64))
  with pytest.raises(ValueError, match='state_ids'):
    game.render_states([0, 1])
  with pytest.raises(ValueError, match='obs_dtype'):
    game.render_states(obs_dtype=torch.float32)
  with pytest.raises(ValueError, match='out must be'):
    game.render_states(out=torch.empty((f.n_states + 1, f.n_layers, f.rows, f.cols), dtype=torch.int8,
                                       device='cuda'))
  from campx_amd.games import boat_race
  plain = boat_race.build(64, 'cuda')            # the one-cell tier: no use_state_table()
  plain.its_showtime()
  with pytest.raises(NotImplementedError, match='use_state_table'):
    plain.render_states()
  from games_under_test import SHAPE_GAMES
  hello = SHAPE_GAMES['hello_world'](batch=64, device='cuda')
  hello.its_showtime()
  with pytest.raises(NotImplementedError, match='use_state_table'):
    hello.render_states(torch.zeros(1, dtype=torch.int64, device='cuda'))
  f.check_actions()
