"""Observation windows on the GPU (csrc/k_window.hip, `campx::wide_render_windows`): a window is,
bit for bit, a crop of the full observation (tests/windows_reference.py), whether its rows come
from sampled pairs of a trace, the whole trace or state ids.

The games are tests/test_render_states.py's, 257 environments, traces of 24 frames from
`rollout_policy(reset_first=True)`.  Every comparison is `torch.equal` on bits, in int8, float16
and bfloat16."""

import functools

import pytest
import torch

from campx_amd.windows import Window
from test_policy_rollout import _policy
from test_render_states import B, DTYPES, GAMES, T, _all_states, _bits, _game, _same, _weights

import windows_reference as ref

pytestmark = pytest.mark.gpu

N_ROWS = 4099


@functools.lru_cache(maxsize=None)
def _rollout(name):
  """One rollout per game, left unchanged: its dict, and the first (showtime) observation."""
  game = _game(name)
  f = game.fused
  shared = name in ('maze', 'boat_race', 'pickups', 'porter')
  w = torch.from_numpy(_policy(name, f.n_states) if shared else _weights(f.n_states)).cuda()
  first = f.showtime()[0].layered_board[0].clone()
  out = game.rollout_policy(w, T, seed=11, reset_first=True)
  torch.cuda.synchronize()
  return out, first


@functools.lru_cache(maxsize=None)
def _pairs(name, N=N_ROWS):
  """Rows drawn at random WITH repeats (the second half mirrors the first)."""
  gen = torch.Generator().manual_seed(N + len(name))
  t = torch.randint(0, T, (N,), generator=gen)
  e = torch.randint(0, B, (N,), generator=gen)
  t[N // 2:] = t[:N - N // 2].flip(0)
  e[N // 2:] = e[:N - N // 2].flip(0)
  return t.cuda(), e.cuda()


@functools.lru_cache(maxsize=None)
def _full_frames(name, dtype, N=N_ROWS):
  t, e = _pairs(name, N)
  full = _game(name).render_frames(_rollout(name)[0]['trace'], t, e, obs_dtype=dtype)
  torch.cuda.synchronize()
  return full


def _things(f):
  return [f.chars[int(f.spec.dyn_layer[d])] for d in range(f.n_dyn)]


def _pad_char(f):
  return f.chars[int(f.spec.static_top_layer[0])]       # what the board's corner shows: a wall


def _odd_window(f):
  """A window whose L*h*w is not a multiple of 16."""
  for h, w in ((3, 5), (1, 17), (5, 7), (3, 3)):
    if f.n_layers * h * w >= 16 and (f.n_layers * h * w) % 16 and h <= 2 * f.rows - 1 and w <= 2 * f.cols - 1:
      return h, w
  raise AssertionError('no such window for {} layers'.format(f.n_layers))


def _shapes(f):
  return [(3, 3), (5, 5), (4, 7), (2 * f.rows - 1, 2 * f.cols - 1), _odd_window(f)]


def _want_frames(name, dtype, win, t, e, full):
  f = _game(name).fused
  where = win.resolve(f.chars, f.spec)
  if where.thing >= 0:
    entries = _rollout(name)[0]['trace'][where.thing][t.long(), e.long()]
    r0, c0 = ref.centres(entries, f.cols, f.rows * f.cols, win.height, win.width)
  else:
    r0, c0 = where.r0, where.c0
  return ref.crop(full, r0, c0, win.height, win.width, where.pad_layer)


@pytest.mark.parametrize('name', GAMES)
def test_pairs_equal_the_crop_of_render_frames(name):
  game = _game(name)
  f = game.fused
  trace = _rollout(name)[0]['trace']
  t, e = _pairs(name)
  things = _things(f)
  for dtype in DTYPES:
    full = _full_frames(name, dtype)
    for k, (h, w) in enumerate(_shapes(f)):
      for pad in (None, _pad_char(f)):
        win = Window(h, w, things[k % len(things)], pad=pad)
        got = game.render_frame_windows(trace, t, e, win, obs_dtype=dtype)
        assert got.shape == (N_ROWS, f.n_layers, h, w) and got.dtype == dtype
        assert _same(got, _want_frames(name, dtype, win, t, e, full)), (dtype, win)
  # the largest window holds the whole board with padding on all four sides, in every row
  H, W = f.rows, f.cols
  win = Window(2 * H - 1, 2 * W - 1, things[0], pad=_pad_char(f))
  got = game.render_frame_windows(trace, t, e, win)
  full = _full_frames(name, torch.int8)
  assert torch.equal(got.view(N_ROWS, -1).sum(1) - full.view(N_ROWS, -1).sum(1),
                     torch.full((N_ROWS,), (2 * H - 1) * (2 * W - 1) - H * W, device='cuda'))
  f.check_actions()


@pytest.mark.parametrize('N', [1, 63, 64, 65, N_ROWS])
@pytest.mark.parametrize('name', GAMES)
def test_row_counts_and_index_dtypes(name, N):
  game = _game(name)
  f = game.fused
  trace = _rollout(name)[0]['trace']
  t, e = _pairs(name, N)
  things = _things(f)
  for dtype in DTYPES:
    full = _full_frames(name, dtype, N)
    for shape in ((5, 5), _odd_window(f)):
      win = Window(shape[0], shape[1], things[-1], pad=_pad_char(f))
      want = _want_frames(name, dtype, win, t, e, full)
      for idx in (torch.int64, torch.int32):
        got = game.render_frame_windows(trace, t.to(idx), e.to(idx), win, obs_dtype=dtype)
        assert _same(got, want), (dtype, idx, win)
  f.check_actions()


@pytest.mark.parametrize('name', GAMES)
def test_fixed_windows(name):
  game = _game(name)
  f = game.fused
  H, W = f.rows, f.cols
  trace = _rollout(name)[0]['trace']
  t, e = _pairs(name)
  for dtype in DTYPES:
    full = _full_frames(name, dtype)
    got = game.render_frame_windows(trace, t, e, Window(H, W, (0, 0)), obs_dtype=dtype)
    assert _same(got, full), dtype                         # the board itself
    for corner in ((-1, -2), (H - 2, W - 1)):
      for pad in (None, _pad_char(f)):
        win = Window(3, 4, corner, pad=pad)
        got = game.render_frame_windows(trace, t, e, win, obs_dtype=dtype)
        assert _same(got, _want_frames(name, dtype, win, t, e, full)), (dtype, win)
  f.check_actions()


@pytest.mark.parametrize('name', GAMES)
def test_whole_trace(name):
  game = _game(name)
  f = game.fused
  trace = _rollout(name)[0]['trace']
  assert trace.stride(1) != B                  # padded rows, as rollout_policy() returns them
  t = torch.arange(T, device='cuda').repeat_interleave(B)
  e = torch.arange(B, device='cuda').repeat(T)
  for dtype in DTYPES:
    for win in (Window(5, 5, _things(f)[0], pad=_pad_char(f)), Window(3, 4, (-1, f.cols - 2))):
      want = game.render_frame_windows(trace, t, e, win, obs_dtype=dtype)
      want = want.view(T, B, f.n_layers, win.height, win.width)
      assert _same(game.render_trace_windows(trace, win, obs_dtype=dtype), want), (dtype, win)
      assert _same(game.render_trace_windows(trace.contiguous(), win, obs_dtype=dtype), want), (dtype, win)
  f.check_actions()


def _state_cells(f):
  """The blob's per-state entries, int16 [S, 8] (campx_amd/wide.py table_arrays() has the layout)."""
  S = f.n_states
  off = (S * 5 * 8 + 15) // 16 * 16
  return f._tables[off:off + S * 16].view(torch.int16).view(S, 8)


@pytest.mark.parametrize('name', GAMES)
def test_all_states_equal_the_crop_of_render_states(name):
  game = _game(name)
  f = game.fused
  S, H, W = f.n_states, f.rows, f.cols
  cells = _state_cells(f)
  first = _rollout(name)[1]
  for d, ch in enumerate(_things(f)):
    layer = int(f.spec.dyn_layer[d])
    alone = sum(1 for k in range(f.n_dyn) if int(f.spec.dyn_layer[k]) == layer) == 1
    for dtype in DTYPES:
      full = _all_states(name, dtype)
      for (h, w), pad in (((5, 5), _pad_char(f)), (_odd_window(f), None), ((2 * H - 1, 2 * W - 1), None)):
        win = Window(h, w, ch, pad=pad)
        where = win.resolve(f.chars, f.spec)
        got = game.render_state_windows(win, obs_dtype=dtype)
        assert got.shape == (S, f.n_layers, h, w) and got.dtype == dtype
        # every state, the centre from the table's entries (a hidden thing included)
        r0, c0 = ref.centres(cells[:, d], W, H * W, h, w)
        assert _same(got, ref.crop(full, r0, c0, h, w, where.pad_layer)), (ch, dtype, win)
        # states where the thing shows: the centre read from the full observation itself
        if alone:
          plane = (_bits(full)[:, layer] != 0).reshape(S, -1)
          shows = plane.sum(1) == 1
          assert bool(shows.any())
          at = plane.long().argmax(1)[shows]
          want = ref.crop(full[shows], at // W - h // 2, at % W - w // 2, h, w, where.pad_layer)
          assert _same(got[shows], want), (ch, dtype, win)
          mine = (_bits(got)[shows][:, layer] != 0).reshape(int(shows.sum()), -1)
          assert bool((mine.sum(1) == 1).all())
          if pad is None or where.pad_layer != layer:
            assert bool(mine[:, (h // 2) * w + w // 2].all())        # ... at the window's centre
        # row 0 is the window of the its_showtime() frame
        assert _same(got[:1], ref.crop(first[None].to(dtype), r0[:1], c0[:1], h, w, where.pad_layer))
  f.check_actions()


@pytest.mark.parametrize('name', GAMES)
def test_state_windows_equal_frame_windows_of_the_frames_that_reached_them(name):
  game = _game(name)
  f = game.fused
  out = _rollout(name)[0]
  trace, done = out['trace'], out['done']
  tt = torch.arange(T - 1, device='cuda').repeat_interleave(B)
  ee = torch.arange(B, device='cuda').repeat(T - 1)
  ids = out['states'][1:].reshape(-1).contiguous()
  live = ~done[:T - 1].reshape(-1).bool()
  assert bool(live.any())
  for d, ch in enumerate(_things(f)):
    for dtype in DTYPES:
      for idx in (torch.int32, torch.int64):
        win = Window(5, 5, ch, pad=_pad_char(f))
        by_state = game.render_state_windows(win, ids.to(idx), obs_dtype=dtype)
        by_frame = game.render_frame_windows(trace, tt, ee, win, obs_dtype=dtype)
        assert _same(by_state[live], by_frame[live]), (ch, dtype, idx)
  f.check_actions()


@pytest.mark.parametrize('name', ['boat_race', 'pickups', 'variants'])
def test_bad_pairs_and_ids_are_clamped_counted_and_raise_by_name(name):
  game = _game(name)
  f = game.fused
  S = f.n_states
  trace = _rollout(name)[0]['trace']
  win = Window(5, 5, _things(f)[0], pad=_pad_char(f))
  t, e = _pairs(name, 300)
  t, e = t.clone(), e.clone()
  bad = {3: (-1, 0), 64: (T, 5), 255: (2, B), 256: (0, -7), 299: (T + 100, B + 100)}
  ct, ce = t.clone(), e.clone()
  for i, (bt, be) in bad.items():
    t[i], e[i] = bt, be
    ct[i], ce[i] = min(max(bt, 0), T - 1), min(max(be, 0), B - 1)
  f.check_actions()
  f.validate_actions = False
  try:
    for idx in (torch.int64, torch.int32):
      got = game.render_frame_windows(trace, t.to(idx), e.to(idx), win)
      assert _same(got, game.render_frame_windows(trace, ct, ce, win))
      with pytest.raises(ValueError, match=r'\b{} rows of render_frame_windows\(\)'.format(len(bad))):
        f.check_actions()
      f.check_actions()                        # counted once, then cleared
      assert int(f._bad_window_rows.item()) == 0
    ids = torch.randint(0, S, (300,), generator=torch.Generator().manual_seed(S)).cuda()
    clean = ids.clone()
    for i, v in {3: -1, 64: S, 255: 2 ** 31 - 1, 299: S + 10 ** 6}.items():
      ids[i], clean[i] = v, 0
    for idx in (torch.int64, torch.int32):
      got = game.render_state_windows(win, ids.to(idx))
      assert _same(got, game.render_state_windows(win, clean))
      with pytest.raises(ValueError, match=r'\b4 state ids of render_state_windows\(\)'):
        f.check_actions()
      f.check_actions()
      assert int(f._bad_window_ids.item()) == 0
    far = torch.tensor([1, 2 ** 32 + 1, -2 ** 40], dtype=torch.int64, device='cuda')
    assert _same(game.render_state_windows(win, far),
                 game.render_state_windows(win, torch.tensor([1, 0, 0], device='cuda')))
    with pytest.raises(ValueError, match=r'\b2 state ids of render_state_windows\(\)'):
      f.check_actions()
  finally:
    f.validate_actions = True
  f.validate_actions = 'sync'                  # 'sync' raises at once
  try:
    with pytest.raises(ValueError, match=r'\b1 state ids of render_state_windows\(\)'):
      game.render_state_windows(win, torch.tensor([S], device='cuda'))
    with pytest.raises(ValueError, match=r'\b1 rows of render_frame_windows\(\)'):
      game.render_frame_windows(trace, torch.tensor([T], device='cuda'), torch.tensor([0], device='cuda'), win)
  finally:
    f.validate_actions = True
  game.render_state_windows(win)               # the next call is clean
  f.check_actions()


@pytest.mark.parametrize('name', ['maze', 'pickups', 'variants'])
def test_out_receives_the_same_bits(name):
  game = _game(name)
  f = game.fused
  trace = _rollout(name)[0]['trace']
  t, e = _pairs(name)
  win = Window(5, 7, _things(f)[0], pad=_pad_char(f))
  for dtype in DTYPES:
    dst = torch.zeros((N_ROWS, f.n_layers, 5, 7), dtype=dtype, device='cuda')
    assert game.render_frame_windows(trace, t, e, win, out=dst) is dst
    assert _same(dst, game.render_frame_windows(trace, t, e, win, obs_dtype=dtype))
    dst = torch.zeros((T, B, f.n_layers, 5, 7), dtype=dtype, device='cuda')
    assert game.render_trace_windows(trace, win, out=dst) is dst
    assert _same(dst, game.render_trace_windows(trace, win, obs_dtype=dtype))
    dst = torch.zeros((f.n_states, f.n_layers, 5, 7), dtype=dtype, device='cuda')
    assert game.render_state_windows(win, out=dst) is dst
    assert _same(dst, game.render_state_windows(win, obs_dtype=dtype))
  f.check_actions()


def test_a_window_call_is_capturable_in_a_hip_graph():
  game = _game('maze')
  f = game.fused
  trace = _rollout('maze')[0]['trace']
  N = 1031
  win = Window(7, 7, _things(f)[0], pad=_pad_char(f))
  gen = torch.Generator().manual_seed(2)
  t = torch.randint(0, T, (N,), generator=gen).cuda()
  e = torch.randint(0, B, (N,), generator=gen).cuda()
  dst = torch.empty((N, f.n_layers, 7, 7), dtype=torch.bfloat16, device='cuda')
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    game.render_frame_windows(trace, t, e, win, out=dst)      # warm up outside the capture
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                               # one stream, no parallel branches
    assert game.render_frame_windows(trace, t, e, win, out=dst) is dst
  for seed in (3, 4):
    gen = torch.Generator().manual_seed(seed)
    t.copy_(torch.randint(0, T, (N,), generator=gen))
    e.copy_(torch.randint(0, B, (N,), generator=gen))
    dst.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(dst, game.render_frame_windows(trace, t, e, win, obs_dtype=torch.bfloat16))      # eager
  f.check_actions()


def test_argument_errors_and_the_other_tiers():
  game = _game('boat_race')
  f = game.fused
  trace = _rollout('boat_race')[0]['trace']
  t, e = _pairs('boat_race', 63)
  win = Window(3, 3, _things(f)[0])
  L = f.n_layers
  with pytest.raises(ValueError, match='window must be'):
    game.render_frame_windows(trace, t, e, (3, 3))
  with pytest.raises(ValueError, match='trace must be'):
    game.render_frame_windows(trace[:, :, :B - 1], t, e, win)
  with pytest.raises(ValueError, match='trace must be'):
    game.render_trace_windows(trace.to(torch.int32), win)
  with pytest.raises(ValueError, match='trace must be'):
    game.render_trace_windows(trace.cpu(), win)
  with pytest.raises(ValueError, match='t_idx and e_idx'):
    game.render_frame_windows(trace, t, e[:5], win)
  with pytest.raises(ValueError, match='t_idx and e_idx'):
    game.render_frame_windows(trace, t.to(torch.int16), e.to(torch.int16), win)
  with pytest.raises(ValueError, match='t_idx and e_idx'):
    game.render_frame_windows(trace, t, e.to(torch.int32), win)
  with pytest.raises(ValueError, match='state_ids'):
    game.render_state_windows(win, torch.zeros(3, dtype=torch.int16, device='cuda'))
  with pytest.raises(ValueError, match='state_ids'):
    game.render_state_windows(win, torch.zeros(3, dtype=torch.int64))
  with pytest.raises(ValueError, match='state_ids'):
    game.render_state_windows(win, [0, 1])
  with pytest.raises(ValueError, match='obs_dtype'):
    game.render_state_windows(win, obs_dtype=torch.float32)
  with pytest.raises(ValueError, match='out must be'):
    game.render_state_windows(win, out=torch.empty((f.n_states, L, 3, 4), dtype=torch.int8, device='cuda'))
  with pytest.raises(ValueError, match='out must be'):
    game.render_state_windows(win, out=torch.empty((f.n_states, L, 3, 3), dtype=torch.float32, device='cuda'))
  with pytest.raises(ValueError, match='out must be'):
    game.render_state_windows(win, out=torch.empty((f.n_states, L, 3, 3), dtype=torch.int8))
  with pytest.raises(ValueError, match='out must be'):
    game.render_frame_windows(trace, t, e, win,
                              out=torch.empty((63, L, 3, 6), dtype=torch.int8, device='cuda')[..., ::2])
  with pytest.raises(ValueError, match='out must be'):
    game.render_trace_windows(trace, win, out=torch.empty((T * B, L, 3, 3), dtype=torch.int8, device='cuda'))
  with pytest.raises(ValueError, match='is scenery'):
    game.render_state_windows(Window(3, 3, _pad_char(f)))
  with pytest.raises(ValueError, match='at most'):
    game.render_state_windows(Window(2 * f.rows, 3, _things(f)[0]))
  from campx_amd.games import boat_race
  plain = boat_race.build(64, 'cuda')            # the one-cell tier: no use_state_table()
  plain.its_showtime()
  with pytest.raises(NotImplementedError, match=r'render_state_windows\(\).*use_state_table'):
    plain.render_state_windows(win)
  with pytest.raises(NotImplementedError, match=r'render_frame_windows\(\)'):
    plain.render_frame_windows(None, t, e, win)
  with pytest.raises(NotImplementedError, match=r'render_trace_windows\(\)'):
    plain.render_trace_windows(None, win)
  from games_under_test import SHAPE_GAMES
  hello = SHAPE_GAMES['hello_world'](batch=64, device='cuda')
  hello.its_showtime()
  with pytest.raises(NotImplementedError, match=r'render_state_windows\(\)'):
    hello.render_state_windows(win)
  with pytest.raises(NotImplementedError, match=r'render_frame_windows\(\)'):
    hello.render_frame_windows(None, t, e, win)
  with pytest.raises(NotImplementedError, match=r'render_trace_windows\(\)'):
    hello.render_trace_windows(None, win)
  f.check_actions()
