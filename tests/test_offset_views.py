"""The one-shot render kernels into output VIEWS at every kind of 16-byte address, on the GPU.

gather_kernel (`render_frames()` on both tiers), window_kernel (the three `render_*_windows()`
calls) and render_kernel (`render_states()`, rollouts) cut their output into 2 KiB windows aligned
in memory; what they do for the first window hangs on the output's address modulo 2 048.  Every
other test hands them fresh allocations - multiples of 512.  Here the output is a view inside an
arena of 0xA5 bytes (tests/offset_views.py) at each residue of `RESIDUES`, in int8, float16 and
bfloat16; the expected rows come from the rollouts' own observations and from
tests/windows_reference.py, never from the same call into a fresh buffer (rollouts excepted, which
have no other reference: they are compared with the same rollout into the call's own buffer).
Every comparison is on bits, and after every call the arena outside the view is still 0xA5.

What this file found when it was written: window_kernel's 16-bit instances left elements 0..7 of
row 0 without scenery and padding wherever the output's address is 16 (mod 32) - NOTES.md has the
figures; k_window.hip now fills that chunk.

The games, rollouts and references are those of tests/test_windows.py, test_render_states.py and
test_gather_render.py."""

import functools

import pytest
import torch

from campx_amd.windows import Window
from test_render_states import B, T, _all_states, _bits, _game, _same

import offset_views as ov
import test_gather_render as tgr
import test_windows as tw
import windows_reference as ref

pytestmark = pytest.mark.gpu

DTYPES = ov.DTYPES
WIDE = tuple(ov.WIDE_GAMES)
# test_gather_render.py's names of the same games, which it rolls out WITH observations
ROLLED = {'maze': 'maze_16x16', 'pickups': 'pieces', 'variants': 'variants', 'maze_15x17': 'maze_15x17'}
ROLLED_BATCH = 1000


def _diff(got, want):
  """Where two tensors first differ, for the assertion's message."""
  if got.shape != want.shape or got.dtype != want.dtype:
    return 'got {} {}, want {} {}'.format(got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
  a, b = _bits(got).reshape(-1), _bits(want).reshape(-1)
  ne = (a != b).nonzero().reshape(-1)
  if ne.numel() == 0:
    return 'equal'
  at = int(ne[0])
  mask = 0xffff if got.element_size() == 2 else 0xff
  return '{} elements differ, {}..{}; the first, {}: got 0x{:x}, want 0x{:x}'.format(
      int(ne.numel()), at, int(ne[-1]), at, int(a[at]) & mask, int(b[at]) & mask)


def _into(shape, dtype, residue, call):
  """`call(out)` on a view of `shape` at `residue`: the view, after the canaries were looked at."""
  view, arena, start = ov.arena_view(shape, dtype, residue, 'cuda')
  assert call(view) is view
  torch.cuda.synchronize()
  assert ov.untouched(arena, start, ov.nbytes(view)), 'bytes outside the view were written'
  return view


def _check(got, want, what):
  assert _same(got, want), (what, _diff(got, want))


def test_the_case_list_names_the_games_as_built():
  """tests/test_offset_views_cpu.py examines the plans of these sizes."""
  for name, dims in list(ov.WIDE_GAMES.items()) + list(ov.LONG_ROWS.items()):
    f = _game(name).fused
    assert (f.n_layers, f.rows, f.cols, f.n_states) == dims, (name, f.n_layers, f.rows, f.cols, f.n_states)
    g = tgr._rolled(ROLLED[name], ROLLED_BATCH)[0].fused
    assert (g.n_layers, g.rows, g.cols) == dims[:3], name
  for name, dims in ov.ONE_CELL_GAMES.items():
    f = tgr._rolled(name, ROLLED_BATCH)[0].fused
    assert (f.n_layers, f.rows, f.cols) == dims, (name, f.n_layers, f.rows, f.cols)
  assert B == ov.BATCH and T >= ov.TRACE_FRAMES + 1


# ------------------------------------------------------------------ windows

@functools.lru_cache(maxsize=None)
def _windows(name):
  """The windows of a game: (3, 3), the odd one, the largest with and without padding, and a fixed
  one that hangs off the board's top-left corner."""
  f = _game(name).fused
  things, pad = tw._things(f), tw._pad_char(f)
  shapes = ov.window_shapes(f.n_layers, f.rows, f.cols)
  assert shapes[1] == tw._odd_window(f)
  big = shapes[2]
  return (Window(3, 3, things[0]), Window(shapes[1][0], shapes[1][1], things[-1], pad=pad),
          Window(big[0], big[1], things[0], pad=pad), Window(big[0], big[1], things[-1]),
          Window(ov.CORNER_SHAPE[0], ov.CORNER_SHAPE[1], ov.CORNER, pad=pad))


@functools.lru_cache(maxsize=None)
def _want_frame_windows(name, dtype, N, k):
  """tests/test_windows.py's expectation: the crop of the full frames."""
  t, e = tw._pairs(name, N)
  return tw._want_frames(name, dtype, _windows(name)[k], t, e, tw._full_frames(name, dtype, N))


@functools.lru_cache(maxsize=None)
def _trace_pairs():
  t = torch.arange(ov.TRACE_FRAMES, device='cuda').repeat_interleave(B)
  e = torch.arange(B, device='cuda').repeat(ov.TRACE_FRAMES)
  return t, e


@functools.lru_cache(maxsize=None)
def _want_trace_windows(name, dtype, k):
  game = _game(name)
  f = game.fused
  win = _windows(name)[k]
  t, e = _trace_pairs()
  full = game.render_frames(tw._rollout(name)[0]['trace'], t, e, obs_dtype=dtype)
  want = tw._want_frames(name, dtype, win, t, e, full)
  return want.view(ov.TRACE_FRAMES, B, f.n_layers, win.height, win.width)


@functools.lru_cache(maxsize=None)
def _state_ids(name, N):
  S = _game(name).fused.n_states
  ids = torch.randint(0, S, (N,), generator=torch.Generator().manual_seed(S + N))
  ids[N // 2:] = ids[:N - N // 2].flip(0)
  return ids.cuda()


@functools.lru_cache(maxsize=None)
def _want_state_windows(name, dtype, k, N):
  """The crop of render_states()'s rows (N None: of all states), the centre from the table's entries."""
  f = _game(name).fused
  win = _windows(name)[k]
  where = win.resolve(f.chars, f.spec)
  full, cells = _all_states(name, dtype), tw._state_cells(f)
  if N is not None:
    ids = _state_ids(name, N)
    full, cells = full[ids], cells[ids]
  if where.thing >= 0:
    r0, c0 = ref.centres(cells[:, where.thing], f.cols, f.rows * f.cols, win.height, win.width)
  else:
    r0, c0 = where.r0, where.c0
  return ref.crop(full, r0, c0, win.height, win.width, where.pad_layer)


@pytest.mark.parametrize('residue', ov.RESIDUES)
@pytest.mark.parametrize('name', WIDE)
def test_frame_windows_into_offset_views(name, residue):
  game = _game(name)
  f = game.fused
  trace = tw._rollout(name)[0]['trace']
  for N in ov.WINDOW_ROWS:
    t, e = tw._pairs(name, N)
    for dtype in DTYPES:
      for k, win in enumerate(_windows(name)):
        got = _into((N, f.n_layers, win.height, win.width), dtype, residue,
                    lambda out: game.render_frame_windows(trace, t, e, win, out=out))
        _check(got, _want_frame_windows(name, dtype, N, k), (N, dtype, win))
  f.check_actions()


@pytest.mark.parametrize('residue', ov.RESIDUES)
@pytest.mark.parametrize('name', WIDE)
def test_state_windows_into_offset_views(name, residue):
  game = _game(name)
  f = game.fused
  for dtype in DTYPES:
    for k, win in enumerate(_windows(name)):
      N = ov.STATE_ROWS[-1]
      got = _into((N, f.n_layers, win.height, win.width), dtype, residue,
                  lambda out: game.render_state_windows(win, _state_ids(name, N), out=out))
      _check(got, _want_state_windows(name, dtype, k, N), ('ids', dtype, win))
      got = _into((f.n_states, f.n_layers, win.height, win.width), dtype, residue,
                  lambda out: game.render_state_windows(win, out=out))
      _check(got, _want_state_windows(name, dtype, k, None), ('all states', dtype, win))
  f.check_actions()


@pytest.mark.parametrize('residue', ov.RESIDUES)
@pytest.mark.parametrize('name', WIDE)
def test_trace_windows_into_offset_views(name, residue):
  game = _game(name)
  f = game.fused
  trace = tw._rollout(name)[0]['trace'][:, :ov.TRACE_FRAMES]
  for dtype in DTYPES:
    for k, win in enumerate(_windows(name)):
      got = _into((ov.TRACE_FRAMES, B, f.n_layers, win.height, win.width), dtype, residue,
                  lambda out: game.render_trace_windows(trace, win, out=out))
      _check(got, _want_trace_windows(name, dtype, k), (dtype, win))
  f.check_actions()


# ------------------------------------------------------------------ gather

@functools.lru_cache(maxsize=None)
def _gather_pairs(name, N):
  """Rows of the first rollout of tests/test_gather_render.py's game, drawn WITH repeats."""
  frames = tgr._frames(name)
  gen = torch.Generator().manual_seed(N + len(name))
  t = torch.randint(0, frames, (N,), generator=gen)
  e = torch.randint(0, ROLLED_BATCH, (N,), generator=gen)
  t[N // 2:] = t[:N - N // 2].flip(0)
  e[N // 2:] = e[:N - N // 2].flip(0)
  return t.cuda(), e.cuda()


@pytest.mark.parametrize('residue', ov.RESIDUES)
@pytest.mark.parametrize('name', list(ROLLED.values()) + list(ov.ONE_CELL_GAMES))
def test_render_frames_into_offset_views(name, residue):
  """Both tiers; expected: the rollout's own observation rows."""
  game, outs = tgr._rolled(name, ROLLED_BATCH)
  obs, trace = outs[0]['obs'], outs[0]['trace']
  for N in ov.GATHER_ROWS:
    t, e = _gather_pairs(name, N)
    for dtype in DTYPES:
      got = _into((N,) + tuple(obs.shape[2:]), dtype, residue,
                  lambda out: game.render_frames(trace, t, e, out=out))
      _check(got, tgr._expect(obs, t, e, dtype), (N, dtype))
  game.fused.check_actions()


@functools.lru_cache(maxsize=None)
def _reached(name, N):
  """(state ids, frame, environment) of N rows of tests/test_windows.py's rollout, with repeats:
  `states[t + 1]` is the state frame t reached, or the reset state behind an episode's end."""
  out = tw._rollout(name)[0]
  gen = torch.Generator().manual_seed(7 * N + len(name))
  t = torch.randint(0, T - 1, (N,), generator=gen)
  e = torch.randint(0, B, (N,), generator=gen)
  t[N // 2:] = t[:N - N // 2].flip(0)
  e[N // 2:] = e[:N - N // 2].flip(0)
  t, e = t.cuda(), e.cuda()
  return out['states'][t + 1, e].contiguous(), out['done'][t, e].bool(), t, e


@pytest.mark.parametrize('residue', ov.RESIDUES)
@pytest.mark.parametrize('name', WIDE + tuple(ov.LONG_ROWS))
def test_render_states_into_offset_views(name, residue):
  """Expected, as test_states_of_a_policy_rollout_against_its_rendered_trace has it: the rendered
  frame that reached the state, and the its_showtime() frame behind an episode's end."""
  game = _game(name)
  f = game.fused
  out, first = tw._rollout(name)
  shape = (f.n_layers, f.rows, f.cols)
  for dtype in DTYPES:
    for N in ov.STATE_ROWS:
      ids, over, t, e = _reached(name, N)
      want = game.render_frames(out['trace'], t, e, obs_dtype=dtype)
      want[over] = first.to(dtype)
      got = _into((N,) + shape, dtype, residue, lambda o: game.render_states(ids, out=o))
      _check(got, want, (N, dtype))
    got = _into((f.n_states,) + shape, dtype, residue, lambda o: game.render_states(out=o))
    _check(got, _all_states(name, dtype), ('all states', dtype))
    _check(got[:1], first[None].to(dtype), ('state 0', dtype))
  f.check_actions()


# ------------------------------------------------------------------ bad indices under a shift

BAD_ROWS = 65
BAD_AT = (0, 1, 20, 21, 40, 63, 64)          # row 0 and the last row among them


def _raises_count(f, pattern):
  with pytest.raises(ValueError, match=pattern):
    f.check_actions()
  f.check_actions()                          # counted once, then cleared


@pytest.mark.parametrize('residue', [16, 2032])
def test_bad_pairs_under_a_shift_in_window_kernel(residue):
  """"A row is counted by the one wave whose window it starts in" hangs on the first window's
  start: exactly 7, not 6 (row 0 missed) and not 8 (a row counted by both waves it lies in)."""
  name = 'pickups'
  game = _game(name)
  f = game.fused
  trace = tw._rollout(name)[0]['trace']
  win = Window(5, 5, tw._things(f)[0], pad=tw._pad_char(f))
  t, e = (x.clone() for x in tw._pairs(name, BAD_ROWS))
  ct, ce = t.clone(), e.clone()
  bad = [(-1, 0), (T, 5), (2, B), (0, -7), (T + 100, B + 100), (-2 ** 31, 3), (T - 1, 2 ** 31 - 1)]
  for i, (bt, be) in zip(BAD_AT, bad):
    t[i], e[i] = bt, be
    ct[i], ce[i] = min(max(bt, 0), T - 1), min(max(be, 0), B - 1)
  ids = _state_ids(name, BAD_ROWS).clone()
  clean = ids.clone()
  for i, v in zip(BAD_AT, (-1, f.n_states, 2 ** 31 - 1, -2 ** 31, f.n_states + 10 ** 6, -5, f.n_states + 1)):
    ids[i], clean[i] = v, 0
  shape = (BAD_ROWS, f.n_layers, 5, 5)
  f.check_actions()
  f.validate_actions = False
  try:
    for dtype in DTYPES:
      full = game.render_frames(trace, ct, ce, obs_dtype=dtype)
      want = tw._want_frames(name, dtype, win, ct, ce, full)
      for idx in (torch.int64, torch.int32):
        got = _into(shape, dtype, residue,
                    lambda out: game.render_frame_windows(trace, t.to(idx), e.to(idx), win, out=out))
        _check(got, want, (dtype, idx))
        _raises_count(f, r'\b{} rows of render_frame_windows\(\)'.format(len(BAD_AT)))
        got = _into(shape, dtype, residue, lambda out: game.render_state_windows(win, ids.to(idx), out=out))
        where = win.resolve(f.chars, f.spec)
        r0, c0 = ref.centres(tw._state_cells(f)[clean][:, where.thing], f.cols, f.rows * f.cols, 5, 5)
        _check(got, ref.crop(_all_states(name, dtype)[clean], r0, c0, 5, 5, where.pad_layer), (dtype, idx))
        _raises_count(f, r'\b{} state ids of render_state_windows\(\)'.format(len(BAD_AT)))
  finally:
    f.validate_actions = True
  f.check_actions()


@pytest.mark.parametrize('residue', [16, 2032])
@pytest.mark.parametrize('name', ['boat_race', 'variants'])
def test_bad_pairs_under_a_shift_in_gather_kernel(name, residue):
  game, outs = tgr._rolled(name, ROLLED_BATCH)
  f = game.fused
  obs, trace = outs[0]['obs'], outs[0]['trace']
  frames, batch = tgr._frames(name), ROLLED_BATCH
  t, e = (x.clone() for x in _gather_pairs(name, BAD_ROWS))
  bad = [(-1, 0), (frames, 5), (2, batch), (0, -7), (frames + 10 ** 6, batch + 10 ** 6), (-2 ** 31, 3),
         (frames - 1, 2 ** 31 - 1)]
  for i, (bt, be) in zip(BAD_AT, bad):
    t[i], e[i] = bt, be
  ct, ce = t.clamp(0, frames - 1), e.clamp(0, batch - 1)
  f.check_actions()
  f.validate_actions = False
  try:
    for dtype in DTYPES:
      for idx in (torch.int64, torch.int32):
        got = _into((BAD_ROWS,) + tuple(obs.shape[2:]), dtype, residue,
                    lambda out: game.render_frames(trace, t.to(idx), e.to(idx), out=out))
        _check(got, tgr._expect(obs, ct, ce, dtype), (dtype, idx))
        _raises_count(f, r'\b{} rows of render_frames'.format(len(BAD_AT)))
  finally:
    f.validate_actions = True
  f.check_actions()


# ------------------------------------------------------------------ rollouts

ROLLOUT_BATCH, ROLLOUT_FRAMES = 65, 3


@functools.lru_cache(maxsize=None)
def _small(name):
  """The maze on its state table and the one-cell boat race, 65 environments."""
  if name == 'maze':
    from campx_amd.games import maze
    game = maze.build(16, 16, batch=ROLLOUT_BATCH, device='cuda')
  else:
    from campx_amd.games import boat_race
    game = boat_race.build(ROLLOUT_BATCH, 'cuda')
  game.its_showtime()
  return game


@pytest.mark.parametrize('residue', [16, 1040, 2032])
@pytest.mark.parametrize('dtype', [torch.int8, torch.float16], ids=['int8', 'f16'])
@pytest.mark.parametrize('name', ['maze', 'boat_race'])
def test_rollouts_into_offset_views(name, dtype, residue):
  """`rollout(actions, obs=view)` takes a destination it did not allocate (no refusal to assert):
  the same rollout from the same state into the call's own buffer is the reference.  65 boat-race
  frames are 11 375 bytes - frames that are no whole chunks, every one at another shift."""
  from campx_amd import wide
  game = _small(name)
  f = game.fused
  assert isinstance(f, wide.WideGame) == (name == 'maze')
  gen = torch.Generator().manual_seed(len(name))
  acts = torch.randint(0, 5, (ROLLOUT_FRAMES, ROLLOUT_BATCH), generator=gen, dtype=torch.int8).cuda()
  own = game.rollout(acts, obs_dtype=dtype, reset_first=True)
  torch.cuda.synchronize()
  want = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in own.items()}
  assert want['obs'].dtype == dtype and len(torch.unique(_bits(want['obs']).reshape(ROLLOUT_FRAMES, -1), dim=0)) > 1
  shape = (ROLLOUT_FRAMES, ROLLOUT_BATCH, f.n_layers, f.rows, f.cols)
  view, arena, start = ov.arena_view(shape, dtype, residue, 'cuda')
  got = game.rollout(acts, obs=view, obs_dtype=dtype, reset_first=True)
  torch.cuda.synchronize()
  assert got['obs'] is view
  assert ov.untouched(arena, start, ov.nbytes(view)), 'bytes outside the view were written'
  _check(view, want['obs'], (name, dtype))
  for k in ('reward', 'discount', 'done', 'trace'):
    if want[k] is not None:
      assert torch.equal(got[k].view(torch.uint8) if got[k].dtype == torch.float32 else got[k],
                         want[k].view(torch.uint8) if want[k].dtype == torch.float32 else want[k]), k
  f.check_actions()


# ------------------------------------------------------------------ a view that is not 16-byte aligned

@pytest.mark.parametrize('dtype,skew', [(torch.int8, 8), (torch.float16, 2)], ids=['int8+8', 'f16+2'])
def test_a_view_that_is_not_16_byte_aligned_is_refused_untouched(dtype, skew):
  """The contract is 16 bytes (include/campx_hip.h): one call of each family raises, and nothing
  - view included - was written."""
  game = _game('pickups')
  f = game.fused
  L, H, W = f.n_layers, f.rows, f.cols
  trace = tw._rollout('pickups')[0]['trace']
  win = Window(3, 3, tw._things(f)[0])
  N = 65
  t, e = tw._pairs('pickups', N)
  one, outs = tgr._rolled('boat_race', ROLLED_BATCH)
  t1, e1 = _gather_pairs('boat_race', N)
  small = _small('boat_race')
  acts = torch.zeros((ROLLOUT_FRAMES, ROLLOUT_BATCH), dtype=torch.int8, device='cuda')
  state = (small.fused.pos.clone(), small.fused.frame)
  calls = [
      ((N, L, 3, 3), lambda out: game.render_frame_windows(trace, t, e, win, out=out)),
      ((N, L, 3, 3), lambda out: game.render_state_windows(win, _state_ids('pickups', N), out=out)),
      ((ov.TRACE_FRAMES, B, L, 3, 3),
       lambda out: game.render_trace_windows(trace[:, :ov.TRACE_FRAMES], win, out=out)),
      ((N, L, H, W), lambda out: game.render_frames(trace, t, e, out=out)),
      ((N, L, H, W), lambda out: game.render_states(_state_ids('pickups', N), out=out)),
      ((N,) + tuple(outs[0]['obs'].shape[2:]), lambda out: one.render_frames(outs[0]['trace'], t1, e1, out=out)),
      ((ROLLOUT_FRAMES, ROLLOUT_BATCH, small.fused.n_layers, small.fused.rows, small.fused.cols),
       lambda out: small.rollout(acts, obs=out, obs_dtype=dtype)),
  ]
  for i, (shape, call) in enumerate(calls):
    view, arena, start = ov.arena_view(shape, dtype, 16, 'cuda', skew=skew)
    assert view.data_ptr() % 16 == skew
    with pytest.raises((RuntimeError, ValueError)):
      call(view)
    torch.cuda.synchronize()
    assert ov.all_canary(arena), i
  # the refused rollout advanced nothing
  assert torch.equal(small.fused.pos, state[0]) and small.fused.frame == state[1]
  f.check_actions()
  one.fused.check_actions()
  small.fused.check_actions()
