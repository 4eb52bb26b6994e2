"""Every reader of an int8 action stream, given streams at every kind of BYTE address, on the GPU.

Every other test hands the kernels a fresh allocation: a multiple of 512 bytes with whatever the
allocator left behind it.  Here the stream is a view inside an arena (tests/action_views.py) at
each offset of `OFFSETS` modulo 16 - and, for a batch that is no multiple of 16, at the offset that
ends it on a 16-byte boundary, where a 16-byte load one byte too far would still be "aligned" -
between guards of 0xA5 (a bad id: a stray byte that is counted shows in the count) or of 0x01 (a
legal move: a stray byte that is used shows in the outputs).  The shapes are the smallest at which
each branch of csrc/k_update.hip's ActionLoader exists; tests/test_action_views_cpu.py asserts
that they reach them all.

Two things are checked of every call, and nothing with a tolerance:

  * the outputs, on bits, against the C oracle on `cleaned = where(bad, 4, dirty)` - a bad id acts
    as "stay" (include/campx_hip.h), and the oracle itself refuses one;
  * with `validate_actions` on, the device counter after a synchronise: EXACTLY numpy's count of
    `(a < 0) | (a > 4)`; then `check_actions()` raises with that number and leaves the counter 0.
    (The flag the kernels raise sits in pinned host memory and the call that launched them looks
    at it on its way out: when it is already up the call itself raises, with the same number,
    and clears the counter - `_Count` takes both.)

A trace has no oracle; `_want_trace()` takes the one `rollout_trace()` makes of the cleaned stream in
a fresh allocation once it renders, through `render_frames()`, to exactly the oracle's frames.

The shape tier is the one reader whose bad ids do not act as action 4 - Hello World's 4 is "quit";
an id outside 0..4 moves nothing, pays None and ends nothing (csrc/k_shape.hip;
tests/test_shape_parity.py test_bad_action_ids_move_nothing_and_are_counted).  Its reference is
the oracle on each environment's stream WITHOUT the bad frames, with those frames put back as
repeats of the frame before them (`_shape_want`).

tests/action_views_big_check.py runs the 512-environment workgroups in processes of their own."""

import contextlib
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from campx_amd import _hip, gamespec
from games_under_test import FUSED_GAMES, SHAPE_GAMES, WIDE_GAMES
from oracle import cpu

import action_views as av

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TABLE_GAMES = ('boat_race', 'sokoban', 'sokoban_l2')      # update_table, update_pair, update_tuple
BIG_FORM_GAMES = TABLE_GAMES[:2]                          # the kernels that have a 512-environment form
BUILDERS = dict(FUSED_GAMES, maze=WIDE_GAMES['maze_16x16'], hello_world=SHAPE_GAMES['hello_world'])
STREAMS = (('clean', 'clean'), ('dirty', 'cleaned'))      # (what the kernels get, what the oracle gets)


# ------------------------------------------------------------------ games and references

@contextlib.contextmanager
def _single_kernel(table):
  """Rollouts in the single fused kernel - the rule interpreter (csrc/k_interp.hip) or, with
  `table`, the game's table (csrc/k_rollout_table.hip) -, as tests/test_fused_parity.py's fixtures
  set it: for building a game and for every call on it."""
  from campx_amd import fused
  saved = fused.COMPILE_TABLE, fused.SPLIT_ROLLOUT
  fused.COMPILE_TABLE, fused.SPLIT_ROLLOUT = table, False
  try:
    yield
  finally:
    fused.COMPILE_TABLE, fused.SPLIT_ROLLOUT = saved


@functools.lru_cache(maxsize=None)
def _game(key, B):
  """`key`: a name of BUILDERS, or name/interp (no table, one kernel), name/fused (its table, one
  kernel), name/states (on its state table), name/serial (the shape tier without its frame-major
  path)."""
  from campx_amd import shapes, wide
  name, _, mode = key.partition('/')
  if mode in ('interp', 'fused'):
    with _single_kernel(mode == 'fused'):
      game = BUILDERS[name](batch=B, device='cuda')
      game.its_showtime()
    assert game.fused.uses_table == (mode == 'fused')
  elif mode == 'serial':
    saved, shapes.FRAME_MAJOR = shapes.FRAME_MAJOR, False
    try:
      game = BUILDERS[name](batch=B, device='cuda')
      game.its_showtime()
    finally:
      shapes.FRAME_MAJOR = saved
    assert game.fused._tables is None
  else:
    game = BUILDERS[name](batch=B, device='cuda')
    if mode == 'states':
      game.use_state_table()
    game.its_showtime()
    if name in TABLE_GAMES and not mode:
      assert game.fused.uses_table
  assert isinstance(game.fused, wide.WideGame) == (mode == 'states' or name == 'maze')
  assert isinstance(game.fused, shapes.ShapeGame) == (name == 'hello_world')
  return game


@functools.lru_cache(maxsize=None)
def _oracle(name):
  return cpu.OracleGame.from_description(gamespec.describe(BUILDERS[name]()))


@functools.lru_cache(maxsize=None)
def _streams(T, B):
  return av.streams(T, B, 1000 * T + B)


def _gpu(x):
  return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def _want(name, T, B, which):
  """The oracle's streams of outputs for `_streams(T, B)[which]`, on the device."""
  ref = _oracle(name).rollout(_streams(T, B)[which], reset_first=True, want_board=False)
  return {k: _gpu(ref[k]) for k in ('obs', 'reward', 'discount', 'done', 'perf')}


def _shape_want_arrays(og, dirty):
  """Hello World's frames for a stream with bad ids in it: the oracle on every environment's
  stream without its bad frames (the tail filled with action 0 and ignored); a bad frame then
  repeats the frame before it - the first frame of a new game at frame 0 and behind a frame that
  ended the episode, which the kernel rebuilds from whatever the id - pays None (NaN), discounts
  by 1 and ends nothing."""
  T, B = dirty.shape
  bad = (dirty < 0) | (dirty > 4)
  packed = np.zeros_like(dirty)
  for e in range(B):
    keep = dirty[~bad[:, e], e]
    packed[:len(keep), e] = keep
  ref = og.rollout(packed, reset_first=True, want_board=False)
  first = og.first_frame()[0]
  j = np.cumsum(~bad, axis=0) - 1
  out = {k: np.empty_like(ref[k]) for k in ('obs', 'reward', 'discount', 'done')}
  for t in range(T):
    ok = np.nonzero(~bad[t])[0]
    for k in out:
      out[k][t, ok] = ref[k][j[t, ok], ok]
    no = np.nonzero(bad[t])[0]
    if t == 0:
      out['obs'][t, no] = first
    else:
      fresh = out['done'][t - 1, no] == 1
      out['obs'][t, no] = np.where(fresh[:, None, None, None], first[None], out['obs'][t - 1, no])
    out['reward'][t, no] = np.float32('nan')
    out['discount'][t, no] = 1.0
    out['done'][t, no] = 0
  return out


@functools.lru_cache(maxsize=None)
def _shape_want(T, B, given):
  og = _oracle('hello_world')
  if given == 'clean':
    ref = og.rollout(_streams(T, B)['clean'], reset_first=True, want_board=False)
  else:
    ref = _shape_want_arrays(og, _streams(T, B)['dirty'])
  return {k: _gpu(ref[k]) for k in ('obs', 'reward', 'discount', 'done')}


def _bits(t):
  return t.view(torch.int32) if t.dtype == torch.float32 else t


def _keys(f, obs=True, trace=False):
  """The streams a call on game `f` must hand back and the reference must have."""
  return ((('obs',) if obs else ()) + ('reward', 'discount', 'done') +
          (('perf',) if f.has_perf else ()) + (('trace',) if trace else ()))


def _compare(got, want, keys, what):
  """Every stream of `keys` - each one there on both sides - on bits."""
  for k in keys:
    g, w = got.get(k), want.get(k)
    assert g is not None and w is not None, (what, k, 'missing', g is None, w is None)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, g.dtype, w.shape, w.dtype)
    assert torch.equal(_bits(g), _bits(w)), (what, k, int((_bits(g) != _bits(w)).sum()))


@functools.lru_cache(maxsize=None)
def _want_trace(key, T, B, which):
  """The trace of `_streams(T, B)[which]` - free of bad ids - from a fresh allocation, taken for
  the reference once its frames, rendered through render_frames(), are the oracle's."""
  game = _game(key, B)
  f = game.fused
  out = f.rollout_trace(_gpu(_streams(T, B)[which]), reset_first=True)
  t = torch.arange(T, device='cuda').repeat_interleave(B)
  e = torch.arange(B, device='cuda').repeat(T)
  frames = game.render_frames(out['trace'], t, e)
  want = _want(key.partition('/')[0], T, B, which)
  assert torch.equal(frames.view(want['obs'].shape), want['obs']), (key, T, B, which)
  _compare(out, want, _keys(f, obs=False), (key, T, B, which, 'reference trace'))
  f.check_actions()
  return out['trace'].clone()


# ------------------------------------------------------------------ the exact count

class _Count(object):
  """The bad ids of the calls run through it: what the calls themselves raised (the pinned flag
  was already up when they looked; `_raise_bad()` then reads and clears the counter) plus what the
  device counter holds after a synchronise."""

  def __init__(self, f):
    self.f, self.raised = f, 0
    assert f.validate_actions is True and int(f._bad.item()) == 0

  def run(self, call):
    try:
      return call()
    except ValueError as e:
      n = re.match(r'(\d+) action ids are outside 0\.\.4', str(e))
      assert n, str(e)
      self.raised += int(n.group(1))

  def settle(self, n_bad, what):
    f = self.f
    torch.cuda.synchronize()
    left = int(f._bad.item())
    assert self.raised + left == n_bad, (what, 'counted', self.raised, left, 'bad ids', n_bad)
    if left:
      with pytest.raises(ValueError, match=r'^{} action ids are outside 0\.\.4'.format(left)):
        f.check_actions()
    assert int(f._bad.item()) == 0 and int(f._bad_flag_view[0]) == 0, what
    f.check_actions()


def _launch(f, run, n_bad, what, **settings):
  c = _Count(f)
  with _hip.config(**settings):
    c.run(run)
  c.settle(n_bad, what)


def _views(T, B, fill, offsets=None, streams=STREAMS, flat=False):
  """(view, arena/start/src for the guards, given, wanted, n_bad, offset) of every stream at every offset."""
  s = _streams(T, B)
  for given, wanted in streams:
    a = s[given][0] if flat else s[given]
    for offset in (av.offsets_for(T, B) if offsets is None else offsets):
      view, arena, start = av.action_view(a, offset, fill, 'cuda')
      yield view, (arena, start, view.clone()), given, wanted, (s['n_bad'] if given == 'dirty' else 0), offset


def _unharmed(view, kept, fill, what):
  """No reader writes: the stream and its guards are what they were."""
  arena, start, src = kept
  assert torch.equal(view, src) and av.guards_hold(arena, start, view.numel(), fill), what


def _rollout(f, view, T):
  bufs = f.rollout_buffers(T)
  return bufs, lambda: f.rollout(view, out=bufs, reset_first=True)


def _rollout_trace(f, view, T):
  bufs = f.rollout_trace_buffers(T)
  return bufs, lambda: f.rollout_trace(view, reset_first=True, out=bufs)


# ------------------------------------------------------------------ 1. the table kernels

def _table_game_cases(name, B, fill, frames):
  game = _game(name, B)
  f = game.fused
  for T in frames:
    for view, kept, given, wanted, n_bad, offset in _views(T, B, fill):
      want = dict(_want(name, T, B, wanted), trace=_want_trace(name, T, B, wanted))
      what = (name, T, B, offset, hex(fill), given)
      # the default: one launch where the library has one for the game at this size
      bufs, run = _rollout(f, view, T)
      _launch(f, run, n_bad, what + ('rollout',))
      _compare(bufs, want, _keys(f, trace=True), what + ('rollout',))
      # update pass, then render
      bufs, run = _rollout(f, view, T)
      _launch(f, run, n_bad, what + ('flow=0',), flow=0)
      _compare(bufs, want, _keys(f, trace=True), what + ('flow=0',))
      # the update pass alone
      bufs, run = _rollout_trace(f, view, T)
      _launch(f, run, n_bad, what + ('rollout_trace',))
      _compare(bufs, want, _keys(f, obs=False, trace=True), what + ('rollout_trace',))
      _unharmed(view, kept, fill, what)


def test_the_default_rollout_is_one_launch_where_frames_are_whole_chunks():
  """Of the grid's batches 16 and 256 (and 512 in the child process) take the one-launch form by
  default - it wants a batch's frame to be whole 16-byte chunks -, the others two kernels."""
  for name in ('boat_race', 'sokoban'):
    for B in (16, 256, 257):
      f = _game(name, B).fused
      assert f._one_launch(65, f.rollout_buffers(65)['trace'].stride(1)) == (B != 257), (name, B)


@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.BATCHES)
def test_boat_race_table_kernel_on_the_full_grid(B, fill):
  _table_game_cases('boat_race', B, fill, av.FRAMES)


@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.BATCHES)
@pytest.mark.parametrize('name', ['sokoban', 'sokoban_l2'])
def test_pair_and_tuple_kernels(name, B, fill):
  _table_game_cases(name, B, fill, av.FEW_FRAMES)


@pytest.mark.parametrize('name,B', [(name, B) for name in ('boat_race', 'sokoban') for B in av.DEFERRED_BATCHES]
                         + [(name, B) for name in sorted(av.DEFERRED_SHARED) for B in av.DEFERRED_SHARED[name]])
def test_deferred_rollouts(name, B):
  """Two calls, so that the second is the shared launch where the library has one - this rollout's
  update pass beside the previous one's render: `DEFERRED_SHARED`, batches whose frames are whole
  16-byte chunks -; the count is read after flush()."""
  f = _game(name, B).fused
  shared = bool(_hip.lib.campx_update_render_shared(ctypes.byref(f.spec), B, 65))
  assert shared == (B in av.DEFERRED_SHARED[name]), (name, B)
  for T in av.FEW_FRAMES:
    want = dict(_want(name, T, B, 'cleaned'), trace=_want_trace(name, T, B, 'cleaned'))
    for fill in av.FILLS:
      for view, kept, given, wanted, n_bad, offset in _views(T, B, fill, streams=STREAMS[1:]):
        what = (name, T, B, offset, hex(fill), 'deferred')
        one, two = f.rollout_buffers(T), f.rollout_buffers(T)
        c = _Count(f)
        c.run(lambda: f.rollout_deferred(view, one, reset_first=True))
        c.run(lambda: f.rollout_deferred(view, two, reset_first=True))
        assert f.flush() is two
        c.settle(2 * n_bad, what)
        _compare(one, want, _keys(f, trace=True), what + (1,))
        _compare(two, want, _keys(f, trace=True), what + (2,))
        _unharmed(view, kept, fill, what)


# ------------------------------------------------------------------ 2. the other readers

@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.STAGED_BATCHES)
@pytest.mark.parametrize('name', ['boat_race', 'sokoban'])
@pytest.mark.parametrize('mode', ['interp', 'fused'])
def test_single_fused_kernel(mode, name, B, fill):
  """Both instances of stage_actions() - the rule interpreter's (csrc/k_interp.hip) and, with the
  game's table, csrc/k_rollout_table.hip's: rows clamped past T, both sides of its 16-row split."""
  with _single_kernel(mode == 'fused'):
    f = _game(name + '/' + mode, B).fused
    for T in av.STAGED_FRAMES:
      for view, kept, given, wanted, n_bad, offset in _views(T, B, fill):
        what = (name, T, B, offset, hex(fill), given, mode)
        bufs, run = _rollout(f, view, T)
        assert bufs['trace'] is None
        _launch(f, run, n_bad, what)
        _compare(bufs, _want(name, T, B, wanted), _keys(f), what)
        _unharmed(view, kept, fill, what)


def _play_cases(key, B, fill, frame_of):
  """play() with a [B] view after reset(): frame 0 of the oracle's one-frame rollout.

  play() hands back views of the game's own buffers, which never move (a caller may keep the
  Observation across calls): one play() of a fresh stream in front takes them, and every call
  under test is then read through them - the same way whether or not the call raised for the
  bad ids it had already been told of on its way out."""
  name = key.partition('/')[0]
  f = _game(key, B).fused
  f.reset()
  obs, reward, discount = f.play(torch.zeros((B,), dtype=torch.int8, device='cuda'))
  got = dict(obs=obs.layered_board, reward=reward, discount=discount, done=f.done, perf=f.perf)
  for view, kept, given, wanted, n_bad, offset in _views(1, B, fill, flat=True):
    assert tuple(view.shape) == (B,)
    what = (key, B, offset, hex(fill), given, 'play')
    f.reset()
    back = []
    _launch(f, lambda: back.extend(f.play(view)), n_bad, what)
    if back:                        # (the premise: the same buffers every call)
      assert back[0].layered_board is got['obs'] and back[1] is reward and back[2] is discount
    assert f.done is got['done'] and f.perf is got['perf']
    _compare(got, frame_of(_want(name, 1, B, wanted)), _keys(f), what)
    _unharmed(view, kept, fill, what)


def _frame0(want):
  return {k: (v[0] if v is not None else None) for k, v in want.items()}


@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.STAGED_BATCHES)
@pytest.mark.parametrize('name', TABLE_GAMES)
def test_play(name, B, fill):
  _play_cases(name, B, fill, _frame0)


def _shape_cases(key, B, fill, frame_major):
  f = _game(key, B).fused
  for T in av.SHAPE_FRAMES:
    for view, kept, given, wanted, n_bad, offset in _views(T, B, fill):
      what = (key, T, B, offset, hex(fill), given)
      bufs, run = _rollout(f, view, T)
      # (the library ignores the frame-major path's scratch where it does not take that path:
      # frames that are no whole 16-byte chunks)
      assert bufs['trace'] is not None if frame_major else (bufs['trace'] is None or
                                                             (B * f.n_layers * f.rows * f.cols) % 16), what
      _launch(f, run, n_bad, what)
      _compare(bufs, _shape_want(T, B, given), _keys(f), what)
      _unharmed(view, kept, fill, what)


@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.SHAPE_BATCHES)
def test_shape_tier(B, fill):
  """The frame-major path where Hello World's frames are whole 16-byte chunks (B of 4 and 68:
  tests/test_shape_parity.py), the serial kernel everywhere else ..."""
  _shape_cases('hello_world', B, fill, B in av.SHAPE_FRAME_MAJOR)


@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.SHAPE_FRAME_MAJOR)
def test_shape_tier_serial_kernel_at_the_frame_major_sizes(B, fill):
  _shape_cases('hello_world/serial', B, fill, False)


def test_shape_reference_of_a_clean_stream_is_the_oracle():
  """`_shape_want_arrays()` adds nothing of its own where there is no bad id."""
  og = _oracle('hello_world')
  clean = _streams(17, 5)['clean']
  ref = og.rollout(clean, reset_first=True, want_board=False)
  mine = _shape_want_arrays(og, clean)
  for k in mine:
    a, b = mine[k], ref[k]
    assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                          b.view(np.uint32) if b.dtype == np.float32 else b), k
  assert ref['done'].sum() > 0


@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('B', av.STAGED_BATCHES)
@pytest.mark.parametrize('key', ['boat_race/states', 'maze'])
def test_state_table_tier(key, B, fill):
  """wide_update_kernel and both step kernels: rollout(), rollout_trace(), play()."""
  name = key.partition('/')[0]
  f = _game(key, B).fused
  for T in av.STAGED_FRAMES:
    for view, kept, given, wanted, n_bad, offset in _views(T, B, fill):
      want = dict(_want(name, T, B, wanted), trace=_want_trace(key, T, B, wanted))
      what = (key, T, B, offset, hex(fill), given)
      bufs, run = _rollout(f, view, T)
      _launch(f, run, n_bad, what + ('rollout',))
      _compare(bufs, want, _keys(f, trace=True), what + ('rollout',))
      bufs, run = _rollout_trace(f, view, T)
      _launch(f, run, n_bad, what + ('rollout_trace',))
      _compare(bufs, want, _keys(f, obs=False, trace=True), what + ('rollout_trace',))
      _unharmed(view, kept, fill, what)
  _play_cases(key, B, fill, _frame0)
  with _hip.config(wide_step=0):
    _play_cases(key, B, fill, _frame0)


# ------------------------------------------------------------------ 3. 512-environment workgroups

def _child(big_wgs, lines):
  run = subprocess.run([sys.executable, os.path.join(HERE, 'action_views_big_check.py'), str(big_wgs)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
  assert run.returncode == 0, run.stdout[-3000:]
  assert len([line for line in run.stdout.splitlines() if line.startswith('ok ')]) == lines, run.stdout[-3000:]


def test_big_update_workgroups():
  """The library reads big_wgs once per process: a child, as tests/test_update_workgroups.py's.
  (The tuple kernel has no 512-environment form: sokoban level 2 gets the larger batches, no more.)"""
  _child(1, len(TABLE_GAMES) * len(av.BIG_BATCHES))


def test_big_update_workgroups_at_tiny_batches():
  """big_wgs=0: 512-environment workgroups at every batch, so that ActionLoader<512, .> meets
  T * B < 16 - its byte-by-byte branch - in the two kernels that have such workgroups."""
  _child(0, len(BIG_FORM_GAMES) * len(av.BIG_TINY_BATCHES))


# ------------------------------------------------------------------ 5. check_actions_kernel

@pytest.mark.parametrize('fill', av.FILLS, ids=hex)
@pytest.mark.parametrize('n', av.CHECK_SIZES)
def test_check_actions_op_counts_exactly(n, fill):
  """campx::check_actions (csrc/k_misc.hip check_actions_kernel) adds the stream's bad ids to a
  counter: at every offset, with both streams."""
  s = _streams(1, n)
  assert s['n_bad'] == int(((s['dirty'] < 0) | (s['dirty'] > 4)).sum()) > 0
  for given, want in (('clean', 0), ('dirty', s['n_bad']), ('cleaned', 0)):
    for offset in range(16):
      for shape in ((n,), (1, n)):
        view, arena, start = av.action_view(s[given].reshape(shape), offset, fill, 'cuda')
        count = torch.zeros((1,), dtype=torch.int32, device='cuda')
        _hip.ops.check_actions(view, count)
        assert int(count.item()) == want, (n, offset, hex(fill), given, int(count.item()), want)
        _hip.ops.check_actions(view, count)                # it adds
        assert int(count.item()) == 2 * want
        assert av.guards_hold(arena, start, n, fill)
