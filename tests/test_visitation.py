"""`WideGame.state_visitation()` on the GPU (csrc/k_visit.hip, `campx::wide_visit`) against
tests/visitation_reference.py - a numpy restatement of the rule in include/campx_hip.h - bit for
bit: every comparison is `array_equal` of 'visits', 'finished', 'final', 'per_frame' and 'counts'.

Tables: the boat race's own (8 states); `wide_table_reference.make_table()` tables of one state and
of the plan's largest table in LDS and the next; a table of 70 001 states (274 workgroups, a last
wave of 49 lanes) and one of 5 003 states a third of whose entries end the episode, so that most of
the mass goes through state 0 at every frame.  The reference does not depend on the path: it is
computed once per (table, frames, restart, start) and every path is held against it.
"""

import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import visitation_reference as visit_ref
import wide_table_reference as ref

pytestmark = pytest.mark.gpu

LDS_MAX = 144 * 1024
UNIT = 1 << 38
FRAMES = [1, 7, 33]
KEYS = ('visits', 'finished', 'final', 'per_frame', 'counts')


def _plan(S, path=0):
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  code = _hip.lib.campx_wide_visit_plan(S, LDS_MAX, path, out)
  return code, list(out)


@functools.lru_cache(maxsize=None)
def _largest():
  lo, hi = 1, 1 << 14
  while lo < hi:                               # the largest S the plan puts in LDS
    mid = (lo + hi + 1) // 2
    lo, hi = (mid, hi) if _plan(mid)[1][0] == 1 else (lo, mid - 1)
  return lo


def big_table(S, done_share, seed):
  """A legal state table of S states with the attributes of a `tabulate.TracedGame` that the
  state-table tier reads (vectorised: `make_table()` is quadratic in S): one hidden thing on a 4 x 4
  board, state s reachable from state s - 1 by action 0, every other entry uniform over the table,
  `done_share` of those ending the episode."""
  rng = np.random.RandomState(seed)
  g = types.SimpleNamespace()
  g.rows, g.cols, g.n_states = 4, 4, S
  g.chars = [' ', '#']
  g.any_reward, g.has_perf = True, False
  board = np.full((4, 4), ord(' '), np.uint8)
  board[0, :] = ord('#')
  g.variants, g.backdrop = [board], board
  g.model_board = lambda cells, movers=True, variant=0: board.copy()
  g.mode_orders = g.variant_masks = None
  g.statics, g.pieces_as_mask = (), True
  g.movers, g.piece_cell, g.z_order = ['#'], [None], list(g.chars)
  g.st_variant = np.zeros(S, np.uint16)
  g.st_cells = rng.randint(0, 16, size=(S, 1)).astype(np.uint16)
  g.st_shows = np.zeros((S, 1), np.uint8)
  g.st_present = np.ones((S, 1), bool)
  g.init_cells = (int(g.st_cells[0, 0]),)
  nxt = rng.randint(0, S, size=S * 5)
  children = np.arange(1, S)
  nxt[5 * (children - 1)] = children
  tree = np.zeros(S * 5, bool)
  tree[5 * (children - 1)] = True
  g.st_next = nxt.reshape(S, 5).astype(np.int32)
  g.st_done = ((rng.rand(S * 5) < done_share) & ~tree).reshape(S, 5).astype(np.uint8)
  g.st_reward = rng.choice(np.array([np.nan, 0.0, 1.0, -1.0], np.float32), size=(S, 5))
  g.discount_list = [1.0] * 16
  g.st_dcode = np.zeros((S, 5), np.uint8)
  g.st_discount = np.where(g.st_done != 0, np.float32(0), np.float32(1)).astype(np.float32)
  g.st_perf = np.zeros((S, 5), np.int8)
  g.st_reached = np.ones((S, 5), bool)
  g.done_bytes = lambda: (g.st_done | (g.st_dcode << 4)).astype(np.uint8)
  return g


@functools.lru_cache(maxsize=None)
def _table(name):
  if name == 'one':
    return ref.make_table(8101, 4, 4, 2, 1, 1)
  if name == 'fits':
    return ref.make_table(8102, 4, 4, 2, 1, _largest())
  if name == 'next':
    return ref.make_table(8103, 4, 4, 2, 1, _largest() + 1)
  if name == 'large':
    return big_table(70001, 0.1, 1)
  if name == 'hot':
    return big_table(5003, 1.0 / 3, 2)
  raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _game(name):
  from campx_amd import wide
  g = _table(name)
  f = wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), 1, 'cuda', g)
  assert f.n_states == g.n_states
  return f


@functools.lru_cache(maxsize=None)
def _boat():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.use_state_table()
  game.its_showtime()
  return game


def _weights(S, seed, bad=0):
  rng = np.random.RandomState(seed)
  w = rng.uniform(0.25, 2.0, size=(S, 5)).astype(np.float32)
  w[rng.rand(S, 5) < 0.2] = 0
  w[np.arange(S), rng.randint(0, 5, size=S)] = 1.25            # (no row is all zero)
  rows = rng.choice(S, size=min(S, bad), replace=False)
  for i, row in enumerate(rows):
    w[row, rng.randint(5)] = (-1.0, np.nan, np.inf)[i % 3]
  return w


def _start(S, kind, seed):
  """-> (the `start` argument as numpy or None, the reference's int64 start or None)"""
  if kind == 'none':
    return None, None
  rng = np.random.RandomState(seed)
  p = rng.rand(S) * (rng.rand(S) < 0.5)
  p[rng.randint(S)] += 1.0
  p /= p.sum()
  if kind == 'float':
    p = p.astype(np.float32)
    return p, visit_ref.quantise(p)
  d = np.floor(p * (UNIT // 2)).astype(np.int64)                # int64: half an environment
  return d, d


def _paths(S):
  return ([1] if _plan(S, path=1)[0] == 0 else []) + [2, 0]


def _eq(res, want, what, keys=KEYS):
  for k in keys:
    got = res[k].cpu().numpy()
    assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.dtype, got.shape)
    assert np.array_equal(got, want[k]), (what, k, int((got != want[k]).sum()))


def _run_matrix(f, nxt, done, cases, seed):
  S = f.n_states
  w = _weights(S, seed)
  policy = torch.from_numpy(w).cuda()
  for frames, restart, kind in cases:
    given, start = _start(S, kind, seed + frames)
    want = visit_ref.visitation(nxt, done, w, frames, start=start, restart=restart)
    assert want['bad_rows'] == 0
    for path in _paths(S):
      arg = None if given is None else torch.from_numpy(given).cuda()
      res = f.state_visitation(policy, frames, start=arg, restart=restart, want_frames=True, path=path)
      _eq(res, want, (S, frames, restart, kind, path))
      assert res['unit'] == UNIT and res['probs'].dtype == torch.float64
      assert np.array_equal(res['probs'].cpu().numpy(), want['counts'] / float(1 << 24))
      if path == 2:                                # and without per_frame: other buffers, same bits
        res = f.state_visitation(policy, frames, start=arg, restart=restart, path=path)
        assert 'per_frame' not in res
        _eq(res, want, (S, frames, restart, kind, path, 'no per_frame'), KEYS[:3] + KEYS[4:])
  f.check_actions()


FULL = [(n, restart, kind) for n in FRAMES for restart in (True, False) for kind in ('none', 'int64', 'float')]
# the large tables: every frames, restart and start value, each path, not their whole product
SOME = [(7, True, 'none'), (33, False, 'int64'), (1, True, 'float'), (33, True, 'float')]


def test_the_plan_is_the_one_the_sizes_were_chosen_for():
  from campx_amd import _hip
  assert _hip.config_get('wide_lds_max') == LDS_MAX and _largest() == 2834
  assert _paths(_largest()) == [1, 2, 0] and _paths(_largest() + 1) == [2, 0]
  assert _plan(70001, path=2)[1] == [2, 0, 256, 274] and 70001 % 64 == 49


def test_the_boat_race_s_own_table():
  game = _boat()
  traced = game.fused.traced
  assert game.fused.n_states == 8
  _run_matrix(game.fused, traced.st_next, traced.st_done, FULL, 21)
  # through the Engine
  w = torch.from_numpy(_weights(8, 22)).cuda()
  res = game.state_visitation(w, 7, want_frames=True)
  want = visit_ref.visitation(traced.st_next, traced.st_done, w.cpu().numpy(), 7)
  _eq(res, want, 'engine')
  out = game.visitation_buffers(7, want_frames=True)
  assert game.state_visitation(w, 7, want_frames=True, out=out)['visits'] is out['visits']
  _eq(out, want, 'engine out=')


@pytest.mark.parametrize('name,cases', [('one', FULL), ('fits', FULL), ('next', FULL), ('large', SOME),
                                        ('hot', SOME)])
def test_every_path_equals_the_reference(name, cases):
  g = _table(name)
  _run_matrix(_game(name), g.st_next, g.st_done, cases, 30 + len(name))
  if name == 'hot':
    w = _weights(g.n_states, 30 + len(name))
    want = visit_ref.visitation(g.st_next, g.st_done, w, 7)
    assert want['finished'][2:].min() > UNIT // 10         # the hot spot is one: state 0 refills
    assert want['per_frame'][3:, 0].min() > UNIT // 10


def test_path_1_on_a_table_that_does_not_fit_raises():
  f = _game('next')
  policy = torch.from_numpy(_weights(f.n_states, 1)).cuda()
  with pytest.raises(ValueError, match='path=1'):
    f.state_visitation(policy, 3, path=1)
  f.state_visitation(policy, 3, path=2)
  f.check_actions()


@pytest.mark.parametrize('name', ['fits', 'next'])
def test_continuation_and_reused_buffers_on_the_device(name):
  g, f = _table(name), _game(name)
  S = g.n_states
  w = _weights(S, 41)
  policy = torch.from_numpy(w).cuda()
  for restart in (True, False):
    whole = visit_ref.visitation(g.st_next, g.st_done, w, 12, restart=restart)
    for path in _paths(S)[:2]:
      first = f.state_visitation(policy, 5, restart=restart, path=path)
      keep = first['final'].clone()
      rest = f.state_visitation(policy, 7, start=first['final'], restart=restart, path=path)
      assert torch.equal(first['final'], keep)                    # the start given is left as it is
      assert np.array_equal(rest['final'].cpu().numpy(), whole['final'])
      assert np.array_equal((first['visits'] + rest['visits']).cpu().numpy(), whole['visits'])
      assert np.array_equal(torch.cat([first['finished'], rest['finished']]).cpu().numpy(), whole['finished'])
      # out= reused across two calls, the second starting from the first's 'final' IN PLACE:
      # 5 frames (odd) and 6 frames (even) - either buffer of the global path is read first
      out = f.visitation_buffers(5, want_frames=True)
      for t in out.values():
        t.fill_(-7)
      a = f.state_visitation(policy, 5, restart=restart, want_frames=True, out=out, path=path)
      assert a['final'] is out['final'] and a['per_frame'] is out['per_frame']
      _eq(a, visit_ref.visitation(g.st_next, g.st_done, w, 5, restart=restart), (name, path, 'out='))
      b = f.state_visitation(policy, 5, start=out['final'], restart=restart, want_frames=True, out=out, path=path)
      want = visit_ref.visitation(g.st_next, g.st_done, w, 5, start=whole['per_frame'][5], restart=restart)
      _eq(b, want, (name, path, 'in place, odd'))
      assert np.array_equal(b['final'].cpu().numpy(), whole['per_frame'][10])
      out6 = dict(f.visitation_buffers(6), final=out['final'])
      c = f.state_visitation(policy, 6, start=out['final'], restart=restart, out=out6, path=path)
      want = visit_ref.visitation(g.st_next, g.st_done, w, 6, start=whole['per_frame'][10], restart=restart)
      _eq(c, want, (name, path, 'in place, even'), KEYS[:3] + KEYS[4:])
  f.check_actions()


@pytest.mark.parametrize('name', ['fits', 'next'])
def test_bad_rows_give_the_reference_s_bits_and_raise_lazily_with_their_count(name):
  g, f = _table(name), _game(name)
  w = _weights(g.n_states, 51, bad=5)
  w[0] = [1, 1, -1, 1, 1]                                        # (the reset state's row too)
  want = visit_ref.visitation(g.st_next, g.st_done, w, 7)
  n_bad = want['bad_rows']
  assert n_bad in (5, 6)
  policy = torch.from_numpy(w).cuda()
  message = '^{} rows of the policy given to state_visitation'.format(n_bad)
  for path in _paths(g.n_states)[:2]:
    out = f.visitation_buffers(7, want_frames=True)
    # the call does not wait for the count: it raises only if the flag is already up when it looks
    try:
      f.state_visitation(policy, 7, want_frames=True, out=out, path=path)
    except ValueError as e:
      assert str(e).startswith(message[1:])
    else:
      with pytest.raises(ValueError, match=message):
        f.check_actions()
    _eq(out, want, (name, path, 'bad rows'))
    f.check_actions()
    f.validate_actions = 'sync'
    try:
      with pytest.raises(ValueError, match=message):
        f.state_visitation(policy, 7, path=path)
    finally:
      f.validate_actions = True
    f.check_actions()


def test_a_game_that_is_not_on_the_tier_refuses():
  from campx_amd.games import boat_race
  game = boat_race.build(batch=8, device='cuda')
  game.its_showtime()
  for call in (lambda: game.state_visitation(torch.ones(8, 5, device='cuda'), 3),
               lambda: game.visitation_buffers(3)):
    with pytest.raises(NotImplementedError, match='state-table tier only'):
      call()
  with pytest.raises(RuntimeError, match='its_showtime'):
    boat_race.build(batch=8, device='cuda').state_visitation(torch.ones(8, 5, device='cuda'), 3)


def test_argument_errors_raise_before_any_launch():
  f = _game('fits')
  S = f.n_states
  policy = torch.from_numpy(_weights(S, 61)).cuda()
  out = f.visitation_buffers(3, want_frames=True)
  for t in out.values():
    t.fill_(7)
  launched = []
  from campx_amd import _hip
  real = _hip.ops.wide_visit

  class Spy(object):
    def __call__(self, *a):
      launched.append(a)
      return real(*a)

  ones = torch.ones(S, device='cuda')
  bad_calls = [
      lambda: f.state_visitation(policy.double(), 3, out=out),
      lambda: f.state_visitation(policy[:-1], 3, out=out),
      lambda: f.state_visitation(policy.cpu(), 3, out=out),
      lambda: f.state_visitation(policy, 0, out=out),
      lambda: f.state_visitation(policy, 3.0, out=out),
      lambda: f.state_visitation(policy, (1 << 20) + 1),
      lambda: f.state_visitation(policy, 3, path=3, out=out),
      lambda: f.state_visitation(policy, 3, start=ones.long()[:-1], out=out),
      lambda: f.state_visitation(policy, 3, start=ones.long().cpu(), out=out),
      lambda: f.state_visitation(policy, 3, start=ones.int(), out=out),
      lambda: f.state_visitation(policy, 3, start=-ones.long(), out=out),
      lambda: f.state_visitation(policy, 3, start=ones.long() * (UNIT // S + 1), out=out),     # total > 2^38
      lambda: f.state_visitation(policy, 3, start=ones, out=out),                               # sums to S
      lambda: f.state_visitation(policy, 3, start=ones * float('nan'), out=out),
      lambda: f.state_visitation(policy, 3, start=torch.cat([-ones[:1], ones[:1] * 2, ones[2:] * 0]), out=out),
      lambda: f.state_visitation(policy, 3, start=out['scratch'], out=out, path=2),
      lambda: f.state_visitation(policy, 3, out={'visits': out['visits']}),
      lambda: f.state_visitation(policy, 4, out=out),                                           # finished of 3
      lambda: f.state_visitation(policy, 3, out=dict(out, counts=out['counts'].long())),
      lambda: f.state_visitation(policy, 3, want_frames=True, out=f.visitation_buffers(3)),
      lambda: f.state_visitation(policy, 3, out=[out]),
  ]
  try:
    _hip.ops.wide_visit = Spy()
    for k, call in enumerate(bad_calls):
      with pytest.raises(ValueError):
        call()
      assert not launched, k
  finally:
    del _hip.ops.wide_visit
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in out.values())                       # nothing was written
  f.state_visitation(policy, 3, want_frames=True, out=out)                     # and the dict was fine


def test_the_c_entry_through_ctypes_with_no_per_frame():
  from campx_amd import _hip
  g, f = _table('next'), _game('next')
  S = g.n_states
  w = _weights(S, 71)
  want = visit_ref.visitation(g.st_next, g.st_done, w, 7, restart=False)
  policy = torch.from_numpy(w).cuda()
  out = f.visitation_buffers(7)
  for t in out.values():
    t.fill_(-3)
  spec = (ctypes.c_char * f._spec_host.numel()).from_buffer(f._spec_host.numpy())
  vp = ctypes.c_void_p
  stream = torch.cuda.current_stream().cuda_stream
  for path in (2, 0):
    code = _hip.lib.campx_wide_visit_launch(
        ctypes.cast(spec, _hip.lib.campx_wide_visit_launch.argtypes[0]), vp(f._tables.data_ptr()),
        vp(policy.data_ptr()), None, 0, 7, vp(out['visits'].data_ptr()), vp(out['finished'].data_ptr()),
        vp(out['final'].data_ptr()), None, vp(out['counts'].data_ptr()), vp(out['scratch'].data_ptr()),
        None, None, path, vp(stream))
    assert code == 0
    torch.cuda.synchronize()
    _eq(out, want, ('ctypes', path), KEYS[:3] + KEYS[4:])
    assert not out['scratch'].any()                            # left all zero
