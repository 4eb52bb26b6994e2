"""The state-table tier on SYNTHETIC tables against tests/wide_table_reference.py - a numpy model
of `CampxWideSpec` written from include/campx_hip.h - bit for bit, no tolerances.

The real games pin the kernels of this tier (k_wide.hip, k_policy.hip, k_states.hip, the gather
launch) to a few points; `wide_table_reference.make_table()` generates legal tables directly, so
the cases below walk the branches the kernels specialise on: every plane count 1..8 with and
without a variant or mask plane (V = 2 / 256, P = 1 / 16), discount codes, hidden performance,
no reward stream, tables of one state, tables either side of the LDS bound, the smallest and the
largest board, rows that are no multiple of 16 bytes, both row paddings.  A table goes through the
production constructor (`WideGame.__init__`, `tabulate.to_wide_spec()`,
`campx_wide_tables_build()`) and every torch op unchanged.

CPU tests: every table validates; the model agrees with `TracedGame.model_board()` and the
committed goldens on real games (a wrong oracle must not pass a wrong kernel); the reference walks
meet what the cases claim; every kernel instantiation is reached by some case (`paths()` restates
the launch code's conditions).
"""

import collections
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest

import policy_reference as pref
import wide_table_reference as ref

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BOARDS = [(4, 4, 2), (5, 5, 7), (3, 7, 3), (15, 17, 6), (1, 127, 2), (32, 32, 16)]
BATCHES = [1, 63, 65, 257, 1000]
ROLLOUTS = ((1, True), (7, False), (9, True), (20, False))       # (T, reset_first), in a row
POLICY_ROLLOUTS = ((1, True), (7, False), (8, False), (9, True), (20, False))
SEED = 0x1234567890abcdef
# seeds are 1000 + index (2000 + index for the extras) unless the reference walk of that seed misses
# what test_the_reference_walk_meets_what_the_case_claims asks for
SEEDS = {10: 3010}

Case = collections.namedtuple(
    'Case', 'seed rows cols L K S V P dcodes perf reward B padded lds0 sixteen')


def _lds_want(S, perf, thresholds):
  """The size rule of campx_wide_update_launch / (`thresholds`) campx_wide_policy_update_launch."""
  entries = (S * 5 * 8 + 15) // 16 * 16
  if thresholds:
    return entries + S * 16 + ((S * 5 + 15) // 16 * 16 if perf else 0) + S * 5 * 4
  return entries + S * 16 + (S * 5 if perf else 0)


@functools.lru_cache(maxsize=None)
def _lds_bound():
  from campx_amd import _hip
  return _hip.config_get('wide_lds_max')


def _largest_in_lds(perf, thresholds):
  S = 1
  while _lds_want(S + 1, perf, thresholds) <= _lds_bound():
    S += 1
  return S


def _cases():
  combos = [(K, 1, 0) for K in range(1, 9)]
  for K in range(1, 8):
    combos += [(K, 2, 0), (K, 256, 0), (K, 1, 1), (K, 1, 16)]
  sizes = [37, 2, 300, 64, 411, 5]
  cases = []
  for i, (K, V, P) in enumerate(combos):
    rows, cols, L = BOARDS[i % 6]
    B = BATCHES[i % 5]
    if rows * cols * L > 4096 and B > 257:
      B = 257
    S = sizes[(i // 2) % 6]
    cases.append(Case(SEEDS.get(i, 1000 + i), rows, cols, L, K, S, V, P, dcodes=i % 3 == 1 and S >= 4,
                      perf=i % 4 in (1, 2), reward=i not in (5, 20, 27), B=B, padded=i % 2 == 0,
                      lds0=i % 7 == 3, sixteen=i % 4 == 0))
  n = len(cases)
  extra = [
      # one state: every LDS offset of the policy kernel degenerates
      dict(K=1, S=1), dict(K=8, S=1, perf=True, B=65), dict(K=4, S=1, B=257, lds0=True, board=1),
      dict(K=2, S=1, reward=False, B=1000, board=2),
      # the general chunk with many planes: discount codes, perf, in LDS and not
      dict(K=3, S=37, dcodes=True, B=65, board=1), dict(K=5, S=64, dcodes=True, perf=True, B=257, board=2),
      dict(K=8, S=300, dcodes=True, perf=True, B=63, lds0=True, board=3),
      dict(K=7, V=256, S=411, dcodes=True, B=65, lds0=True, board=0),
      dict(K=7, P=16, S=300, dcodes=True, perf=True, B=1000, board=4),
      dict(K=6, S=37, reward=False, perf=True, B=257, lds0=True, board=1),
      # plain chunks read through the caches, with and without perf
      dict(K=3, S=64, B=257, lds0=True, board=2), dict(K=5, S=37, perf=True, B=65, lds0=True, board=0),
      dict(K=6, V=2, S=64, perf=True, B=1000, lds0=True, board=1), dict(K=8, S=37, B=1000, lds0=True, board=0),
      dict(K=4, P=16, S=300, B=63, lds0=True, board=3), dict(K=2, S=5, perf=True, B=1, lds0=True, board=5),
      # the largest board with everything on it
      dict(K=7, V=256, S=300, B=63, board=5, sixteen=True), dict(K=7, P=16, S=64, perf=True, B=65, board=5, sixteen=True),
      dict(K=8, S=37, dcodes=True, B=257, board=5),
      # the smallest with everything on it
      dict(K=7, P=16, S=37, B=1000, board=0, sixteen=True), dict(K=7, V=256, S=300, perf=True, B=257, board=0, sixteen=True),
  ]
  # either side of the LDS bound: the policy kernel's size rule (thresholds counted in) ...
  for perf in (False, True):
    S = _largest_in_lds(perf, True)
    extra += [dict(K=2 if perf else 1, S=S, perf=perf, B=65, board=0, P=3 if perf else 0),
              dict(K=2 if perf else 1, S=S + 1, perf=perf, B=65, board=0, P=3 if perf else 0)]
  # ... and the update kernel's
  S = _largest_in_lds(True, False)
  extra += [dict(K=3, S=S, perf=True, B=63, board=2, V=2), dict(K=3, S=S + 1, perf=True, B=63, board=2, V=2)]
  for j, e in enumerate(extra):
    rows, cols, L = BOARDS[e.pop('board', j % 6)]
    d = dict(seed=2000 + j, rows=rows, cols=cols, L=L, K=1, S=37, V=1, P=0, dcodes=False, perf=False,
             reward=True, B=BATCHES[j % 5], padded=j % 2 == 1, lds0=False, sixteen=False)
    d.update(e)
    if d['rows'] * d['cols'] * d['L'] > 4096 and d['B'] > 257:
      d['B'] = 257
    cases.append(Case(**d))
  assert len(cases) == n + len(extra)
  return cases


def _id(c):
  return 'K{}-V{}-P{}-{}x{}x{}-S{}-B{}{}{}{}{}{}'.format(
      c.K, c.V, c.P, c.rows, c.cols, c.L, c.S, c.B, '-dc' if c.dcodes else '', '-pf' if c.perf else '',
      '' if c.reward else '-nr', '-pad' if c.padded else '', '-lds0' if c.lds0 else '')


CASES = _cases()
IDS = [_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


@functools.lru_cache(maxsize=None)
def _table(c):
  return ref.make_table(c.seed, c.rows, c.cols, c.L, c.K, c.S, V=c.V, P=c.P, dcodes=c.dcodes,
                        perf=c.perf, any_reward=c.reward)


def _actions(c, salt, T, bad=False):
  """Random action ids int8 [T, B]; `bad`: ids 5, -1 and 127 in every fifth environment."""
  rng = np.random.RandomState(c.seed * 16 + salt)
  a = rng.randint(0, 5, size=(T, c.B)).astype(np.int8)
  if bad:
    for t in range(T):
      a[t, (t % 5)::5] = (5, -1, 127)[t % 3]
  return a


def _policy(c):
  """test_policy_rollout._policy's style: exact zeros in every fourth row, rows scaled by 1e-3 and
  1e3 in turn."""
  rng = np.random.RandomState(c.seed + 77)
  w = rng.uniform(0.05, 1.0, size=(c.S, 5)).astype(np.float32)
  for s in range(0, c.S, 4):
    w[s, rng.choice(5, size=rng.randint(1, 5), replace=False)] = 0.0
  w[1::3] *= np.float32(1e-3)
  w[2::3] *= np.float32(1e3)
  return w


def paths(c):
  """The kernel instantiations a case reaches, from the launch code's own conditions
  (campx_wide_policy_update_launch, campx_wide_update_launch and the kernels' choice of chunk)."""
  planes = c.K + (1 if c.V > 1 or c.P > 0 else 0)
  out = set()
  bound = 0 if c.lds0 else _lds_bound()
  lds = _lds_want(c.S, c.perf, True) <= bound
  for states in (True, False):
    out.add('policy<{},{},{}>'.format(*('true' if x else 'false' for x in (lds, c.perf, states))))
  plain = not c.dcodes and c.reward
  # policy calls of T = 8 at frame 8 and T = 20 at frame 25 hold whole chunks; T = 1, 7, 9 do not
  out.add('policy plain K={}'.format(planes) if plain else 'policy general K={}'.format(planes))
  out.add('policy general K={}'.format(planes))
  lds = _lds_want(c.S, c.perf, False) <= bound
  out.add('update<{},{}>'.format('true' if lds else 'false', 'true' if c.perf else 'false'))
  out.add('update plain K={}'.format(planes) if plain else 'update general K={}'.format(planes))
  out.add('update general K={}'.format(planes))
  return out


# ------------------------------------------------------------------------------------- CPU

def test_the_case_list_covers_what_it_says():
  assert 60 <= len(CASES) <= 120
  combos = {(c.K, c.V, c.P) for c in CASES}
  for K in range(1, 9):
    assert (K, 1, 0) in combos
  for K in range(1, 8):
    assert {(K, 2, 0), (K, 256, 0), (K, 1, 1), (K, 1, 16)} <= combos
  assert {(c.rows, c.cols, c.L) for c in CASES} == set(BOARDS)
  assert {1, 2, 37} <= {c.S for c in CASES}
  for perf in (False, True):
    S = _largest_in_lds(perf, True)
    assert _lds_want(S, perf, True) <= _lds_bound() < _lds_want(S + 1, perf, True)
    assert {S, S + 1} <= {c.S for c in CASES if c.perf == perf and not c.lds0}
  assert {(c.B, c.padded) for c in CASES} >= {(B, p) for B in BATCHES for p in (True, False)}
  assert sum(not c.reward for c in CASES) >= 2
  for flag in ('dcodes', 'perf'):
    assert {getattr(c, flag) for c in CASES} == {True, False}
  # the largest and the smallest board with all mask bits / the top of the variant plane
  for board in (BOARDS[0], BOARDS[5]):
    assert {(7, 256, 0), (7, 1, 16)} <= {(c.K, c.V, c.P) for c in CASES if (c.rows, c.cols, c.L) == board}


def test_every_kernel_instantiation_is_reached_by_some_case():
  reached = collections.defaultdict(list)
  for c, name in zip(CASES, IDS):
    for p in paths(c):
      reached[p].append(name)
  rows = ['policy<{},{},{}>'.format(a, b, s) for a in ('true', 'false') for b in ('true', 'false')
          for s in ('true', 'false')]
  rows += ['update<{},{}>'.format(a, b) for a in ('true', 'false') for b in ('true', 'false')]
  for K in range(1, 9):
    rows += ['policy plain K={}'.format(K), 'policy general K={}'.format(K),
             'update plain K={}'.format(K), 'update general K={}'.format(K)]
  for row in rows:
    assert reached[row], row
  # the general chunk with discount codes at more than two planes, in LDS and not, with perf and not
  hard = [c for c in CASES if c.dcodes and c.K + (c.V > 1 or c.P > 0) > 2]
  assert {(c.lds0, c.perf) for c in hard} >= {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_the_table_is_a_legal_spec(c):
  from campx_amd import _hip, tabulate
  g = _table(c)
  spec, arrays = tabulate.to_wide_spec(g)
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0
  assert (spec.rows, spec.cols, spec.n_layers, spec.n_dyn, spec.n_states) == (c.rows, c.cols, c.L, c.K, c.S)
  assert spec.n_variants == (c.V if c.V > 1 else 0) and spec.n_pieces == c.P
  assert (spec.any_dcode, spec.has_perf, spec.any_reward) == (int(c.dcodes), int(c.perf), int(c.reward))
  w = ref.view(g)
  assert (w.K, w.P, w.V, w.S) == (c.K, c.P, c.V, c.S)
  # what the generator promises
  S = c.S
  seen, queue = {0}, [0]
  while queue:
    s = queue.pop()
    for a in range(5):
      n = int(g.st_next[s, a])
      if not g.st_done[s, a] and n not in seen:
        seen.add(n)
        queue.append(n)
  assert len(seen) == S                          # reachable without passing an episode's end
  assert g.st_done.sum() >= 1
  top = w.tops[w.variant]
  for d in range(c.K):
    on = w.shows[:, d]
    assert (top[np.arange(S), w.cells[:, d]][on] != w.thing_layer[d]).all()
    for p in range(c.P):
      assert not (on & (((w.mask >> p) & 1) != 0) & (w.cells[:, d] == w.piece_cell[p])).any()
    for e in range(d):
      assert not (on & w.shows[:, e] & (w.cells[:, d] == w.cells[:, e])).any()
  if c.V > 1:
    assert {0, c.V - 1} <= set(w.variant.tolist())
    assert np.array_equal(arrays['variant_top_layer'], w.tops.astype(np.uint8))
  if c.P:
    assert {0, (1 << c.P) - 1} <= set(w.mask.tolist()) and len(set(w.piece_cell.tolist())) == c.P
    assert np.array_equal(arrays['state_pieces'], w.mask.astype(np.uint16))
  if c.dcodes:
    assert set(range(1, 16)) <= set(g.st_dcode.reshape(-1).tolist())
    assert len(set(g.discount_list[1:])) == 15
  if c.perf:
    assert {-128, 127} <= set(g.st_perf.reshape(-1).tolist())


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_the_reference_walk_meets_what_the_case_claims(c):
  """In the model's walk alone: the 20-frame rollout has an episode's end and a frame that follows
  one in the same column; a case with discount codes meets at least three of them."""
  g = _table(c)
  walker = ref.Walker(g, c.B)
  codes = set()
  for i, (T, reset) in enumerate(ROLLOUTS):
    acts = _actions(c, 10 + i, T)
    starts = np.where(walker.over | reset, 0, walker.state)
    want = walker.rollout(acts, reset_first=reset)
    froms = np.concatenate([starts[None], np.where(want['done'][:-1] != 0, 0, want['states'][:-1])])
    codes |= set(g.st_dcode[froms, acts.astype(np.int64)].reshape(-1).tolist())
    if T >= 20:
      assert want['done'].any() and want['done'][:-1].any()
  if c.dcodes:
    assert len(codes - {0}) >= 3, codes


def _golden_frames(name):
  with np.load(os.path.join(GOLDEN_DIR, name)) as f:
    return {k: f[k] for k in f.files}


def _real_games():
  """(name, builder of the game on the generic tier, golden or None) of the real games the model
  is pinned on."""
  import random_pickups
  import test_wide_parity
  from campx_amd.games import maze
  defs = random_pickups.definitions()
  pick = {k[3:]: v for k, v in _golden_frames('random_pickups.npz').items() if k.startswith('k3_')}
  tide = {k[4:]: v for k, v in _golden_frames('random_pickups.npz').items() if k.startswith('k12_')}
  return [('maze', lambda: maze.build(16, 16), _golden_frames('maze_16x16.npz')),
          ('pickups', random_pickups.builder(defs[3]), pick),
          ('variants', random_pickups.builder(defs[12]), tide),
          ('six things', test_wide_parity._coin_field, None)]


@pytest.mark.parametrize('which', range(4), ids=['maze', 'pickups', 'variants', 'six-things'])
def test_the_model_is_pinned_on_real_games(which):
  """`render()` and `trace()` fed from a real `TracedGame`: every state's board is
  `TracedGame.model_board()`'s and the board the game's own classes rendered when it was tabulated;
  walked along the golden's actions, the frames are the golden's (maze, pickups, variants: frames
  of the reference engine), or - the six-things game has no golden - the game's own classes'."""
  from campx_amd import tabulate
  name, build, gold = _real_games()[which]
  traced = tabulate.trace(build())
  spec, arrays = tabulate.to_wide_spec(traced)
  w = ref.view(traced)
  S = traced.n_states
  assert (w.K, w.P, w.V if w.V > 1 else 0) == (spec.n_dyn, spec.n_pieces, spec.n_variants)
  if name == 'pickups':
    assert w.P == 7
  if name == 'variants':
    assert w.V > 1
  if name == 'six things':
    assert w.K == 6
  obs, board = ref.render(traced, np.arange(S))
  for s in range(S):
    cells = tuple(traced.st_cells[s]) + ((traced.st_mode[s],) if len(traced.mode_orders) > 1 else ())
    want = traced.model_board(cells, variant=int(traced.st_variant[s]))
    assert np.array_equal(board[s].astype(np.uint8), want), s
  assert np.array_equal(board.astype(np.uint8).reshape(S, -1), traced.st_board)
  assert np.array_equal(obs, np.stack([board == np.int8(ord(ch)) for ch in traced.chars], 1).astype(np.int8))
  # the trace against the arrays the production side hands to the table builder
  tr = ref.trace(traced, np.arange(S))
  assert np.array_equal(tr[:w.K] & 0x3ff, (arrays['state_cells'] & 0x3ff).T)
  assert np.array_equal(tr[:w.K] >> 15, 1 - (arrays['state_cells'] >> 15).T)
  # ... bits 10-14: the layer of the scenery of the state's variant, without the movers, at the cell
  layer_of = {ord(ch): i for i, ch in enumerate(traced.chars)}
  bare = [traced.model_board(traced.init_cells, movers=False, variant=v).reshape(-1) for v in range(w.V)]
  for s in range(S):
    under = bare[int(traced.st_variant[s]) if w.V > 1 else 0]
    assert [(int(e) >> 10) & 31 for e in tr[:w.K, s]] == [layer_of[int(under[int(e) & 0x3ff])] for e in tr[:w.K, s]], s
  if w.P:
    assert np.array_equal(tr[w.K], arrays['state_pieces'])
  if w.V > 1:
    assert np.array_equal(tr[w.K], arrays['state_variant'])
  if gold is not None:
    acts = gold['actions']
    T, N = acts.shape
    walker = ref.Walker(traced, N)
    first = ref.render(traced, np.zeros(N, np.int64))
    assert np.array_equal(first[1], gold['board'][0].astype(np.int8))
    assert np.array_equal(first[0], gold['layered'][0].astype(np.int8))
    want = walker.rollout(acts, reset_first=True)
    obs, board = ref.render(traced, want['states'].reshape(-1))
    assert np.array_equal(board.reshape(gold['board'][1:].shape), gold['board'][1:].astype(np.int8))
    assert np.array_equal(obs.reshape(gold['layered'][1:].shape), gold['layered'][1:].astype(np.int8))
    for k in ('reward', 'discount'):
      assert np.array_equal(want[k].view(np.uint32), gold[k].astype(np.float32).view(np.uint32)), k
    assert np.array_equal(want['done'], gold['done'])
  else:
    acts = np.resize([1] * 6 + [3] * 2 + [0] * 6 + [2] * 2, 40).astype(np.int8)[:, None]
    walker = ref.Walker(traced, 1)
    want = walker.rollout(acts, reset_first=True)
    onehot = tabulate.default_actions()
    game = build()
    game.its_showtime()
    for t in range(len(acts)):
      if game.game_over:
        game = build()
        game.its_showtime()
      seen, reward, discount = game.play(onehot[int(acts[t, 0])])
      obs, board = ref.render(traced, want['states'][t])
      assert np.array_equal(board[0].astype(np.uint8), seen.board.numpy()), t
      assert np.array_equal(obs[0], seen.layered_board.numpy().astype(np.int8)), t
      assert np.float32(discount) == want['discount'][t, 0] and int(game.game_over) == want['done'][t, 0]
    assert want['done'].sum() >= 1


# ------------------------------------------------------------------------------------- GPU

def _bits(x):
  """A tensor's bits as a numpy array (16-bit floats as int16, float32 as uint32)."""
  import torch
  if x.dtype in (torch.float16, torch.bfloat16):
    return x.contiguous().view(torch.int16).cpu().numpy()
  a = x.cpu().numpy()
  return a.view(np.uint32) if a.dtype == np.float32 else a


def _eq(got, want, what):
  got = _bits(got)
  want = np.asarray(want)
  if want.dtype == np.float32:
    want = want.view(np.uint32)
  if got.dtype == np.int16 and want.dtype == np.uint16:
    got = got.view(np.uint16)
  assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  assert np.array_equal(got, want), what


def _sixteen(obs, dtype):
  import torch
  return ref.as_bits16(obs, ref.F16_ONE if dtype == torch.float16 else ref.BF16_ONE)


def _want_obs(obs, dtype):
  import torch
  return obs if dtype == torch.int8 else _sixteen(obs, dtype)


class _BadIds(object):
  """Bad action ids raise lazily, from whichever call sees the flag first: count them all."""

  def __init__(self):
    self.count = 0

  def call(self, fn, *args, **kwargs):
    try:
      return fn(*args, **kwargs)
    except ValueError as e:
      m = re.match(r'(\d+) action ids are outside 0\.\.4', str(e))
      assert m, str(e)
      self.count += int(m.group(1))
      return None


def _game(c):
  from campx_amd import wide
  g = _table(c)
  f = wide.WideGame(types.SimpleNamespace(rows=c.rows, cols=c.cols), c.B, 'cuda', g)
  assert f.n_states == c.S and f._n_planes == ref.view(g).planes
  assert f.any_reward == c.reward and f.has_perf == c.perf
  return g, f


def _scalars(c, out, want, what):
  for k in ('reward', 'discount', 'done', 'perf'):
    if out.get(k) is None:
      assert k in ('reward', 'perf') and not (c.reward if k == 'reward' else c.perf), (what, k)
    else:
      _eq(out[k], want[k], (what, k))


def _state(f, walker, what):
  _eq(f.state, walker.state.astype(np.int32), (what, 'state'))
  _eq(f.done, walker.over.astype(np.uint8), (what, 'done'))
  _eq(f.ret, walker.ret, (what, 'ret'))


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_every_launch_of_the_tier_against_the_model(c, monkeypatch):
  import contextlib
  import torch
  from campx_amd import _hip, fused
  monkeypatch.setattr(fused, 'PAD_ROWS', c.padded)
  DTYPES = (torch.int8, torch.float16, torch.bfloat16)
  with (_hip.config(wide_lds_max=0) if c.lds0 else contextlib.nullcontext()):
    g, f = _game(c)
    B, S = c.B, c.S
    planes = f._n_planes
    bad = _BadIds()

    # 1. showtime(): state 0, broadcast over the environments
    first, reward, discount = f.showtime()
    obs0, board0 = ref.render(g, [0])
    _eq(first.layered_board, np.repeat(obs0, B, 0), 'showtime obs')
    _eq(first.board, np.repeat(board0, B, 0), 'showtime board')
    _eq(f._step_trace, np.repeat(ref.trace(g, [0]), B, 1), 'showtime trace')
    assert reward is None and discount == 1.0
    walker = ref.Walker(g, B)
    _state(f, walker, 'showtime')

    # 2. play(): a few frames, ids 5 / -1 / 127 in some environments
    acts = _actions(c, 1, 4, bad=True)
    for t in range(len(acts)):
      bad.call(f.play, torch.from_numpy(acts[t]).cuda())
      want = walker.rollout(acts[t:t + 1])
      obs, board = ref.render(g, want['states'][0])
      _eq(f._obs, obs, ('play obs', t))
      _eq(f._board, board, ('play board', t))
      _eq(f._step_trace, ref.trace(g, want['states'][0]), ('play trace', t))
      if c.reward:
        _eq(f._reward, want['reward'][0], ('play reward', t))
      _eq(f._discount, want['discount'][0], ('play discount', t))
      _eq(f._step_done, want['done'][0], ('play done', t))
      if c.perf:
        _eq(f.perf, want['perf'][0], ('play perf', t))
      _state(f, walker, ('play', t))
    bad.call(f.check_actions)
    assert bad.count == walker.bad > 0

    # 3. rollout(): T = 1, 7, 9, 20 in a row; rollout_trace() from the same start
    for i, (T, reset) in enumerate(ROLLOUTS):
      what = 'rollout T={}'.format(T)
      a = _actions(c, 10 + i, T)
      ids = torch.from_numpy(a).cuda()
      start = (f.state.clone(), f.done.clone(), f.ret.clone())
      out = f.rollout(ids, want_board=True, reset_first=reset)
      before = (walker.state.copy(), walker.over.copy(), walker.ret.copy())
      want = walker.rollout(a, reset_first=reset)
      obs, board = ref.render(g, want['states'].reshape(-1))
      obs = obs.reshape((T, B) + obs.shape[1:])
      want_trace = ref.trace(g, want['states'].reshape(-1)).reshape(planes, T, B)
      _eq(out['obs'], obs, (what, 'obs'))
      _eq(out['board'], board.reshape((T, B) + board.shape[1:]), (what, 'board'))
      _eq(out['trace'], want_trace, (what, 'trace'))
      _scalars(c, out, want, what)
      _state(f, walker, what)
      if c.sixteen and reset:                 # (from a reset: the same frames whatever came before)
        for dtype in DTYPES[1:]:
          again = f.rollout(ids, obs_dtype=dtype, reset_first=True)
          _eq(again['obs'], _sixteen(obs, dtype), (what, dtype))
          _eq(again['trace'], want_trace, (what, dtype, 'trace'))
          _state(f, walker, (what, dtype))
      for x, y in zip((f.state, f.done, f.ret), start):
        x.copy_(y)
      only = f.rollout_trace(ids, reset_first=reset)
      _eq(only['trace'], want_trace, (what, 'rollout_trace trace'))
      _scalars(c, only, want, (what, 'rollout_trace'))
      _state(f, walker, (what, 'rollout_trace'))

      # 4. render_frames(): sampled (t, e) pairs of the 20-frame rollout's trace
      if T == 20:
        rng = np.random.RandomState(c.seed + 5)
        t_idx, e_idx = rng.randint(0, T, size=300), rng.randint(0, B, size=300)
        t_idx[:2], e_idx[:2] = (0, T - 1), (0, B - 1)
        for dtype in DTYPES:
          got = f.render_frames(only['trace'], torch.from_numpy(t_idx).cuda(), torch.from_numpy(e_idx).cuda(),
                                obs_dtype=dtype)
          _eq(got, _want_obs(obs[t_idx, e_idx], dtype), ('render_frames', dtype))
    f.check_actions()

    # 5. rollout_policy() against PolicyWalker on the same table
    w = _policy(c)
    policy = torch.from_numpy(w).cuda()
    pw = pref.PolicyWalker(g, B)
    pw.state, pw.over, pw.ret = walker.state.copy(), walker.over.copy(), walker.ret.copy()
    calls = [dict(T=T, reset_first=reset) for T, reset in POLICY_ROLLOUTS]
    calls += [dict(T=9, first_frame=(1 << 40) + 6), dict(T=7, want_states=False),
              dict(T=20, want_states=False, reset_first=True)]
    for kw in calls:
      what = 'rollout_policy {}'.format(sorted(kw.items()))
      T, states = kw.pop('T'), kw.get('want_states', True)
      out = f.rollout_policy(policy, T, seed=SEED, **kw)
      kw.pop('want_states', None)
      want = pw.rollout(w, T, seed=SEED, **kw)
      assert want['bad'] == 0
      _eq(out['actions'], want['actions'], (what, 'actions'))
      if states:
        _eq(out['states'], want['states'], (what, 'states'))
      else:
        assert 'states' not in out
      _scalars(c, out, want, what)
      _state(f, pw, what)
      after = g.st_next[want['states'].astype(np.int64), want['actions'].astype(np.int64)]
      _eq(out['trace'], ref.trace(g, after.reshape(-1)).reshape(planes, T, B), (what, 'trace'))
    assert f._policy_frame == (1 << 40) + 6 + 9 + 7 + 20
    f.check_actions()

    # 6. render_states(): every state, and a repeated and shuffled list of ids
    rng = np.random.RandomState(c.seed + 6)
    ids = rng.randint(0, S, size=4099)
    ids[:2] = (0, S - 1)
    every = ref.render(g, np.arange(S))[0]
    some = every[ids]
    for n, dtype in enumerate(DTYPES):
      _eq(f.render_states(obs_dtype=dtype), _want_obs(every, dtype), ('render_states all', dtype))
      dev = torch.from_numpy(ids.astype(np.int32 if n == 1 else np.int64)).cuda()
      _eq(f.render_states(dev, obs_dtype=dtype), _want_obs(some, dtype), ('render_states ids', dtype))
    f.check_actions()


@pytest.mark.gpu
@pytest.mark.parametrize('lds0', [False, True], ids=['lds', 'lds0'])
def test_rollout_trace_streams_are_rollouts(lds0):
  """`rollout()` and `rollout_trace()` launch the update pass through one function: the same actions
  from the same start leave the same 'trace', 'reward', 'discount', 'done' and 'perf' - bit for bit,
  against each other and against the model - on a table with discount codes and hidden performance,
  with the table in LDS and read through the caches."""
  import contextlib
  import torch
  from campx_amd import _hip
  c = Case(seed=4100, rows=3, cols=7, L=3, K=2, S=37, V=1, P=0, dcodes=True, perf=True, reward=True,
           B=17, padded=False, lds0=lds0, sixteen=False)
  T = 3
  with (_hip.config(wide_lds_max=0) if lds0 else contextlib.nullcontext()):
    g, f = _game(c)
    f.showtime()
    walker = ref.Walker(g, c.B)
    lead = _actions(c, 30, 5)                    # (a start that is not state 0 everywhere)
    f.rollout_trace(torch.from_numpy(lead).cuda())
    walker.rollout(lead)
    assert len(set(walker.state.tolist())) > 1
    a = _actions(c, 31, T)
    ids = torch.from_numpy(a).cuda()
    start = (f.state.clone(), f.done.clone(), f.ret.clone())
    full = f.rollout(ids)
    after = (f.state.clone(), f.done.clone(), f.ret.clone())
    for x, y in zip((f.state, f.done, f.ret), start):
      x.copy_(y)
    only = f.rollout_trace(ids)
    want = walker.rollout(a)
    want['trace'] = ref.trace(g, want['states'].reshape(-1)).reshape(f._n_planes, T, c.B)
    assert len(set(want['discount'].reshape(-1).tolist()) - {0.0, 1.0}) >= 2 and want['perf'].any()
    for k in ('trace', 'reward', 'discount', 'done', 'perf'):
      _eq(only[k], _bits(full[k]), ('rollout_trace against rollout', k))
      _eq(full[k], want[k], ('rollout', k))
      _eq(only[k], want[k], ('rollout_trace', k))
    for x, y in zip((f.state, f.done, f.ret), after):
      _eq(x, _bits(y), 'state after')
    _state(f, walker, 'rollout_trace')


DIRECT = [i for i, c in enumerate(CASES) if (c.K in (3, 5, 8) or c.S == 1) and c.B <= 257][:12]


@pytest.mark.gpu
@pytest.mark.parametrize('c', [CASES[i] for i in DIRECT], ids=[IDS[i] for i in DIRECT])
@pytest.mark.parametrize('missing', ['discount', 'done', 'all'])
def test_missing_output_streams_take_the_general_chunk(c, missing):
  """`WideGame` always asks for 'discount' and 'done'; the ops take None for either (and for
  'reward', 'perf'), which sends every frame through the general chunk whatever the table: driven
  directly, as test_policy_rollout._op_args does it.  T = 20 from frame 8: two whole chunks that
  would otherwise be plain."""
  import contextlib
  import torch
  from campx_amd import _hip
  T, B = 20, c.B
  with (_hip.config(wide_lds_max=0) if c.lds0 else contextlib.nullcontext()):
    g, f = _game(c)
    planes = f._n_planes
    drop = ('reward', 'discount', 'done', 'perf') if missing == 'all' else (missing,)
    # the open-loop update pass
    a = _actions(c, 20, T)
    bufs = f.rollout_trace_buffers(T)
    for k in drop:
      bufs[k] = None
    _hip.ops.wide_update(f._spec_host, f._tables, f.state, f.done, f.ret, torch.from_numpy(a).cuda(),
                         bufs['reward'], bufs['discount'], bufs['done'], bufs['perf'], bufs['trace'],
                         f._bad, None, True)
    walker = ref.Walker(g, B)
    want = walker.rollout(a, reset_first=True)
    _eq(bufs['trace'], ref.trace(g, want['states'].reshape(-1)).reshape(planes, T, B), 'update trace')
    for k in ('reward', 'discount', 'done', 'perf'):
      if bufs[k] is not None:
        _eq(bufs[k], want[k], ('update', k))
    _state(f, walker, 'update')
    # the closed loop
    w = _policy(c)
    bufs = f.rollout_policy_buffers(T)
    for k in drop:
      bufs[k] = None
    _hip.ops.wide_policy_update(f._spec_host, f._tables, f.state, f.done, f.ret, torch.from_numpy(w).cuda(),
                                5, 8, bufs['reward'], bufs['discount'], bufs['done'], bufs['perf'],
                                bufs['trace'], bufs['actions'], bufs['states'], f._bad_rows, None, False)
    pw = pref.PolicyWalker(g, B)
    pw.state, pw.over, pw.ret = walker.state.copy(), walker.over.copy(), walker.ret.copy()
    want = pw.rollout(w, T, seed=5, first_frame=8)
    _eq(bufs['actions'], want['actions'], 'policy actions')
    _eq(bufs['states'], want['states'], 'policy states')
    after = g.st_next[want['states'].astype(np.int64), want['actions'].astype(np.int64)]
    _eq(bufs['trace'], ref.trace(g, after.reshape(-1)).reshape(planes, T, B), 'policy trace')
    for k in ('reward', 'discount', 'done', 'perf'):
      if bufs[k] is not None:
        _eq(bufs[k], want[k], ('policy', k))
    _state(f, pw, 'policy')
    assert int(f._bad.item()) == 0 and int(f._bad_rows.item()) == 0
