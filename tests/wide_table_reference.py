"""The state-table tier restated in numpy from include/campx_hip.h (`CampxWideSpec`, the trace
entry, `CampxTransition.done`), and a generator of synthetic state TABLES that a game could have
produced: the checker of tests/test_wide_table_fuzz.py.  No torch, no HIP, no code shared with
campx_amd/csrc; nothing from `campx_amd` that computes an observation or a trace.

A table is anything with the attributes of a `tabulate.TracedGame` that the state-table tier reads
(`SyntheticTable` below fills them; a real `TracedGame` has them): `view()` turns either into the
header's terms -

  things      the movers that are not handed over as a piece mask: their layer, and per state the
              cell they are on (0 for one that is not on the board) and whether they SHOW there;
  pieces      with `pieces_as_mask`, the movers that have a `piece_cell` and show in some state:
              cell, layer, and per state the 16-bit mask of those that show;
  tops        [V][rows*cols] the front-most scenery layer per cell in each variant of the scenery
              (backdrop picture, then the things that never move, back to front), and per state
              the variant that shows

- and `render()` / `trace()` / `Walker` say what the header says of them:

  observation the top layer per cell is the scenery's of the state's variant; a piece that shows
              replaces it on its cell, a thing that shows on its; `obs` is one-hot over the layers,
              `board` is `layer_char[top]`;
  trace       per thing `cell | (scenery layer it covers there) << 10 | shows << 15`; one more
              plane with the variant index (V > 1) or the piece mask (P > 0);
  walk        (state, action) -> state; an action id outside 0..4 is action 4 and is counted; an
              environment whose episode ended starts its next frame from state 0 with `ret`
              cleared; the discount of a frame is `discount_list[code]`, or - code 0 - 0.0 when the
              frame ended the episode and 1.0 otherwise.
"""

import numpy as np

N_ACTIONS = 5
REWARDS = np.array([np.nan, -0.0, 0.0, 1.0, -1.0, 0.1, 1e6], np.float32)
DONE_SHARE = 0.12
_CHARS = ' #$*+.:=@ABDEGKPXkosx~'


# --------------------------------------------------------------------------- the generator

class SyntheticTable(object):
  """A state table with the attributes of a `tabulate.TracedGame` (see `make_table`)."""

  mode_orders = None
  variant_masks = None
  statics = ()
  pieces_as_mask = True

  def model_board(self, cells, movers=True, variant=0):
    """The scenery alone (character codes [rows, cols]) of picture `variant`: all that
    `tabulate.to_wide_spec()` asks of a table.  What a STATE looks like is `render()`'s business."""
    assert not movers
    return self.variants[variant].copy()

  def done_bytes(self):
    return (self.st_done | (self.st_dcode << 4)).astype(np.uint8)


def default_discount(code, done, discount_list):
  """include/campx_hip.h, CampxTransition.done: the frame reports discount_list[code], or - code
  0 - the default, 0.0 when it terminated and 1.0 otherwise."""
  code, done = np.asarray(code), np.asarray(done)
  listed = np.asarray(discount_list, np.float32)[code]
  return np.where(code != 0, listed, np.where(done != 0, np.float32(0), np.float32(1))).astype(np.float32)


def make_table(seed, rows, cols, n_layers, K, S, V=1, P=0, dcodes=False, perf=False,
               any_reward=True):
  """A legal table of S states for K things on a rows x cols board of n_layers characters, with V
  pictures of the scenery or P pieces of it; seeded, the same on every machine.

  Only what a game could produce: every state reachable from state 0 along entries that do not
  end the episode; things that show stand on distinct cells, on no cell whose piece shows, and
  never paint the layer the scenery shows there; hidden things are anywhere (or nowhere)."""
  assert 1 <= K <= 8 and S >= 1 and n_layers >= 2 and rows * cols >= 16
  assert not (V > 1 and P > 0) and (K <= 7 or (V == 1 and P == 0))
  assert S >= 2 or (V == 1 and P == 0), 'one state cannot show two variants or two masks'
  assert S >= 4 or not dcodes, 'fifteen codes need fifteen entries'
  rng = np.random.RandomState(seed)
  HW = rows * cols
  g = SyntheticTable()
  g.rows, g.cols, g.n_states = rows, cols, S
  g.chars = sorted(rng.choice(list(_CHARS), size=n_layers, replace=False).tolist())
  codes = np.array([ord(c) for c in g.chars], np.uint8)
  g.any_reward, g.has_perf = bool(any_reward), bool(perf)

  # the scenery: V pictures; every layer appears in each, so that every thing finds cells to show on
  tops = rng.randint(0, n_layers, size=(V, HW))
  for v in range(V):
    tops[v, rng.choice(HW, size=n_layers, replace=False)] = np.arange(n_layers)
  g.variants = [codes[tops[v]].reshape(rows, cols) for v in range(V)]
  g.backdrop = g.variants[0]
  variant = rng.randint(0, V, size=S)
  if V > 1:
    variant[rng.choice(S, size=2, replace=False)] = [0, V - 1]
  g.st_variant = variant.astype(np.uint16)

  # the pieces: P distinct cells, each of a layer the plain scenery does not show there
  piece_cell = rng.choice(HW, size=P, replace=False) if P else np.zeros(0, np.int64)
  piece_layer = np.array([(tops[0, c] + 1 + rng.randint(0, n_layers - 1)) % n_layers for c in piece_cell],
                         np.int64)
  mask = rng.randint(0, 1 << 16, size=S) & ((1 << P) - 1)
  mask[rng.randint(0, S, size=max(1, S // 8))] = (1 << P) - 1     # (crowded boards too)
  if P:
    mask[rng.choice(S, size=2, replace=False)] = [0, (1 << P) - 1]

  # the things: two may share a layer
  layer = rng.randint(0, n_layers, size=K)
  g.movers = [g.chars[l] for l in layer] + [g.chars[l] for l in piece_layer]
  g.piece_cell = [None] * K + [int(c) for c in piece_cell]
  g.z_order = list(g.chars)
  cells = np.zeros((S, K + P), np.int64)
  shows = np.zeros((S, K + P), np.uint8)
  present = np.ones((S, K + P), bool)
  for s in range(S):
    taken = np.zeros(HW, bool)
    for p in range(P):
      taken[piece_cell[p]] = (mask[s] >> p) & 1
    top = tops[variant[s]]
    for d in range(K):
      free = np.flatnonzero(~taken & (top != layer[d])) if rng.rand() < 0.7 else ()
      if len(free):
        cells[s, d] = free[rng.randint(len(free))]
        shows[s, d] = 1
        taken[cells[s, d]] = True
      else:                                    # hidden: anywhere, or not on the board at all
        cells[s, d] = rng.randint(HW)
        present[s, d] = rng.rand() < 0.6
  for p in range(P):
    cells[:, K + p] = piece_cell[p]
    shows[:, K + p] = (mask >> p) & 1
  g.st_cells, g.st_shows, g.st_present = cells.astype(np.uint16), shows, present
  g.init_cells = tuple(int(c) for c in cells[0])

  # the transitions: a random spanning structure from state 0, the rest uniform over the states
  nxt = rng.randint(0, S, size=(S, N_ACTIONS))
  tree = np.zeros((S, N_ACTIONS), bool)
  open_slots = [(0, a) for a in range(N_ACTIONS)]
  for s in range(1, S):
    parent, a = open_slots.pop(rng.randint(len(open_slots)))
    nxt[parent, a], tree[parent, a] = s, True
    open_slots.extend((s, b) for b in range(N_ACTIONS))
  g.st_next = nxt.astype(np.int32)
  rest = np.flatnonzero(~tree.reshape(-1))
  n_done = max(1, int(round(DONE_SHARE * S * N_ACTIONS)))
  done = np.zeros(S * N_ACTIONS, np.uint8)
  done[rng.choice(rest, size=min(n_done, len(rest)), replace=False)] = 1
  g.st_done = done.reshape(S, N_ACTIONS)
  if any_reward:
    g.st_reward = REWARDS[rng.randint(0, len(REWARDS), size=(S, N_ACTIONS))]
    g.st_reward.reshape(-1)[rng.choice(S * N_ACTIONS, size=min(len(REWARDS), S * N_ACTIONS), replace=False)] = \
        REWARDS[:min(len(REWARDS), S * N_ACTIONS)]
  else:
    g.st_reward = np.full((S, N_ACTIONS), np.nan, np.float32)
  g.discount_list = [1.0] + [float(x) for x in rng.permutation(
      np.array([0.0, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 0.999, 1.0, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7], np.float32))]
  dcode = np.zeros(S * N_ACTIONS, np.uint8)
  if dcodes:
    dcode[:] = rng.randint(0, 16, size=S * N_ACTIONS)
    dcode[rng.choice(S * N_ACTIONS, size=15, replace=False)] = np.arange(1, 16)
  g.st_dcode = dcode.reshape(S, N_ACTIONS)
  g.st_discount = default_discount(g.st_dcode, g.st_done, g.discount_list)
  if perf:
    g.st_perf = rng.randint(-128, 128, size=(S, N_ACTIONS)).astype(np.int8)
    g.st_perf.reshape(-1)[rng.choice(S * N_ACTIONS, size=2, replace=False)] = [-128, 127]
  else:
    g.st_perf = np.zeros((S, N_ACTIONS), np.int8)
  g.st_reached = np.ones((S, N_ACTIONS), bool)
  return g


# --------------------------------------------------------------------------- the model

class View(object):
  """A table in the header's terms (module docstring)."""


def integer_table():
  """A synthetic table with discounts of 1 (no discount codes; an entry that ends the episode
  bootstraps from nothing), its rewards - 0.1 and 1e6 among them - replaced by small integers: 0.1
  becomes 2 and 1e6 becomes 3 (None stays None).  With alpha = gamma = epsilon = 0.5 and q0 = 0 a
  learner's first frames round nothing away."""
  F = np.float32
  g = make_table(77, 4, 5, 4, 2, 12, dcodes=False, perf=True)
  r = g.st_reward
  g.st_reward = np.where(r == F(0.1), F(2), np.where(np.abs(r) == F(1e6), np.sign(r) * F(3), r)).astype(F)
  reward = np.where(np.isnan(g.st_reward), 0, g.st_reward)
  assert np.array_equal(reward, np.rint(reward)) and (g.st_discount[g.st_done == 0] == 1).all()
  return g


def _scenery(table, v):
  """Character codes [rows*cols] of picture v of the scenery: the backdrop's picture, then the things
  that never move (and the several-cell drapes this picture holds), back to front."""
  variants = getattr(table, 'variants', None)
  board = np.array(variants[v] if variants else table.backdrop, np.uint8).reshape(-1).copy()
  static = {ch: np.asarray(m) for ch, m in (getattr(table, 'statics', None) or ())}
  masks = getattr(table, 'variant_masks', None)
  if masks:
    static.update({ch: np.asarray(m) for ch, m in masks[v].items()})
  orders = getattr(table, 'mode_orders', None)
  for ch in (orders[0] if orders else table.z_order):
    if ch in static:
      board[static[ch].reshape(-1) != 0] = ord(ch)
  return board


def view(table):
  cached = table.__dict__.get('_wide_view')
  if cached is not None:
    return cached
  w = View()
  w.rows, w.cols, w.chars = int(table.rows), int(table.cols), list(table.chars)
  w.layer_char = np.array([ord(c) for c in w.chars], np.uint8)
  layer_of = {ord(c): i for i, c in enumerate(w.chars)}
  n_movers = len(table.movers)
  as_mask = bool(getattr(table, 'pieces_as_mask', False))
  shows = np.asarray(table.st_shows)[:, :n_movers] != 0
  is_piece = [as_mask and table.piece_cell[k] is not None for k in range(n_movers)]
  things = [k for k in range(n_movers) if not is_piece[k]]
  pieces = [k for k in range(n_movers) if is_piece[k] and shows[:, k].any()]
  w.K, w.P, w.S = len(things), len(pieces), int(table.n_states)
  w.thing_layer = np.array([layer_of[ord(table.movers[k])] for k in things], np.int64)
  present = np.asarray(table.st_present)[:, :n_movers]
  cells = np.where(present, np.asarray(table.st_cells)[:, :n_movers], 0).astype(np.int64)
  w.cells, w.shows = cells[:, things], shows[:, things]
  variants = getattr(table, 'variants', None)
  w.V = len(variants) if variants else 1
  w.tops = np.array([[layer_of[int(c)] for c in _scenery(table, v)] for v in range(w.V)], np.int64)
  w.variant = (np.asarray(table.st_variant, np.int64) if w.V > 1 else np.zeros(w.S, np.int64))
  w.piece_cell = np.array([int(table.piece_cell[k]) for k in pieces], np.int64)
  w.piece_layer = np.array([layer_of[ord(table.movers[k])] for k in pieces], np.int64)
  w.mask = np.zeros(w.S, np.int64)
  for p, k in enumerate(pieces):
    w.mask |= shows[:, k].astype(np.int64) << p
  w.planes = w.K + (1 if w.V > 1 or w.P > 0 else 0)
  table.__dict__['_wide_view'] = w
  return w


def top_layers(table, state_ids):
  """int64 [N, rows*cols]: the layer every cell shows in the given states."""
  w = view(table)
  s = np.asarray(state_ids, np.int64).reshape(-1)
  n = np.arange(len(s))
  top = w.tops[w.variant[s]].copy()
  for p in range(w.P):
    on = ((w.mask[s] >> p) & 1) != 0
    top[n[on], w.piece_cell[p]] = w.piece_layer[p]
  for d in range(w.K):
    on = w.shows[s, d]
    top[n[on], w.cells[s, d][on]] = w.thing_layer[d]
  return top


def render(table, state_ids):
  """-> (obs int8 [N, L, H, W] one-hot over the layers, board int8 [N, H, W] character codes)."""
  w = view(table)
  top = top_layers(table, state_ids)
  obs = (top[:, None, :] == np.arange(len(w.chars))[None, :, None]).astype(np.int8)
  board = w.layer_char[top].astype(np.int8)
  return obs.reshape(len(top), len(w.chars), w.rows, w.cols), board.reshape(len(top), w.rows, w.cols)


F16_ONE, BF16_ONE = 0x3c00, 0x3f80


def as_bits16(obs, one):
  """The 16-bit forms of an int8 0 / 1 observation, as their bit patterns (int16)."""
  return (obs.astype(np.int16) * np.int16(one)).astype(np.int16)


def trace(table, state_ids):
  """-> uint16 [planes, N]: per thing cell | covered scenery layer << 10 | shows << 15, then the
  variant index or the piece mask."""
  w = view(table)
  s = np.asarray(state_ids, np.int64).reshape(-1)
  out = np.zeros((w.planes, len(s)), np.uint16)
  tops = w.tops[w.variant[s]]
  n = np.arange(len(s))
  for d in range(w.K):
    cell = w.cells[s, d]
    out[d] = cell | (tops[n, cell] << 10) | (w.shows[s, d].astype(np.int64) << 15)
  if w.V > 1:
    out[w.K] = w.variant[s]
  elif w.P > 0:
    out[w.K] = w.mask[s]
  return out


class Walker(object):
  """B environments walked through a table's `st_*` arrays under given actions."""

  def __init__(self, table, batch):
    self.table = table
    self.B = int(batch)
    self.state = np.zeros(self.B, np.int64)
    self.over = np.zeros(self.B, bool)
    self.ret = np.zeros(self.B, np.float32)
    self.bad = 0

  def reset(self):
    self.state[:] = 0
    self.over[:] = False
    self.ret[:] = 0

  def rollout(self, actions, reset_first=False):
    """actions int8 [T, B] -> dict(states int64 (the state each frame REACHED), reward, discount
    float32, done uint8, perf int8, all [T, B]); `state`, `over`, `ret`, `bad` carry over."""
    g = self.table
    actions = np.asarray(actions)
    T = actions.shape[0]
    out = dict(states=np.zeros((T, self.B), np.int64), reward=np.zeros((T, self.B), np.float32),
               discount=np.zeros((T, self.B), np.float32), done=np.zeros((T, self.B), np.uint8),
               perf=np.zeros((T, self.B), np.int8))
    if reset_first:
      self.over[:] = True
    for t in range(T):
      a = actions[t].astype(np.int64)
      wrong = (a < 0) | (a >= N_ACTIONS)
      self.bad += int(wrong.sum())
      a = np.where(wrong, N_ACTIONS - 1, a)
      s = np.where(self.over, 0, self.state)
      ret = np.where(self.over, np.float32(0), self.ret).astype(np.float32)
      reward = g.st_reward[s, a].astype(np.float32)
      self.ret = (ret + np.where(np.isnan(reward), np.float32(0), reward)).astype(np.float32)
      self.state = g.st_next[s, a].astype(np.int64)
      self.over = g.st_done[s, a] != 0
      out['states'][t] = self.state
      out['reward'][t] = reward
      out['discount'][t] = g.st_discount[s, a]
      out['done'][t] = self.over
      out['perf'][t] = g.st_perf[s, a]
    return out
