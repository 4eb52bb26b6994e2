"""The tables of a `tabulate.TracedGame` restated ONE EDGE AT A TIME: the checker of
tests/test_traced_tables.py.

`campx_amd.tabulate._fill_tables` builds the state table, the discount codes, the hidden
performance and the dense table of both state-graph walkers from arrays, without a Python loop over
states or edges; so the two walkers agreeing with each other no longer says anything about it.
This is the loop it replaced, a Python statement per edge and field, fed with the game's own graph
(`st_next` / `st_reached` / `st_reward` / `st_done` / `st_discount`) in the order a breadth-first
walk meets the edges - derived here, from the graph alone.  numpy only; nothing from `campx_amd`.
"""

import collections

import numpy as np

N_ACTIONS = 5


def edges_of(game):
  """[(s, a, t, reward, over, discount)] in the order the one-frame-per-play walk plays them:
  breadth-first from state 0, actions 0..4; a state joins the queue the first time an edge that
  does not end the episode reaches it.  A state only ever reached by ending edges has none."""
  queue, queued, edges = collections.deque([0]), {0}, []
  while queue:
    s = queue.popleft()
    for a in range(N_ACTIONS):
      assert game.st_reached[s, a], (s, a)
      t, over = int(game.st_next[s, a]), bool(game.st_done[s, a])
      edges.append((s, a, t, game.st_reward[s, a], over, float(game.st_discount[s, a])))
      if not over and t not in queued:
        queued.add(t)
        queue.append(t)
  return edges


def _perf_of(game):
  """None, or f(cells before, cells after) -> the hidden performance of a frame
  (`Engine.set_hidden_penalty` / `Engine.set_hidden_performance`)."""
  HW, movers = game.rows * game.cols, game.movers
  if game.penalty_spec is not None:
    who, masks, unit = game.penalty_spec
    cls = np.zeros(HW, np.int32)
    for k, m in enumerate(masks):
      cls[np.flatnonzero(m.detach().cpu().numpy().reshape(-1))] = k + 1
    watched = [movers.index(ch) for ch in who]
    return lambda src, dst: int(unit) * sum(int(cls[dst[k]]) for k in watched)
  if game.perf_spec is not None:
    agent, masks = game.perf_spec
    cls = np.zeros(HW, np.int32)
    for k, m in enumerate(masks):
      cls[np.flatnonzero(m.detach().cpu().numpy().reshape(-1))] = k + 1
    n_cls, who = len(masks), movers.index(agent)

    def perf_of(src, dst):
      a, b = int(cls[src[who]]), int(cls[dst[who]])
      if a == 0 or b == 0:
        return 0
      fwd = 1 if a == n_cls else a + 1
      back = n_cls if a == 1 else a - 1
      return int(b == fwd) - int(b == back)
    return perf_of
  return None


def tables_of(game):
  """{field: value} of everything `_fill_tables` derives from the graph: the state table's
  per-edge fields with their defaults for edges never played, `discount_list`, and - for a game
  with a dense table - that table.  From `game`'s graph, `st_cells`, `st_mode`, `st_shows`."""
  HW, K, S = game.rows * game.cols, len(game.movers), game.n_states
  Kt = K + (1 if len(game.mode_orders) > 1 else 0)
  state_cells = [tuple(int(c) for c in game.st_cells[s]) + ((int(game.st_mode[s]),) if Kt > K else ())
                 for s in range(S)]
  edges = edges_of(game)
  perf_of = _perf_of(game)

  # ---- the state table: one row per reachable state
  out = dict(
      st_next=np.tile(np.arange(S, dtype=np.int32)[:, None], (1, N_ACTIONS)),
      st_reward=np.full((S, N_ACTIONS), np.nan, np.float32),
      st_done=np.zeros((S, N_ACTIONS), np.uint8),
      st_discount=np.ones((S, N_ACTIONS), np.float32),
      st_dcode=np.zeros((S, N_ACTIONS), np.uint8),
      st_perf=np.zeros((S, N_ACTIONS), np.int8),
      st_reached=np.zeros((S, N_ACTIONS), bool))
  discount_list = [1.0]               # code -> value; code 0 stands for the default
  for s, a, t, reward, over, discount in edges:
    out['st_next'][s, a] = t
    out['st_reward'][s, a] = reward
    out['st_done'][s, a] = int(over)
    out['st_discount'][s, a] = discount
    if discount != (0.0 if over else 1.0):
      if discount not in discount_list[1:]:
        assert len(discount_list) < 16
        discount_list.append(discount)
      out['st_dcode'][s, a] = 1 + discount_list[1:].index(discount)
    out['st_perf'][s, a] = perf_of(state_cells[s], state_cells[t]) if perf_of else 0
    out['st_reached'][s, a] = True
  out['discount_list'] = discount_list
  out['any_reward'] = bool((~np.isnan(out['st_reward'][out['st_reached']])).any())
  out['has_perf'] = perf_of is not None
  out['init_cells'] = state_cells[0]
  out['init_visible'] = [int(v) for v in game.st_shows[0]]
  out['n'] = None
  if game.dense_reason is not None:
    return out

  # ---- the dense table (one-cell tier)
  n = HW ** Kt * N_ACTIONS
  out.update(
      n=n, next_cells=np.zeros((Kt, n), np.uint16), visible=np.zeros((Kt, n), np.uint8),
      reward=np.full((n,), np.nan, np.float32), done=np.zeros((n,), np.uint8),
      discount=np.ones((n,), np.float32), dcode=np.zeros((n,), np.uint8),
      perf=np.zeros((n,), np.int8), reached=np.zeros((n,), bool))
  # entries nobody can reach: stay where you are, pay nothing
  idx = np.arange(n) // N_ACTIONS
  for k in range(Kt - 1, -1, -1):
    out['next_cells'][k] = idx % HW
    idx = idx // HW
  for s, a, t, _, _, _ in edges:
    i = 0
    for c in state_cells[s]:
      i = i * HW + c
    i = i * N_ACTIONS + a
    dst = state_cells[t]
    for k in range(K):
      out['next_cells'][k, i] = dst[k]
      out['visible'][k, i] = game.st_shows[t, k]
    if Kt > K:
      out['next_cells'][K, i] = dst[K]            # the mode: never visible
    out['reward'][i] = out['st_reward'][s, a]
    out['done'][i] = out['st_done'][s, a]
    out['discount'][i] = out['st_discount'][s, a]
    out['dcode'][i] = out['st_dcode'][s, a]
    out['perf'][i] = out['st_perf'][s, a]
    out['reached'][i] = True
  return out


def first_difference(game, want):
  """The first field of `want` (`tables_of`) that `game` has otherwise, or None: arrays by dtype,
  shape and value - float32 as bit patterns -, anything else by `repr`."""
  for name, w in want.items():
    v = getattr(game, name)
    if isinstance(w, np.ndarray):
      same = (isinstance(v, np.ndarray) and v.dtype == w.dtype and v.shape == w.shape and
              np.array_equal(v.view(np.uint32) if v.dtype == np.float32 else v,
                             w.view(np.uint32) if w.dtype == np.float32 else w))
    else:
      same = repr(v) == repr(w)
    if not same:
      return name
  return None
