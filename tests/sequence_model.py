"""Sequences of the state-table tier's stateful calls: the plan of a case and a host model that
runs it, for tests/test_state_table_sequences.py (GPU) and tests/test_sequence_model_cpu.py.

`plan(game_name, seed)` is a pure function of its arguments: 14 operations, each a dict with all of
its arguments (arrays are named by a salt and made by `actions()` / `policy()` / `population()`
below).  `SequenceModel` runs such a plan on the host.  It holds the four existing references over
one table - `wide_table_reference.Walker`, `policy_reference.PolicyWalker`,
`population_reference.PopulationWalker`, `learner_reference.Learners` - and re-implements no
arithmetic: every verb calls one of them, then hands `state`, `over` and `ret` to the other three
(and the Philox frame counter among the three that have one).  What it adds is the rule of the two
frame counters (campx_amd/wide.py):

  frame          every call advances it by its frames; `reset_first` restarts it at the call's
                 frames; reset() sets it to 0;
  policy_frame   only the sampling calls - policy, population, learn - advance it; an explicit
                 `first_frame` sets it; reset() leaves it alone.

`Walker.rollout()` returns the state each frame REACHED ('reached' below); `PolicyWalker` and
`PopulationWalker` return the state each frame STARTED FROM ('states', as the device returns it).

`defect=` makes the model wrong on purpose, one contract at a time (DEFECTS): the CPU file shows
that each defect changes some compared output of some case of every game, i.e. that the sequences
can see it.
"""

import functools

import numpy as np

import learner_reference as lref
import policy_reference as pref
import population_reference as popref
import wide_table_reference as wref

N_OPS = 14
GAMES = ('boat_race', 'maze', 'pickups', 'syn7v3', 'syn28p5', 'syn29')
# (states, hidden performance) of every game: what the plan needs to know of a table to replace an
# operation the game cannot take (a forced LDS path that does not fit).  Asserted on the CPU.
FACTS = {'boat_race': (8, 1), 'maze': (159, 0), 'pickups': (470, 0),
         'syn7v3': (7, 1), 'syn28p5': (28, 1), 'syn29': (29, 1)}
SYNTHETIC = {'syn7v3': dict(S=7, V=3), 'syn28p5': dict(S=28, P=5), 'syn29': dict(S=29)}
BATCHES = (1, 63, 64, 65, 256, 257, 1000)
ROLLOUT_T = (1, 2, 3, 5, 8, 9, 23)
CARRYING = ('play', 'rollout', 'trace', 'deferred', 'policy', 'population', 'learn', 'graph')
CLOSED = ('policy', 'population', 'learn')
KINDS = CARRYING + ('reset', 'bad')
PAIRS = [(x, y) for x in CARRYING for y in CARRYING]
DEFAULT_SEEDS = 4
FAR = (1 << 40) + 1
DEFECTS = {
    'a': 'open-loop calls also advance policy_frame',
    'b': 'reset() zeroes policy_frame',
    'c': 'a closed-loop call reads `state` instead of row 0 for an `over` environment at its first frame',
    'd': '`ret` is not restarted for such an environment',
    'e': 'learn leaves `over` as it found it',
    'f': 'the graph warm-up\'s two runs of frames are not undone',
    'g': 'the bad frames of `bad` stay where they are instead of taking action 4'}
# Seed offsets per game, searched on the CPU until the conditions of tests/test_sequence_model_cpu.py
# hold at DEFAULT_SEEDS seeds: per game the first offset 0, 1, 2 .. at which they do.
OFFSETS = {'boat_race': 3, 'maze': 9, 'pickups': 2, 'syn7v3': 1, 'syn28p5': 0, 'syn29': 0}


# --------------------------------------------------------------------------- tables and arrays

@functools.lru_cache(maxsize=None)
def table(name):
  """The table of a game, tabulated on the host (the real games) or generated (the synthetic
  ones: discount codes and hidden performance, as test_learner's)."""
  if name in SYNTHETIC:
    kw = dict(SYNTHETIC[name])
    S = kw.pop('S')
    return wref.make_table(S * 100 + 11, 4, 5, 4, 2, S, dcodes=True, perf=True, **kw)
  from campx_amd import tabulate
  if name == 'boat_race':
    from campx_amd.games import boat_race
    return tabulate.trace(boat_race.build())
  if name == 'maze':
    from campx_amd.games import maze
    return tabulate.trace(maze.build(16, 16))
  import random_pickups
  return tabulate.trace(random_pickups.builder(random_pickups.definitions()[3])())


def toward_done(g):
  """int64 [S]: per state the first action of a shortest way to an entry that ends the episode
  (None for a table without one).  Only steers the seeded policies and the first Q-table, so that
  episodes end while a case runs; nothing is compared with it."""
  if '_toward_done' not in g.__dict__:
    done = (np.asarray(g.st_done) != 0) & np.asarray(g.st_reached, bool)
    best = None
    if done.any():
      nxt = np.asarray(g.st_next, np.int64)
      dist = np.full(g.n_states, np.inf)
      for _ in range(g.n_states):
        cand = np.where(done, 1.0, 1.0 + dist[nxt])
        cand[~np.asarray(g.st_reached, bool)] = np.inf
        dist = cand.min(1)
      best = cand.argmin(1).astype(np.int64)
    g.__dict__['_toward_done'] = best
  return g.__dict__['_toward_done']


def actions(salt, T, B):
  return np.random.RandomState(salt).randint(0, 5, size=(T, B)).astype(np.int8)


def policy(g, salt, bad_rows=0):
  """Seeded weights float32 [S, 5]: rows 0, 4, 8 .. are one-hot, rows 1, 5, 9 .. have a weight of
  exactly 0, the others favour the way to an episode's end.  `bad_rows`: row 0 and that many rows
  less one elsewhere get a NaN or a negative weight."""
  rng = np.random.RandomState(salt)
  S = g.n_states
  w = rng.uniform(0.05, 1.0, size=(S, 5)).astype(np.float32)
  best = toward_done(g)
  if best is None:
    best = rng.randint(0, 5, size=S)
  rows = np.arange(S)
  w[rows, best] *= np.float32(8)
  w[0::4] = 0
  w[rows[0::4], best[0::4]] = 1
  odd = rows[1::4]
  w[odd, (best[odd] + 1 + rng.randint(0, 4, size=len(odd))) % 5] = 0
  if bad_rows:
    where = np.concatenate([[0], 1 + rng.choice(S - 1, size=min(bad_rows, S) - 1, replace=False)])
    for i, s in enumerate(where):
      w[s, rng.randint(5)] = np.nan if i % 2 == 0 else -0.5
  return w


def population(g, salt, P):
  return np.stack([policy(g, salt + 17 * m) for m in range(P)])


def first_q(g, B, salt):
  """The Q-table every learner of a case starts from: small noise, the way to an episode's end
  raised."""
  rng = np.random.RandomState(salt)
  q = rng.uniform(-0.1, 0.1, size=(B, g.n_states, 5)).astype(np.float32)
  best = toward_done(g)
  if best is not None:
    q[:, np.arange(g.n_states), best] += np.float32(1)
  return q


def hyper(B):
  from test_learner import _hyper
  return _hyper(B)


def pairs(salt, T, B, n=64):
  rng = np.random.RandomState(salt)
  t, e = rng.randint(0, T, size=n), rng.randint(0, B, size=n)
  t[:2], e[:2] = (0, T - 1), (0, B - 1)
  return t.astype(np.int64), e.astype(np.int64)


# --------------------------------------------------------------------------- the plan

def _lds_max():
  from campx_amd import _hip
  return _hip.config_get('wide_lds_max')


def population_fits(S, perf, B, P):
  import ctypes
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  return _hip.lib.campx_wide_population_plan(S, perf, B, P, _lds_max(), 1, out) == 0


def learn_fits(S, perf, B):
  import ctypes
  from campx_amd import _hip
  out = (ctypes.c_int64 * 4)()
  return _hip.lib.campx_wide_learn_plan(S, perf, B, _lds_max(), 1, out) == 0


def _kinds(rng, forced):
  """14 kinds: the forced adjacent pairs as one block at a drawn place, the rest drawn; redrawn
  until the case has 6 distinct kinds and 4 closed-loop calls."""
  block = [k for pair in forced for k in pair]
  weights = np.array([2, 3, 2, 2, 4, 4, 4, 3, 1.5, 1.5])
  while True:
    rest = list(rng.choice(KINDS, size=N_OPS - len(block), p=weights / weights.sum()))
    at = int(rng.randint(0, len(rest) + 1))
    kinds = rest[:at] + block + rest[at:]
    if len(set(kinds)) >= 6 and sum(k in CLOSED for k in kinds) >= 4:
      return kinds


def plan(game_name, seed):
  """The 14 operations of case (game_name, seed)."""
  S, perf = FACTS[game_name]
  gi = GAMES.index(game_name)
  rng = np.random.RandomState(1000 * seed + gi + 100003 * OFFSETS[game_name])
  B = int(rng.choice(BATCHES))
  case_seed = (int(rng.randint(1 << 31)) << 33) | (int(rng.randint(1 << 31)) << 2) | 1
  k = gi * DEFAULT_SEEDS + seed
  forced = [PAIRS[i] for i in (k, k + 24, k + 48) if seed < DEFAULT_SEEDS and i < len(PAIRS)]
  salt = lambda: int(rng.randint(1 << 30))
  draw = lambda xs: xs[int(rng.randint(len(xs)))]
  ops = []
  for kind in _kinds(rng, forced):
    op = dict(kind=kind, B=B)
    if kind == 'play':
      op.update(n=int(rng.randint(1, 4)), salt=salt())
    elif kind == 'rollout':
      op.update(T=int(draw(ROLLOUT_T)), reset_first=bool(rng.rand() < 0.2), salt=salt(),
                form=draw(('full', 'board', 'last', 'f16', 'bf16', 'out')))
    elif kind == 'trace':
      op.update(T=int(draw(ROLLOUT_T)), reset_first=bool(rng.rand() < 0.2), salt=salt(), pairs=salt())
    elif kind == 'deferred':
      op.update(T=int(draw(ROLLOUT_T)), n=int(rng.randint(1, 4)), salt=salt())
    elif kind in ('policy', 'population'):
      op.update(T=int(draw(ROLLOUT_T)), salt=salt(), seed=case_seed,
                first_frame=None if rng.rand() < 0.8 else draw((0, 6, FAR)),
                want_states=bool(rng.rand() >= 0.25), reuse_out=bool(rng.rand() < 1 / 3),
                reset_first=bool(rng.rand() < 0.2))
      if kind == 'population':
        P = draw([p for p in range(1, 17) if B % p == 0] + [B])
        path = draw((0, 1, 2))
        if path == 1 and not population_fits(S, perf, B, P):
          path = 2                                # (replaced here, never skipped at run time)
        op.update(P=int(P), path=int(path))
    elif kind == 'learn':
      T = int(draw(ROLLOUT_T))
      path = draw((0, 1, 2))
      if path == 1 and not learn_fits(S, perf, B):
        path = 2
      op.update(T=T, rule=draw(lref.RULES), window=draw((None, 1, 3, T, T + 2)), seed=case_seed,
                path=int(path), reset_first=bool(rng.rand() < 0.2))
    elif kind == 'graph':
      op.update(n=int(draw((1, 4))), salt=salt())
    elif kind == 'bad':
      op.update(what=draw(('policy', 'rollout')), T=int(draw(ROLLOUT_T)), k=int(rng.randint(1, 4)),
                salt=salt(), seed=case_seed)
    ops.append(op)
  assert len(ops) == N_OPS
  return ops


# --------------------------------------------------------------------------- the model

class SequenceModel(object):
  """Runs the operations of a plan on the host; `run(op)` returns what the device is to return,
  name by name, as numpy arrays (floats compared by bits).  `render=False` leaves out the frames
  (they are a function of 'reached', which is returned either way)."""

  def __init__(self, g, B, q_salt=0, render=True, defect=None):
    assert defect is None or defect in DEFECTS
    self.g, self.B, self.render, self.defect = g, int(B), render, defect
    self.walker = wref.Walker(g, B)
    self.policy_walker = pref.PolicyWalker(g, B)
    self.population_walker = popref.PopulationWalker(g, B)
    self.learners = lref.Learners(g, B, first_q(g, B, q_salt))
    self.state, self.over, self.ret = self.walker.state, self.walker.over, self.walker.ret
    self.frame = 0
    self.policy_frame = 0
    self.captured = set()
    self.log = []

  @property
  def q(self):
    return self.learners.q

  def _hand(self, src):
    """`state`, `over`, `ret` from the walker that ran to the other three (and here)."""
    self.state, self.over, self.ret = src.state.copy(), src.over.copy(), src.ret.copy()
    for w in (self.walker, self.policy_walker, self.population_walker, self.learners):
      w.state, w.over, w.ret = self.state.copy(), self.over.copy(), self.ret.copy()
      if w is not self.walker:
        w.frame = self.policy_frame

  def _frames(self, reached):
    """The rendered frames of reached states [..]: obs [.., L, H, W], board [.., H, W]."""
    shape = np.shape(reached)
    obs, board = wref.render(self.g, np.asarray(reached).reshape(-1))
    return obs.reshape(shape + obs.shape[1:]), board.reshape(shape + board.shape[1:])

  def _trace(self, reached):
    T, B = reached.shape
    return wref.trace(self.g, reached.reshape(-1)).reshape(-1, T, B)

  def _acts(self, salt, T, reset_first=False):
    """The action ids int8 [T, B] of an open-loop call: drawn from the salt, and - a table with an
    entry that ends the episode - half of them steered along the way there from where the model
    stands (a scout `Walker` walks ahead), so that episodes end under open-loop calls too.  The
    device is sent exactly these ('sent' in what the verbs return)."""
    acts = actions(salt, T, self.B)
    best = toward_done(self.g)
    if best is None:
      return acts
    steer = np.random.RandomState(salt + 7).rand(T, self.B) < 0.5
    scout = wref.Walker(self.g, self.B)
    scout.state, scout.over, scout.ret = self.state.copy(), self.over.copy() | bool(reset_first), self.ret.copy()
    for t in range(T):
      s = np.where(scout.over, 0, scout.state)
      acts[t] = np.where(steer[t], best[s], acts[t])
      scout.rollout(acts[t:t + 1])
    return acts

  def _open(self, acts, reset_first=False, stay_bad=False):
    """An open-loop call of the walker, frame counters included."""
    T = len(acts)
    sent = acts.copy()
    if stay_bad:                         # defect g: a frame with a bad id does not happen
      outs = []
      for t in range(T):
        before = (self.walker.state.copy(), self.walker.over.copy(), self.walker.ret.copy())
        if reset_first and t == 0:
          before[1][:] = True
        outs.append(self.walker.rollout(acts[t:t + 1], reset_first=reset_first and t == 0))
        wrong = (acts[t] < 0) | (acts[t] > 4)
        for now, was in zip((self.walker.state, self.walker.over, self.walker.ret), before):
          now[wrong] = was[wrong]
      want = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
    else:
      want = self.walker.rollout(acts, reset_first=reset_first)
    want['reached'] = want.pop('states')
    want['sent'] = sent
    self.frame = T if reset_first else self.frame + T
    if self.defect == 'a':
      self.policy_frame += T
    self._hand(self.walker)
    return want

  def _stream(self, want, obs=True, board=False):
    out = {k: want[k] for k in ('sent', 'reached', 'reward', 'discount', 'done', 'perf')}
    out['trace'] = self._trace(want['reached'])
    if self.render:
      frames = self._frames(want['reached'])
      if obs:
        out['obs'] = frames[0]
      if board:
        out['board'] = frames[1]
    return out

  # the start of a closed-loop call, with the defects that live there
  def _closed(self, walker, reset_first, call):
    was = self.over.copy() | bool(reset_first)
    old_ret = self.ret.copy()
    restart = reset_first
    if self.defect == 'c':               # reads `state`: the episode is not over, its return is
      walker.over[:] = False
      walker.ret = np.where(was, np.float32(0), walker.ret).astype(np.float32)
      restart = False
    want = call(restart)
    self.policy_frame = walker.frame
    T = want['T']
    self.frame = T if reset_first else self.frame + T
    if self.defect == 'd':
      walker.ret = np.where(was, (old_ret + walker.ret).astype(np.float32), walker.ret).astype(np.float32)
    if self.defect == 'e' and walker is self.learners:
      walker.over = was.copy()
    self._hand(walker)
    return want

  def run(self, op):
    self.log.append(op)
    return getattr(self, '_op_' + op['kind'])(op)

  def _op_play(self, op):
    want = self._open(self._acts(op['salt'], op['n']))
    return self._stream(want, board=True)

  def _op_rollout(self, op):
    want = self._open(self._acts(op['salt'], op['T'], op['reset_first']), op['reset_first'])
    return self._stream(want, board=op['form'] in ('board', 'last'))

  def _op_trace(self, op):
    want = self._open(self._acts(op['salt'], op['T'], op['reset_first']), op['reset_first'])
    out = self._stream(want, obs=False)
    t, e = pairs(op['pairs'], op['T'], self.B)
    out['frames'] = (self._frames(want['reached'][t, e])[0] if self.render else want['reached'][t, e])
    return out

  def _op_deferred(self, op):
    return {'call%d' % i: self._stream(self._open(self._acts(op['salt'] + i, op['T'])))
            for i in range(op['n'])}

  def _op_graph(self, op):
    n = op['n']
    if n not in self.captured:
      self.captured.add(n)
      if self.defect == 'f':             # two warm-up runs of n frames of action 0, left standing
        keep = self.frame
        self._open(np.zeros((2 * n, self.B), np.int8))
        self.frame = keep
    want = self._open(self._acts(op['salt'], n))
    out = self._stream(want, obs=False)
    if self.render:
      out['obs'], out['board'] = self._frames(want['reached'][-1])
    return out

  def _op_reset(self, op):
    self.walker.reset()
    self.frame = 0
    if self.defect == 'b':
      self.policy_frame = 0
    self._hand(self.walker)
    out = {'reached': np.zeros(self.B, np.int64)}
    if self.render:
      out['obs'], out['board'] = self._frames(out['reached'])
    return out

  def _sampled(self, want, g_states):
    """What a sampling walker returned, plus the trace of the states its frames reached."""
    after = self.g.st_next[g_states.astype(np.int64), want['actions'].astype(np.int64)]
    want['trace'] = self._trace(np.asarray(after, np.int64))
    return want

  def _op_policy(self, op, bad_rows=0):
    w = policy(self.g, op['salt'], bad_rows)
    T = op['T']

    def call(reset_first):
      want = self.policy_walker.rollout(w, T, seed=op['seed'], first_frame=op['first_frame'],
                                        reset_first=reset_first)
      want['T'] = T
      return want
    want = self._closed(self.policy_walker, op['reset_first'], call)
    return self._sampled(want, want['states'])

  def _op_population(self, op):
    w = population(self.g, op['salt'], op['P'])
    T = op['T']

    def call(reset_first):
      want = self.population_walker.rollout(w, T, seed=op['seed'], first_frame=op['first_frame'],
                                            reset_first=reset_first)
      want['T'] = T
      return want
    want = self._closed(self.population_walker, op['reset_first'], call)
    return self._sampled(want, want['states'] % self.g.n_states)

  def _op_learn(self, op):
    alpha, gamma, epsilon = hyper(self.B)
    T = op['T']

    def call(reset_first):
      want = self.learners.learn(T, alpha, gamma, epsilon, rule=op['rule'], seed=op['seed'],
                                 reset_first=reset_first, window=op['window'])
      want['T'] = T
      return want
    want = self._closed(self.learners, op['reset_first'], call)
    out = {k: want[k] for k in ('reward_sum', 'episodes', 'perf_sum')}
    out['q'] = self.learners.q.copy()
    return out

  def _op_bad(self, op):
    T, B = op['T'], self.B
    if op['what'] == 'rollout':
      acts = self._acts(op['salt'], T)
      at = np.random.RandomState(op['salt'] + 1).choice(T * B, size=min(op['k'], T * B), replace=False)
      acts.reshape(-1)[at] = 7
      before = self.walker.bad
      want = self._open(acts, stay_bad=self.defect == 'g')
      out = self._stream(want)
      out['count'] = self.walker.bad - before
      return out
    op = dict(op, first_frame=None, reset_first=True)
    if self.defect != 'g':
      out = self._op_policy(op, bad_rows=op['k'])
      out['count'] = out.pop('bad')
      return out
    # defect g: frame by frame, an environment that met a bad row put back where it was
    w = policy(self.g, op['salt'], op['k'])
    walker, outs, count = self.policy_walker, [], 0
    walker.over[:] = True
    for t in range(T):
      before = (walker.state.copy(), walker.over.copy(), walker.ret.copy())
      rows = np.where(walker.over, 0, walker.state)
      wrong = pref.thresholds(w[rows])[1]
      outs.append(walker.rollout(w, 1, seed=op['seed']))
      count += outs[-1]['bad']
      walker.state[wrong], walker.over[wrong] = before[0][wrong], before[1][wrong]
      walker.ret[wrong] = before[2][wrong]
    self.policy_frame = walker.frame
    self.frame = T
    self._hand(walker)
    want = {k: np.concatenate([o[k] for o in outs]) for k in outs[0] if k != 'bad'}
    want['count'] = count
    return self._sampled(want, want['states'])


def run_plan(name, seed, defect=None, render=False):
  """The whole case on the host: [(op, outputs, (state, over, ret, frame, policy_frame, q))]."""
  ops = plan(name, seed)
  m = SequenceModel(table(name), ops[0]['B'], q_salt=seed, render=render, defect=defect)
  steps = []
  for op in ops:
    began = (m.over.copy(), m.policy_frame)
    out = m.run(op)
    steps.append((op, out, (m.state.copy(), m.over.copy(), m.ret.copy(), m.frame, m.policy_frame,
                            m.q.copy()), began))
  return steps


# --------------------------------------------------------------------------- the one-cell tier

ONE_CELL_GAMES = ('boat_race', 'sokoban', 'wall_world')
ONE_CELL_KINDS = ('play', 'rollout', 'rollout-out', 'pipelined', 'deferred', 'deferred-shared',
                  'trace', 'graph', 'reset')
ONE_CELL_BATCHES = (7, 8, 64, 1000, 1002, 4096, 9000, 9008)        # tests/test_api_sequences.py's
# `trace` and `graph` each directly in front of a pipelined and of a deferred rollout, over two seeds
ONE_CELL_FORCED = ((('trace', 'pipelined'), ('graph', 'deferred')),
                   (('trace', 'deferred-shared'), ('graph', 'pipelined')))


def one_cell_plan(name, seed):
  """(14 kinds, batch, salt of the case's actions) of the one-cell test: a pure function too."""
  rng = np.random.RandomState(1000 * seed + 7 * len(name) + 3)
  B = int(rng.choice(ONE_CELL_BATCHES))
  blocks = [list(pair) for pair in (ONE_CELL_FORCED[seed] if seed < len(ONE_CELL_FORCED) else ())]
  n_rest = N_OPS - sum(len(b) for b in blocks)
  kinds = [[k] for k in rng.choice(ONE_CELL_KINDS, size=n_rest)]
  for block in blocks:
    kinds.insert(int(rng.randint(1, len(kinds) + 1)), block)        # (not first: in mid-sequence)
  return [k for group in kinds for k in group], B, int(rng.randint(1 << 30))
