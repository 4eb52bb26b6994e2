"""Random SEQUENCES across the stateful calls of the state-table tier - play(), rollout(),
rollout_trace() / render_frames(), rollout_deferred() / flush(), rollout_policy(),
rollout_population(), learn_tabular(), a capture_play() replay, reset(), and calls with bad ids or
bad policy rows - against tests/sequence_model.py, which runs the same plan through the four numpy
references.  After EVERY operation `state`, `done`, `ret`, `frame`, `_policy_frame`, the learners'
`q` and every tensor the call returned are compared, integers by value and floats by bits: the
hand-off between the six kernels is what is tested, each family alone is pinned elsewhere.
tests/test_sequence_model_cpu.py shows what these sequences can see.

Second test: the one-cell tier with rollout_trace() / render_frames(), a graph replay and reset()
among play(), rollout(), pipelined and deferred rollouts, against the C oracle, as
tests/test_api_sequences.py runs the older calls.
"""

import os
import re
import types

import numpy as np
import pytest
import torch

import sequence_model as sm
import wide_table_reference as wref
from test_policy_rollout import _game, _same

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get('CAMPX_SEQ_SEEDS', str(sm.DEFAULT_SEEDS)))
STREAMS = ('reward', 'discount', 'done', 'perf')


def _np(x):
  if torch.is_tensor(x):
    if x.dtype in (torch.float16, torch.bfloat16):
      return x.contiguous().view(torch.int16).cpu().numpy()
    return x.cpu().numpy()
  return np.asarray(x)


def _eq(got, want, what):
  """Integers by value, floats by bits, shapes alike."""
  got, want = _np(got), np.asarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  if want.dtype == np.float32:
    assert got.dtype == np.float32 and _same(got, want), what
  else:
    assert got.dtype.kind in 'iub' and np.array_equal(got.astype(np.int64), want.astype(np.int64)), what


def _fused(name, B):
  from campx_amd import wide
  g = sm.table(name)
  if name in sm.SYNTHETIC:
    f = wide.WideGame(types.SimpleNamespace(rows=g.rows, cols=g.cols), B, 'cuda', g)
    f.showtime()
    return f, f
  game = _game(name, B)
  f = game.fused
  for k in ('st_next', 'st_done', 'st_reached'):          # the table the CPU conditions were shown on
    assert np.array_equal(np.asarray(getattr(f.traced, k)), np.asarray(getattr(g, k))), k
  assert _same(np.asarray(f.traced.st_reward, np.float32), np.asarray(g.st_reward, np.float32))
  return f, game


class _Device(object):
  """The operations of a plan on a `WideGame`: `run(op, want)` issues the calls, with the actions
  the model sent, and compares all they return with `want`."""

  def __init__(self, name, f, g, log):
    self.name, self.f, self.g, self.log = name, f, g, log
    self.synthetic = name in sm.SYNTHETIC
    B = f.batch
    self.kept, self.kept_closed, self.graphs = {}, {}, {}
    self.q = None
    self.hyper = [torch.from_numpy(x).cuda() for x in sm.hyper(B)]

  def eq(self, got, want, what):
    _eq(got, want, (self.log, what))

  def stream(self, out, want, what, keys=STREAMS + ('trace',)):
    for k in keys:
      if k == 'trace':
        assert out['trace'].dtype == torch.int16
        if self.synthetic:
          self.eq(out['trace'].view(torch.int16).cpu().numpy().view(np.uint16), want['trace'], (what, k))
      elif out.get(k) is None:
        assert k == 'perf' and not self.f.has_perf, (self.log, what, k)
      else:
        self.eq(out[k], want[k], (what, k))

  def run(self, op, want):
    getattr(self, 'op_' + op['kind'])(op, want)
    torch.cuda.synchronize()

  def op_play(self, op, want):
    f = self.f
    for t in range(op['n']):
      obs, reward, discount = f.play(torch.from_numpy(want['sent'][t]).cuda())
      self.eq(obs.layered_board, want['obs'][t], ('play obs', t))
      self.eq(obs.board, want['board'][t], ('play board', t))
      self.eq(reward, want['reward'][t], ('play reward', t))
      self.eq(discount, want['discount'][t], ('play discount', t))
      self.eq(f._step_done, want['done'][t], ('play done', t))

  def op_rollout(self, op, want):
    f, T, form = self.f, op['T'], op['form']
    ids = torch.from_numpy(want['sent']).cuda()
    kw = dict(reset_first=op['reset_first'])
    if form == 'board':
      kw['want_board'] = True
    elif form == 'last':
      kw.update(keep_obs=False, want_board=True)
    elif form in ('f16', 'bf16'):
      kw['obs_dtype'] = torch.float16 if form == 'f16' else torch.bfloat16
    elif form == 'out':
      if T not in self.kept:
        self.kept[T] = f.rollout_buffers(T)
      kw['out'] = self.kept[T]
    out = f.rollout(ids, **kw)
    self.stream(out, want, form)
    if form == 'last':
      assert out['obs'] is f._obs and out['board'] is f._board
      self.eq(out['obs'], want['obs'][-1], 'last obs')
      self.eq(out['board'], want['board'][-1], 'last board')
    elif form in ('f16', 'bf16'):
      assert out['obs'].dtype == kw['obs_dtype']
      self.eq(out['obs'], wref.as_bits16(want['obs'], wref.F16_ONE if form == 'f16' else wref.BF16_ONE), form)
    else:
      assert form != 'out' or out is self.kept[T]
      self.eq(out['obs'], want['obs'], 'obs')
      if form == 'board':
        self.eq(out['board'], want['board'], 'board')

  def op_trace(self, op, want):
    f = self.f
    out = f.rollout_trace(torch.from_numpy(want['sent']).cuda(), reset_first=op['reset_first'])
    assert 'obs' not in out
    self.stream(out, want, 'rollout_trace')
    t, e = sm.pairs(op['pairs'], op['T'], f.batch)
    frames = f.render_frames(out['trace'], torch.from_numpy(t).cuda(), torch.from_numpy(e).cuda())
    self.eq(frames, want['frames'], 'render_frames')

  def op_deferred(self, op, want):
    f, T, n = self.f, op['T'], op['n']
    bufs = [f.rollout_buffers(T), f.rollout_buffers(T)]
    for i in range(n):
      w = want['call%d' % i]
      prev = f.rollout_deferred(torch.from_numpy(w['sent']).cuda(), bufs[i & 1])
      assert (prev is None) == (i == 0), self.log
      self.stream(bufs[i & 1], w, ('deferred', i))
      if prev is not None:
        assert prev is bufs[(i - 1) & 1]
        self.eq(prev['obs'], want['call%d' % (i - 1)]['obs'], ('deferred obs', i - 1))
    last = f.flush()
    assert last is bufs[(n - 1) & 1] and f.flush() is None
    self.eq(last['obs'], want['call%d' % (n - 1)]['obs'], 'flush obs')
    self.stream(last, want['call%d' % (n - 1)], 'flush')

  def closed(self, out, want, op, what):
    self.stream(out, want, what)
    self.eq(out['actions'], want['actions'], (what, 'actions'))
    if op['want_states']:
      assert out['states'].dtype == torch.int32
      self.eq(out['states'], want['states'], (what, 'states'))

  def closed_out(self, op):
    if not op['reuse_out']:
      return None
    key = (op['T'], op['want_states'])
    if key not in self.kept_closed:
      self.kept_closed[key] = self.f.rollout_policy_buffers(*key)
    return self.kept_closed[key]

  def op_policy(self, op, want):
    w = torch.from_numpy(sm.policy(self.g, op['salt'])).cuda()
    bufs = self.closed_out(op)
    out = self.f.rollout_policy(w, op['T'], seed=op['seed'], first_frame=op['first_frame'],
                                reset_first=op['reset_first'], out=bufs, want_states=op['want_states'])
    assert bufs is None or out is bufs
    assert op['want_states'] or bufs is not None or 'states' not in out
    self.closed(out, want, op, 'rollout_policy')

  def op_population(self, op, want):
    w = torch.from_numpy(sm.population(self.g, op['salt'], op['P'])).cuda()
    bufs = self.closed_out(op)
    out = self.f.rollout_population(w, op['T'], seed=op['seed'], first_frame=op['first_frame'],
                                    reset_first=op['reset_first'], out=bufs,
                                    want_states=op['want_states'], path=op['path'])
    assert bufs is None or out is bufs
    self.closed(out, want, op, 'rollout_population')          # ('states': member * n_states + state)

  def op_learn(self, op, want):
    f = self.f
    alpha, gamma, epsilon = self.hyper
    res = f.learn_tabular(op['T'], self.q, alpha, gamma, epsilon, rule=op['rule'], seed=op['seed'],
                          reset_first=op['reset_first'], window=op['window'], path=op['path'])
    assert res['q'] is self.q
    self.eq(res['reward_sum'], want['reward_sum'], 'reward_sum')
    self.eq(res['episodes'], want['episodes'], 'episodes')
    if f.has_perf:
      self.eq(res['perf_sum'], want['perf_sum'], 'perf_sum')
    else:
      assert 'perf_sum' not in res and not want['perf_sum'].any()

  def op_graph(self, op, want):
    f, n = self.f, op['n']
    if n not in self.graphs:               # captured here, in the middle of the sequence
      frame = f.frame
      self.graphs[n] = f.capture_play(n)
      assert f.frame == frame
    graph = self.graphs[n].replay(torch.from_numpy(want['sent']).cuda())
    torch.cuda.synchronize()
    self.stream(dict(reward=graph.reward, discount=graph.discount, done=graph.done, perf=graph.perf),
                want, 'graph', keys=STREAMS)
    self.eq(graph.observation.layered_board, want['obs'], 'graph observation')
    self.eq(graph.observation.board, want['board'], 'graph board')

  def op_reset(self, op, want):
    first, reward, discount = self.f.reset()
    assert reward is None and discount == 1.0
    self.eq(first.layered_board, want['obs'], 'reset obs')
    self.eq(first.board, want['board'], 'reset board')

  def op_bad(self, op, want):
    f, T = self.f, op['T']
    assert f.validate_actions is True
    if op['what'] == 'rollout':
      bufs, words = f.rollout_buffers(T), r'^(\d+) action ids are outside 0\.\.4'
      with pytest.raises(ValueError) as caught:   # (from the call itself if the flag is up as it returns)
        f.rollout(torch.from_numpy(want['sent']).cuda(), out=bufs)
        f.check_actions()
    else:
      bufs = f.rollout_policy_buffers(T)
      words = r'^(\d+) environment-frames of rollout_policy\(\) met bad policy rows'
      w = torch.from_numpy(sm.policy(self.g, op['salt'], op['k'])).cuda()
      with pytest.raises(ValueError) as caught:
        f.rollout_policy(w, T, seed=op['seed'], reset_first=True, out=bufs)
        f.check_actions()
    found = re.match(words, str(caught.value))
    assert found and int(found.group(1)) == want['count'] > 0, (self.log, str(caught.value), want['count'])
    # ... and nothing else was counted (the message about policy rows has a ';' of its own)
    assert str(caught.value).count(';') == (op['what'] == 'policy'), (self.log, str(caught.value))
    f.check_actions()                      # ... and the counters were cleared
    self.stream(bufs, want, 'bad')
    if op['what'] == 'rollout':
      self.eq(bufs['obs'], want['obs'], 'bad obs')
    else:
      self.eq(bufs['actions'], want['actions'], 'bad actions')
      self.eq(bufs['states'], want['states'], 'bad states')


def _run_case(name, ops, q_salt):
  B = ops[0]['B']
  f, keep = _fused(name, B)
  g = sm.table(name)
  m = sm.SequenceModel(g, B, q_salt=q_salt)
  log = []
  dev = _Device(name, f, g, log)
  dev.q = torch.from_numpy(m.q.copy()).cuda()
  for op in ops:
    log.append(op)
    want = m.run(op)
    dev.run(op, want)
    _eq(f.state, m.state, (log, 'state'))
    _eq(f.done, m.over, (log, 'done'))
    _eq(f.ret, m.ret, (log, 'ret'))
    assert f.frame == m.frame, (log, 'frame', f.frame, m.frame)
    assert f._policy_frame == m.policy_frame, (log, '_policy_frame', f._policy_frame, m.policy_frame)
    _eq(dev.q, m.q, (log, 'q'))
  f.check_actions()
  del keep
  return log


@pytest.mark.parametrize('seed', range(SEEDS))
@pytest.mark.parametrize('name', sm.GAMES)
def test_a_sequence_across_the_families_matches_the_model(name, seed):
  ops = sm.plan(name, seed)
  assert len(_run_case(name, ops, seed)) == sm.N_OPS


# --------------------------------------------------------------------------- the one-cell tier

ONE_CELL_SEEDS = int(os.environ.get('CAMPX_SEQ_SEEDS', '2'))


@pytest.mark.parametrize('seed', range(ONE_CELL_SEEDS))
@pytest.mark.parametrize('name', sm.ONE_CELL_GAMES)
def test_one_cell_sequences_with_the_trace_calls_in_the_loop(name, seed):
  from campx_amd import gamespec
  from campx_amd.games import boat_race, sokoban, wall_world
  from oracle import cpu
  from test_api_sequences import _same as same
  build = dict(boat_race=boat_race.build, sokoban=sokoban.build, wall_world=wall_world.build)[name]
  kinds, B, salt = sm.one_cell_plan(name, seed)
  rng = np.random.RandomState(salt)
  game = build(batch=B, device='cuda')
  first, _, _ = game.its_showtime()
  f = game.fused
  assert type(f).__name__ == 'FusedGame'
  og = cpu.OracleGame.from_description(gamespec.describe(build()))
  obs0, board0 = og.first_frame()
  assert np.array_equal(first.layered_board.cpu().numpy()[0], obs0.astype(np.int8))
  log, kept, graphs = [], {}, {}
  carried = dict(ret=np.zeros(B, np.float32), over=np.ones(B, bool), reset=False)

  def acts(T):
    return rng.randint(0, 5, size=(T, B)).astype(np.int8)

  def oracle(a):
    """The oracle fed the same actions, the returns it implies carried along; the first call after
    a reset() rebuilds every environment."""
    ref = og.rollout(a, reset_first=carried['reset'])
    if carried['reset']:
      carried['over'][:] = True
    carried['reset'] = False
    for t in range(len(a)):
      r = np.where(np.isnan(ref['reward'][t]), np.float32(0), ref['reward'][t]).astype(np.float32)
      carried['ret'] = (np.where(carried['over'], np.float32(0), carried['ret']) + r).astype(np.float32)
      carried['over'] = ref['done'][t] != 0
    return ref

  def scalars(out, ref, what):
    if out.get('perf') is not None and ref.get('perf') is not None:
      assert same(out['perf'].cpu().numpy(), ref['perf']), (log, what, 'perf')
    for k in ('reward', 'discount', 'done'):
      if out[k] is None:
        assert k == 'reward' and not f.any_reward
      else:
        assert same(out[k].cpu().numpy(), ref[k]), (log, what, k)

  def check(out, ref, what):
    assert same(out['obs'].cpu().numpy(), ref['obs']), (log, what, 'obs')
    scalars(out, ref, what)

  def played(a, what):
    obs, reward, discount = game.play(torch.from_numpy(a[0]))
    ref = oracle(a)
    assert same(obs.layered_board.cpu().numpy(), ref['obs'][0]), (log, what)
    assert same(obs.board.cpu().numpy(), ref['board'][0]), (log, what)
    assert reward is None or same(reward.cpu().numpy(), ref['reward'][0]), (log, what)
    assert same(discount.cpu().numpy(), ref['discount'][0]), (log, what)

  for kind in kinds:
    T = int(rng.choice([1, 5, 16, 23, 40]))
    log.append((kind, T))
    frame = f.frame
    if kind == 'play':
      n = int(rng.randint(1, 4))
      for _ in range(n):
        played(acts(1), 'play')
      T = n
    elif kind == 'rollout':
      a = acts(T)
      check(game.rollout(torch.from_numpy(a).cuda()), oracle(a), 'rollout')
    elif kind == 'rollout-out':
      a = acts(T)
      out = kept.setdefault(T, game.rollout_buffers(T))
      assert game.rollout(torch.from_numpy(a).cuda(), out=out) is out
      check(out, oracle(a), 'rollout out=')
    elif kind == 'pipelined':
      bufs = [f.rollout_buffers(T), f.rollout_buffers(T)]
      refs = []
      for i in range(3):
        a = acts(T)
        f.rollout(torch.from_numpy(a).cuda(), out=bufs[i & 1], pipelined=True)
        refs.append(oracle(a))
        if i >= 1:
          check(bufs[(i - 1) & 1], refs[i - 1], ('pipelined', i - 1))
      torch.cuda.synchronize()
      check(bufs[0], refs[2], 'pipelined last')
      T = 3 * T
    elif kind in ('deferred', 'deferred-shared'):
      one = game.rollout_buffers(T)
      bufs = [one, game.rollout_buffers(T, share=one) if kind == 'deferred-shared' else game.rollout_buffers(T)]
      refs = []
      n = int(rng.randint(1, 5))
      for i in range(n):
        a = acts(T)
        prev = game.rollout_deferred(torch.from_numpy(a).cuda(), bufs[i & 1])
        refs.append(oracle(a))
        assert (prev is None) == (i == 0), log
        scalars(bufs[i & 1], refs[i], ('deferred scalars', i))
        if prev is not None:
          assert prev is bufs[(i - 1) & 1]
          check(prev, refs[i - 1], ('deferred', i - 1))
      T = n * T
      if rng.rand() < 0.5:
        check(game.flush(), refs[-1], 'flush')
      else:                                # not flushed: a play() first, the owed frames after it
        played(acts(1), 'play after deferred')
        check(game.flush(), refs[-1], 'late flush')
        T += 1
    elif kind == 'trace':
      a = acts(T)
      out = f.rollout_trace(torch.from_numpy(a).cuda())
      ref = oracle(a)
      scalars(out, ref, 'rollout_trace')
      t, e = sm.pairs(int(rng.randint(1 << 30)), T, B)
      frames = f.render_frames(out['trace'], torch.from_numpy(t).cuda(), torch.from_numpy(e).cuda())
      assert same(frames.cpu().numpy(), ref['obs'][t, e]), (log, 'render_frames')
    elif kind == 'graph':
      T = 4
      if 4 not in graphs:
        graphs[4] = game.capture_play(4)
        assert f.frame == frame
      a = acts(4)
      graph = graphs[4].replay(torch.from_numpy(a).cuda())
      torch.cuda.synchronize()
      ref = oracle(a)
      scalars(dict(reward=graph.reward, discount=graph.discount, done=graph.done, perf=graph.perf), ref, 'graph')
      assert same(graph.observation.layered_board.cpu().numpy(), ref['obs'][-1]), (log, 'graph observation')
      assert same(graph.observation.board.cpu().numpy(), ref['board'][-1]), (log, 'graph board')
    else:
      assert kind == 'reset'
      shown, reward, discount = f.reset()
      assert reward is None and discount == 1.0
      assert same(shown.layered_board.cpu().numpy(), np.broadcast_to(obs0, (B,) + obs0.shape)), (log, 'reset')
      assert same(shown.board.cpu().numpy(), np.broadcast_to(board0, (B,) + board0.shape)), (log, 'reset')
      carried['reset'] = True
      frame, T = 0, 0
    torch.cuda.synchronize()
    assert f.frame == frame + T, (log, 'frame')
    if not carried['reset']:
      assert same(f.ret.cpu().numpy(), carried['ret']), (log, 'episode returns')
      assert np.array_equal(f.done.cpu().numpy() != 0, carried['over']), (log, 'game-over flags')
  f.check_actions()
