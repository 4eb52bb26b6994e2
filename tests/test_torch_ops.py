"""The torch custom-op boundary (csrc/campx_torch.cpp): registration, schemas, loud
failure without a HIP device (CPU part); behaviour through the ops, opcheck and
torch.compile on the GPU (gpu part)."""

import ctypes

import numpy as np
import pytest
import torch

from campx_amd import _hip, gamespec
from campx_amd.games import boat_race


def _spec_tensor():
  spec = gamespec.lower(gamespec.describe(boat_race.build()))
  return torch.frombuffer(bytearray(gamespec.spec_bytes(spec)), dtype=torch.uint8)


def test_ops_are_registered_with_mutable_schemas():
  for name in _hip.OP_NAMES:
    op = getattr(torch.ops.campx, name).default
    assert op._schema.returns == []            # everything is written in place
  s = str(torch.ops.campx.rollout.default._schema)
  for written in ('Tensor(a!) pos', 'Tensor(b!) done', 'Tensor(d!) obs', 'Tensor(f!)? reward',
                  'Tensor(j!)? trace', 'bool reset_first'):
    assert written in s, s
  s = str(torch.ops.campx.step.default._schema)
  assert 'Tensor actions' in s and 'Tensor(k!)? bad_flag' in s


def test_no_cpu_kernel_so_cpu_tensors_fail_loudly():
  spec = _spec_tensor()
  B = 8
  pos = torch.zeros((2, B), dtype=torch.int8)
  done = torch.zeros((B,), dtype=torch.uint8)
  obs = torch.zeros((B, 7, 5, 5), dtype=torch.int8)
  acts = torch.zeros((B,), dtype=torch.int8)
  with pytest.raises((NotImplementedError, RuntimeError)) as e:
    torch.ops.campx.step(spec, spec, pos, done, None, None, acts, obs, None, None, None,
                         None, None, None, None)
  assert 'CPU' in str(e.value)
  with pytest.raises((NotImplementedError, RuntimeError)):
    torch.ops.campx.reset(spec, spec, pos, done, None, None, obs, None)


def test_meta_kernels_trace_without_a_device():
  """The Meta registration is the fake-tensor implementation: tracing needs no GPU."""
  spec = _spec_tensor().to('meta')
  B = 8
  pos = torch.zeros((2, B), dtype=torch.int8, device='meta')
  done = torch.zeros((B,), dtype=torch.uint8, device='meta')
  obs = torch.zeros((3, B, 7, 5, 5), dtype=torch.int8, device='meta')
  acts = torch.zeros((3, B), dtype=torch.int8, device='meta')
  assert torch.ops.campx.rollout(spec, spec, pos, done, None, None, acts, obs, None, None,
                                 None, None, None, None, None, None, True) is None



def _registered_ops():
  """The ops of the campx namespace, read from torch's registry."""
  return {s.name.split('::', 1)[1] for s in torch._C._jit_get_all_schemas()
          if s.name.startswith('campx::')}


def test_op_names_are_the_registered_ops():
  assert len(set(_hip.OP_NAMES)) == len(_hip.OP_NAMES)
  assert set(_hip.OP_NAMES) == _registered_ops()
  assert 'update_render' in _hip.OP_NAMES


def _meta_argument(kind):
  return {'Tensor': torch.zeros((2,), dtype=torch.int8, device='meta'), 'Optional[Tensor]': None,
          'List[Tensor]': [], 'int': 0, 'float': 0.0, 'bool': False}[kind]


@pytest.mark.parametrize('name', _hip.OP_NAMES)
def test_every_meta_kernel_takes_the_schema_s_arguments_and_returns_nothing(name):
  """The Meta registration of EVERY op, with arguments made from its schema alone."""
  op = getattr(torch.ops.campx, name).default
  args = [_meta_argument(str(a.type)) for a in op._schema.arguments]
  assert any(torch.is_tensor(a) for a in args)
  assert op(*args) is None


# ----------------------------------------------------------------------- GPU

def _game(batch=256):
  game = boat_race.build(batch=batch, device='cuda')
  game.its_showtime()
  return game


@pytest.mark.gpu
def test_play_and_rollout_go_through_the_ops(golden, monkeypatch):
  gold = golden('boat_race')
  T, N = gold['actions'].shape
  game = _game(N)
  calls = []
  real_step, real_rollout = game.fused._step, game.fused._rollout
  monkeypatch.setattr(game.fused, '_step', lambda *a: (calls.append('step'), real_step(*a))[1])
  monkeypatch.setattr(game.fused, '_rollout',
                      lambda *a: (calls.append('rollout'), real_rollout(*a))[1])
  obs, reward, discount = game.play(torch.from_numpy(gold['actions'][0]))
  assert np.array_equal(obs.layered_board.cpu().numpy(), gold['layered'][1])
  out = game.rollout(torch.from_numpy(gold['actions'][1:]))
  assert np.array_equal(out['obs'].cpu().numpy(), gold['layered'][2:])
  assert calls == ['step', 'rollout']


@pytest.mark.gpu
def test_ops_run_on_the_current_stream():
  """Work is enqueued on torch's current stream: a rollout issued on a side stream is
  ordered after what that stream already holds, with no synchronisation in the op."""
  game = _game(4096)
  acts = torch.randint(0, 5, (30, 4096), dtype=torch.int8, device='cuda')
  want = game.rollout(acts, reset_first=True)
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  bufs = game.fused.rollout_buffers(30)
  with torch.cuda.stream(side):
    torch.cuda._sleep(20_000_000)              # ~10 ms of work ahead of the op on `side`
    got = game.rollout(acts, out=bufs, reset_first=True)
    done_early = side.query()
  side.synchronize()
  assert not done_early
  assert torch.equal(got['obs'], want['obs']) and torch.equal(got['reward'], want['reward'])


@pytest.mark.gpu
def test_opcheck():
  game = _game(128)
  f = game.fused
  acts = torch.randint(0, 5, (128,), dtype=torch.int8, device='cuda')
  args = (f._spec_host, f._spec_dev, f.pos, f.done, f.ret, None, acts, f._obs, f._board,
          f._reward, f._discount, f._step_done, f.perf, f._bad, None)
  torch.library.opcheck(torch.ops.campx.step.default, args)      # all four checks
  acts = torch.randint(0, 5, (5, 128), dtype=torch.int8, device='cuda')
  b = f.rollout_buffers(5, want_board=True)
  args = (f._spec_host, f._spec_dev, f.pos, f.done, f.ret, None, acts, b['obs'], b['board'],
          b['reward'], b['discount'], b['done'], b['perf'], b['trace'], f._bad, None, True)
  torch.library.opcheck(torch.ops.campx.rollout.default, args)


@pytest.mark.gpu
def test_torch_compile_traces_through_the_op_without_a_graph_break(golden):
  """A policy-in-the-loop step - observation -> action ids -> campx::step - compiles as
  ONE graph (fullgraph=True raises on any graph break) and matches eager."""
  game_c, game_e = _game(512), _game(512)
  w = torch.randn(7 * 25, 5, device='cuda')

  def loop(f, steps):
    total = torch.zeros((), device='cuda')
    for _ in range(steps):
      logits = f._obs.view(f.batch, -1).float() @ w
      ids = logits.argmax(dim=1).to(torch.int8)
      torch.ops.campx.step(f._spec_host, f._spec_dev, f.pos, f.done, f.ret, None, ids,
                           f._obs, f._board, f._reward, f._discount, f._step_done, f.perf,
                           None, None)
      total = total + f._reward.sum()
    return total

  compiled = torch.compile(loop, fullgraph=True, backend='aot_eager')
  a = compiled(game_c.fused, 3)
  b = loop(game_e.fused, 3)
  torch.cuda.synchronize()
  assert torch.equal(a, b)
  assert torch.equal(game_c.fused._obs, game_e.fused._obs)
  assert torch.equal(game_c.fused.pos, game_e.fused.pos)


@pytest.mark.gpu
def test_play_is_capturable_in_a_hip_graph():
  """campx::step only enqueues kernels on the current stream (no allocation, no
  synchronisation), so a policy-in-the-loop stretch of play() calls can be captured in a
  HIP graph and replayed: one graph launch for many frames."""
  game_g, game_e = _game(1024), _game(1024)
  for g in (game_g, game_e):
    g.fused.validate_actions = False
  w = torch.randn(7 * 25, 5, device='cuda')

  def frames(game, n):
    f = game.fused
    for _ in range(n):
      ids = (f._obs.view(f.batch, -1).float() @ w).argmax(dim=1).to(torch.int8)
      game.play(ids)

  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    frames(game_g, 2)                          # warm up allocations outside the capture
  torch.cuda.current_stream().wait_stream(side)
  frames(game_e, 2)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    frames(game_g, 6)
  for _ in range(3):
    graph.replay()
  frames(game_e, 18)
  torch.cuda.synchronize()
  assert torch.equal(game_g.fused._obs, game_e.fused._obs)
  assert torch.equal(game_g.fused.pos, game_e.fused.pos)
  assert torch.equal(game_g.fused.ret, game_e.fused.ret)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['boat_race', 'sokoban', 'wall_world', 'sokoban_l2'])
def test_pipelined_rollouts_match_in_order_rollouts(name):
  """Update pass on a side stream, overlapping the previous launch's render: same bits."""
  import sys, os
  sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
  from games_under_test import FUSED_GAMES
  if True:
    B, T = 4096, 40
    a = FUSED_GAMES[name](batch=B, device='cuda'); a.its_showtime()
    b = FUSED_GAMES[name](batch=B, device='cuda'); b.its_showtime()
    gen = torch.Generator().manual_seed(3)
    acts = [torch.randint(0, 5, (T, B), generator=gen, dtype=torch.int8).cuda() for _ in range(5)]
    torch.cuda.synchronize()
    bufs = [b.fused.rollout_buffers(T)]
    bufs.append(b.fused.rollout_buffers(T, share=bufs[0]))
    for i, x in enumerate(acts):
      want = a.rollout(x, reset_first=(i % 2 == 0))
      got = b.rollout(x, out=bufs[i & 1], reset_first=(i % 2 == 0), pipelined=True)
      for k in ('obs', 'reward', 'discount', 'done', 'perf', 'trace'):
        if want[k] is not None:
          assert torch.equal(want[k], got[k]), (i, k)
      if i == 2:                                 # an in-order call in between
        o1, r1, _ = a.play(x[0]); o2, r2, _ = b.play(x[0])
        assert torch.equal(o1.layered_board, o2.layered_board) and torch.equal(r1, r2)
    assert torch.equal(a.fused.pos, b.fused.pos) and torch.equal(a.fused.ret, b.fused.ret)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['boat_race', 'sokoban'])
def test_pipelined_rollouts_do_not_overwrite_a_trace_still_being_rendered(name):
  """Six pipelined calls with different actions, two alternating buffer sets with their own
  observation buffers, ONE synchronisation at the end: the side stream must not start the
  update pass of call i + 2 before the render of call i has read the trace they share.
  Long renders (T = 100 at B = 65 536) against update passes a tenth as long make the
  overrun certain without that ordering."""
  import sys, os
  sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
  from games_under_test import FUSED_GAMES
  B, T, N = 65536, 100, 6
  a = FUSED_GAMES[name](batch=B, device='cuda'); a.its_showtime()
  b = FUSED_GAMES[name](batch=B, device='cuda'); b.its_showtime()
  gen = torch.Generator().manual_seed(11)
  acts = [torch.randint(0, 5, (T, B), generator=gen, dtype=torch.int8).cuda() for _ in range(N)]
  # what each call must show at a sample of frames, from in-order rollouts
  frames = [0, T // 2, T - 1]
  want = []
  for i, x in enumerate(acts):
    out = a.rollout(x, reset_first=(i == 0))
    want.append([out['obs'][f].clone() for f in frames])
  torch.cuda.synchronize()
  bufs = [b.fused.rollout_buffers(T), b.fused.rollout_buffers(T)]
  kept = []
  for i, x in enumerate(acts):
    got = b.rollout(x, out=bufs[i & 1], reset_first=(i == 0), pipelined=True)
    # keep the sampled frames by a copy queued on the main stream (ordered after the render)
    kept.append([got['obs'][f].clone() for f in frames])
  torch.cuda.synchronize()
  for i in range(N):
    for j, f in enumerate(frames):
      assert torch.equal(kept[i][j], want[i][j]), (i, f)
  assert torch.equal(a.fused.pos, b.fused.pos)


# ------------------------------------------------- arguments the ops refuse (GPU, no launches)
#
# Every case spoils ONE argument of a valid call and names a piece of the message the op must
# raise - before anything is launched: the state is untouched afterwards, and the valid call,
# made once at the end, gives what the engine's own rollout() / play() give a twin game.
# B = 5: rollout_buffers() pads the rows to a pitch of 16, so pitch and batch size differ.
# The boat race and the smallest maze of tests/test_wide_parity.py have ONE trace plane; what
# only the planes of a trace can tell - the pitch of a one-frame call, how far apart the planes
# are - is refused for a game of two (sokoban), and is not a fault of a one-plane trace at all.

_B = 5


def _same(a, b):
  a, b = a.contiguous(), b.contiguous()
  if a.dtype == torch.float32 and b.dtype == torch.float32:
    a, b = a.view(torch.int32), b.view(torch.int32)          # NaN (reward None) included
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _padded(like, *shape):
  """A [..., B] view of a fresh array whose rows are `shape[-1]` apart."""
  return like.new_empty(shape)[..., :_B]


def _more_planes(v, T):
  t = v['trace']
  return _padded(t, t.shape[0] + 1, t.shape[1], 16)


# fault -> (the spoiled argument(s) from the valid ones `v` and the frame count, the message)
_FAULTS = {
    'spec_host short': (lambda v, T: dict(spec_host=v['spec_host'][:-1]), 'spec_host must be'),
    'spec_dev short': (lambda v, T: dict(spec_dev=v['spec_dev'][:-1]),
                       'spec_dev must be the CampxSpec blob'),
    'tables short': (lambda v, T: dict(tables=v['tables'][:-1]),
                     'tables must be the campx_wide_tables_build() blob'),
    'pos int32': (lambda v, T: dict(pos=v['pos'].to(torch.int32)), 'pos must be'),
    'state int64': (lambda v, T: dict(state=v['state'].long()), 'state must be'),
    'done short': (lambda v, T: dict(done=v['done'][:-1]), 'done must have shape'),
    'reward pitch': (lambda v, T: dict(reward=_padded(v['reward'], T, 32)), 'same pitch'),
    'reward stride 2': (lambda v, T: dict(reward=v['reward'].new_empty((T, 16, 2))[:, :_B, 0]),
                        'contiguous within a row'),
    'reward bare row': (lambda v, T: dict(reward=v['reward'].new_empty((1, _B))), 'must reach'),
    'trace planes apart': (lambda v, T: dict(trace=_padded(v['trace'], v['trace'].shape[0], T + 1,
                                                           16)[:, :T]), 'planes'),
    'trace uint8': (lambda v, T: dict(trace=v['trace'].to(torch.uint8)), 'int16'),
    'trace plane count': (lambda v, T: dict(trace=_more_planes(v, T)), 'trace must be'),
    'bad_flag unpinned': (lambda v, T: dict(bad_flag=torch.zeros((1,), dtype=torch.int32)),
                          'pinned host memory'),
    'bad_count two': (lambda v, T: dict(bad_count=torch.zeros((2,), dtype=torch.int32,
                                                              device='cuda')),
                      'bad_count must have shape'),
    'obs float32': (lambda v, T: dict(obs=v['obs'].float()), 'obs must be int8, float16 or bfloat16'),
    'prev_obs float32': (lambda v, T: dict(prev_obs=v['prev_obs'].float()),
                         'obs must be int8, float16 or bfloat16'),
    'board of the last frame': (lambda v, T: dict(board=v['board'][0].clone()),
                                'both keep every frame or both the last'),
    'prev_trace is trace': (lambda v, T: dict(prev_trace=v['trace']), 'a trace buffer each'),
    'source 3': (lambda v, T: dict(source=3), 'source must be 0, 1 or 2'),
    'pairs without t_idx': (lambda v, T: dict(t_idx=None), 'need t_idx and e_idx'),
    'path 3': (lambda v, T: dict(path=3), 'path must be'),
    'counts int64': (lambda v, T: dict(counts=v['counts'].long()), 'counts must be'),
}


def _applies(fault, T, planes):
  if fault == 'reward pitch':            # one row has no pitch of its own
    return T > 1
  if fault == 'reward bare row':         # one frame: only the planes of the trace tell the pitch
    return T == 1 and planes > 1
  if fault == 'trace planes apart':
    return T > 1 and planes > 1
  return True


_STATE = ['spec_host short', 'pos int32', 'done short']
_WIDE_STATE = ['spec_host short', 'tables short', 'state int64', 'done short']
_STREAMS = ['reward pitch', 'reward stride 2', 'reward bare row']
_COUNTED = ['bad_flag unpinned', 'bad_count two']
_OP_FAULTS = {
    'step': _STATE + _COUNTED + ['obs float32'],
    'rollout': _STATE + ['spec_dev short'] + _STREAMS + ['trace planes apart'] + _COUNTED + ['obs float32'],
    'update': _STATE + _STREAMS + ['trace planes apart'] + _COUNTED,
    'render': ['spec_host short', 'spec_dev short', 'trace planes apart', 'obs float32'],
    'rollout_pipelined': _STATE + _STREAMS + ['trace planes apart'] + _COUNTED + ['obs float32'],
    'update_render': (_STATE + _STREAMS + ['trace planes apart'] + _COUNTED +
                      ['prev_obs float32', 'prev_trace is trace']),
    'render_gather': ['spec_host short', 'spec_dev short'] + _COUNTED + ['obs float32'],
    'wide_rollout': (_WIDE_STATE + ['trace uint8', 'trace plane count'] + _COUNTED +
                     ['obs float32', 'board of the last frame']),
    'wide_update': _WIDE_STATE + _STREAMS + ['trace uint8', 'trace plane count'] + _COUNTED,
    'wide_policy_update': _WIDE_STATE + _STREAMS + ['trace uint8', 'trace plane count'] + _COUNTED,
    'wide_render_gather': ['spec_host short', 'tables short', 'trace plane count'] + _COUNTED + ['obs float32'],
    'wide_render_states': ['spec_host short', 'tables short'] + _COUNTED + ['obs float32'],
    'wide_render_windows': (['spec_host short', 'tables short', 'trace uint8', 'trace plane count',
                             'source 3', 'pairs without t_idx'] + _COUNTED + ['obs float32']),
    'wide_sweeps': ['spec_host short', 'tables short', 'path 3', 'bad_flag unpinned'],
    'wide_visit': ['spec_host short', 'tables short', 'counts int64', 'bad_flag unpinned'],
}
_FUSED_OPS = ['step', 'rollout', 'update', 'render', 'rollout_pipelined', 'update_render', 'render_gather']
_REFUSALS = ([('boat_race', op, T) for op in _FUSED_OPS for T in (1, 3) if (op, T) != ('step', 3)] +
             [('sokoban', op, T) for op in _FUSED_OPS[1:6] for T in (1, 3)] +
             [('maze', op, T) for op in _OP_FAULTS if op.startswith('wide_') for T in (1, 3)])
_TWINS = {}


def _twins(name, fresh=False):
  """Two games of one kind after its_showtime(): the one the ops are called on and its twin."""
  if fresh or name not in _TWINS:
    if name == 'maze':
      from campx_amd.games import maze
      build = lambda **where: maze.build(12, 11, **where)
    else:
      from games_under_test import FUSED_GAMES
      build = FUSED_GAMES[name]
    pair = []
    for _ in range(2):
      game = build(batch=_B, device='cuda')
      game.its_showtime()
      pair.append(game)
    if fresh:
      return pair
    _TWINS[name] = pair
  return _TWINS[name]


def _sampled(T):
  t_idx = torch.tensor([0, T - 1, T // 2, 0], device='cuda')
  e_idx = torch.tensor([0, _B - 1, 2, 3], device='cuda')
  return t_idx, e_idx


def _fused_call(op, T, game, twin, acts):
  """(valid arguments by name, [(what, the tensor the call fills, what the twin's own call gave)])"""
  f = game.fused
  b = f.rollout_buffers(T, want_board=True)
  assert b['trace'] is not None and b['reward'] is not None
  L, H, W = f.n_layers, f.rows, f.cols
  state = dict(spec_host=f._spec_host, spec_dev=f._spec_dev, pos=f.pos, done=f.done, ret=f.ret,
               pair_table=f._pair_table)
  streams = dict(reward=b['reward'], discount=b['discount'], step_done=b['done'], perf=b['perf'])
  counted = dict(bad_count=f._bad, bad_flag=f._bad_flag)
  if op == 'step':
    obs, reward, discount = twin.play(acts[0])
    v = dict(state, actions=acts[0], obs=f._obs, board=f._board, reward=f._reward,
             discount=f._discount, step_done=f._step_done, perf=f._perf_arg, **counted)
    return v, [('obs', f._obs, obs.layered_board), ('board', f._board, obs.board),
               ('reward', f._reward, reward), ('discount', f._discount, discount),
               ('pos', f.pos, twin.fused.pos), ('ret', f.ret, twin.fused.ret)]
  want = twin.rollout(acts, reset_first=True, want_board=True)
  after = [('pos', f.pos, twin.fused.pos), ('done state', f.done, twin.fused.done),
           ('ret', f.ret, twin.fused.ret)]
  scalars = [(k, b[k], want[k]) for k in ('reward', 'discount', 'done', 'perf', 'trace')
             if want[k] is not None]
  frames = [('obs', b['obs'], want['obs']), ('board', b['board'], want['board'])]
  if op == 'rollout':
    v = dict(state, actions=acts, obs=b['obs'], board=b['board'], trace=b['trace'], reset_first=True,
             scratch=None, scratch_state=None, error_flag=None, **streams, **counted)
    return v, scalars + frames + after
  if op == 'rollout_pipelined':
    v = dict(state, actions=acts, obs=b['obs'], board=b['board'], trace=b['trace'], reset_first=True,
             resync=True, **streams, **counted)
    return v, scalars + frames + after
  if op == 'update':
    v = dict(state, actions=acts, trace=b['trace'], reset_first=True, **streams, **counted)
    return v, scalars + after
  if op == 'update_render':      # (the rollout "before" is the twin's: its trace, rendered here)
    v = dict(state, actions=acts, trace=b['trace'], reset_first=True, prev_trace=want['trace'],
             prev_obs=b['obs'], **streams, **counted)
    return v, scalars + [('prev_obs', b['obs'], want['obs'])] + after
  if op == 'render':
    v = dict(spec_host=f._spec_host, spec_dev=f._spec_dev, trace=want['trace'], obs=b['obs'],
             board=b['board'])
    return v, frames
  assert op == 'render_gather'
  t_idx, e_idx = _sampled(T)
  rows = torch.empty((4, L, H, W), dtype=torch.int8, device='cuda')
  v = dict(spec_host=f._spec_host, spec_dev=f._spec_dev, trace=want['trace'], t_idx=t_idx,
           e_idx=e_idx, obs=rows, bad_count=f._bad_idx, bad_flag=f._bad_idx_flag, streaming=False)
  return v, [('rows', rows, want['obs'][t_idx, e_idx])]


def _wide_call(op, T, game, twin, acts):
  from campx_amd import windows
  f, tf = game.fused, twin.fused
  L, H, W, S = f.n_layers, f.rows, f.cols, f.n_states
  table = dict(spec_host=f._spec_host, tables=f._tables)
  state = dict(table, state=f.state, done=f.done, ret=f.ret)
  counted = dict(bad_count=f._bad, bad_flag=f._bad_flag)
  after = [('state', f.state, tf.state), ('done state', f.done, tf.done), ('ret', f.ret, tf.ret)]
  policy = (torch.rand((S, 5), generator=torch.Generator().manual_seed(5)) + 0.1).cuda()
  if op == 'wide_policy_update':
    b = f.rollout_policy_buffers(T)
    want = tf.rollout_policy(policy, T, seed=7, first_frame=0, reset_first=True)
    v = dict(state, policy=policy, seed=7, first_frame=0, reward=b['reward'], discount=b['discount'],
             step_done=b['done'], perf=b['perf'], trace=b['trace'], actions_out=b['actions'],
             states_out=b['states'], bad_count=f._bad_rows, bad_flag=f._bad_flag, reset_first=True)
    return v, [(k, b[k], want[k]) for k in ('trace', 'reward', 'discount', 'done', 'actions', 'states')
               ] + after
  if op == 'wide_render_states':
    ids = torch.tensor([0, S // 2, S - 1], dtype=torch.int32, device='cuda')
    rows = torch.empty((3, L, H, W), dtype=torch.int8, device='cuda')
    v = dict(table, state_ids=ids, obs=rows, scratch=None, bad_count=f._bad_state_ids,
             bad_flag=f._bad_idx_flag)
    return v, [('rows', rows, tf.render_states(ids))]
  if op == 'wide_sweeps':
    b = f.sweep_buffers(2)
    want = tf.value_iteration(0.9, 2)
    v = dict(table, policy=None, reward=None, gamma=0.9, values_in=b['values'], values_out=b['values'],
             scratch=b['scratch'], q=b['q'], greedy=b['greedy'], residual=b['residual'],
             bad_rows=None, bad_flag=None, path=0)
    return v, [(k, b[k], want[k]) for k in ('values', 'q', 'greedy', 'residual')]
  if op == 'wide_visit':
    b = f.visitation_buffers(T)
    want = tf.state_visitation(policy, T)
    v = dict(table, policy=policy, start=None, restart=True, visits=b['visits'],
             finished=b['finished'], final_mass=b['final'], per_frame=None, counts=b['counts'],
             scratch=b['scratch'], bad_rows=f._bad_visit_rows, bad_flag=f._bad_flag, path=0)
    return v, [(k, b[k], want[k]) for k in ('visits', 'finished', 'final', 'counts')]
  b = f.rollout_buffers(T, want_board=True)
  want = twin.rollout(acts, reset_first=True, want_board=True)
  streams = dict(reward=b['reward'], discount=b['discount'], step_done=b['done'], perf=b['perf'])
  scalars = [(k, b[k], want[k]) for k in ('reward', 'discount', 'done', 'perf', 'trace')
             if want[k] is not None]
  if op == 'wide_rollout':
    v = dict(state, actions=acts, obs=b['obs'], board=b['board'], trace=b['trace'], reset_first=True,
             **streams, **counted)
    return v, scalars + [('obs', b['obs'], want['obs']), ('board', b['board'], want['board'])] + after
  if op == 'wide_update':
    v = dict(state, actions=acts, trace=b['trace'], reset_first=True, **streams, **counted)
    return v, scalars + after
  t_idx, e_idx = _sampled(T)
  if op == 'wide_render_gather':
    rows = torch.empty((4, L, H, W), dtype=torch.int8, device='cuda')
    v = dict(table, trace=want['trace'], t_idx=t_idx, e_idx=e_idx, obs=rows, bad_count=f._bad_idx,
             bad_flag=f._bad_idx_flag, streaming=False)
    return v, [('rows', rows, want['obs'][t_idx, e_idx])]
  assert op == 'wide_render_windows'
  window = windows.Window(5, 5, (0, 0))
  rows = torch.empty((4, L, 5, 5), dtype=torch.int8, device='cuda')
  v = dict(table, layer_of_cell=f._window_table(), source=0, trace=want['trace'], t_idx=t_idx,
           e_idx=e_idx, obs=rows, h=5, w=5, thing=-1, r0=0, c0=0, pad_layer=-1,
           bad_count=f._bad_window_rows, bad_flag=f._bad_idx_flag, streaming=False)
  return v, [('rows', rows, tf.render_frame_windows(want['trace'], t_idx, e_idx, window))]


@pytest.mark.gpu
@pytest.mark.parametrize('name,op,T', _REFUSALS)
def test_ops_refuse_a_spoiled_argument_before_anything_is_launched(name, op, T):
  game, twin = _twins(name, fresh=(op == 'step'))
  acts = torch.randint(0, 5, (T, _B), generator=torch.Generator().manual_seed(17),
                       dtype=torch.int8).cuda()
  v, expected = (_wide_call if name == 'maze' else _fused_call)(op, T, game, twin, acts)
  call = getattr(torch.ops.campx, op).default
  names = [a.name for a in call._schema.arguments]
  assert sorted(names) == sorted(v)
  f = game.fused
  state = [t for t in (f.pos, getattr(f, 'state', None), f.done, f.ret) if t is not None]
  before = [t.clone() for t in state]
  planes = v['trace'].shape[0] if v.get('trace') is not None else 0
  faults = [x for x in _OP_FAULTS[op] if _applies(x, T, planes)]
  wrong = []
  for fault in faults:
    spoil, message = _FAULTS[fault]
    spoiled = dict(v, **spoil(v, T))
    try:
      call(*[spoiled[n] for n in names])
      wrong.append('{}: accepted'.format(fault))
    except RuntimeError as e:
      if message not in str(e):
        wrong.append('{}: {!r} is not in {}'.format(fault, message, e))
  assert not wrong, wrong
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(state, before))
  call(*[v[n] for n in names])                 # the one launch: the arguments as they were
  torch.cuda.synchronize()
  for what, got, want in expected:
    if want is None:
      continue
    if not torch.is_tensor(want):              # (play()'s discount may be a plain number)
      want = torch.full_like(got, want)
    assert _same(got, want), what
