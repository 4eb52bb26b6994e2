"""Closed-loop rollouts on the GPU: `WideGame.rollout_policy()` (csrc/k_policy.hip,
`campx::wide_policy_update`) against tests/policy_reference.py - the sampling rule and a host
walk of the game's state table, byte for byte - and against the existing kernels fed the actions
it sampled.

The games:
  * maze        the 16x16 maze (159 states; the state-table tier by default);
  * boat_race   the 5x5 boat race put on its state table by `Engine.use_state_table()` (8 states,
                hidden performance);
  * pickups     tests/random_pickups.py definition 3, seven coins on a 4x9 board: the coins are a
                piece MASK, the trace's second plane (470 states, episodes that end);
  * porter      tests/lanes_probes.py's porter on the 10x12 board of test_tabulate_batched.py, put
                on its state table by `use_state_table()`: 5 044 states, two planes.  Its table
                (entries, trace entries and thresholds: 76 bytes per state, 383 KB) is past the
                144 KiB that are staged in LDS, so it takes `wide_policy_update_kernel<false, ..>`,
                which reads table and weights through L1 / L2.  The others take the LDS path;
  * variants    tests/random_pickups.py definition 12 (test_render_states.py's), a tide that turns
                the whole floor: the scenery comes in VARIANTS, and which one shows is the trace's
                second plane (two planes, no discount codes: the K = 2 plain chunks, in LDS).

The weights here are ordinary numbers; tests/test_float_edges.py samples rows of subnormal, -0.0
and FLT_MAX weights.
"""

import re

import numpy as np
import pytest
import torch

import policy_reference as ref

pytestmark = pytest.mark.gpu

GAMES = ['maze', 'boat_race', 'pickups', 'porter', 'variants']
PORTER_BIG = ['############', '#P         #', '# X    #   #', '#      #   #', '#   ####   #',
              '#          #', '#      G   #', '#   #      #', '#   #      #', '############']


def _engine(name, B):
  if name == 'maze':
    from campx_amd.games import maze
    return maze.build(16, 16, batch=B, device='cuda')
  if name == 'boat_race':
    from campx_amd.games import boat_race
    game = boat_race.build(B, 'cuda')
    game.use_state_table()
    return game
  if name == 'pickups':
    import random_pickups
    return random_pickups.builder(random_pickups.definitions()[3])(batch=B, device='cuda')
  if name == 'variants':
    import random_pickups
    return random_pickups.builder(random_pickups.definitions()[12])(batch=B, device='cuda')
  import lanes_probes
  game = lanes_probes.ascii_art_to_game(
      PORTER_BIG, what_lies_beneath=' ', sprites={'P': lanes_probes.Porter},
      drapes={'X': lanes_probes.Crate, '#': lanes_probes.things.FixedDrape,
              'G': lanes_probes.things.FixedDrape},
      z_order='G#XP', update_schedule='PX#G', batch=B, device='cuda')
  game.use_state_table()
  return game


def _game(name, B):
  from campx_amd import wide
  game = _engine(name, B)
  game.its_showtime()
  assert isinstance(game.fused, wide.WideGame), type(game.fused)
  if name == 'variants':
    assert game.fused.spec.n_variants > 1 and game.fused._n_planes == game.fused.n_dyn + 1
  return game


_POLICIES = {}


def _policy(name, S):
  """Random positive weights [S, 5]; every fourth row has exact zeros, and rows are scaled by
  1e-3 and 1e3 in turn.  Computed once per game."""
  if name not in _POLICIES:
    rng = np.random.RandomState(len(name) * 100 + S)
    w = rng.uniform(0.05, 1.0, size=(S, 5)).astype(np.float32)
    for s in range(0, S, 4):
      zeros = rng.choice(5, size=rng.randint(1, 5), replace=False)
      w[s, zeros] = 0.0
    w[1::3] *= np.float32(1e-3)
    w[2::3] *= np.float32(1e3)
    _POLICIES[name] = w
  return _POLICIES[name]


def _same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  if a.dtype.kind == 'f':
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
  return np.array_equal(a, b)


def _check_against_walk(f, out, want, walker, want_states=True):
  for k in ('actions', 'reward', 'discount', 'done', 'perf') + (('states',) if want_states else ()):
    if out.get(k) is None:
      assert k in ('reward', 'perf') and not (f.any_reward if k == 'reward' else f.has_perf), k
      continue
    got = out[k].cpu().numpy()
    assert got.dtype == want[k].dtype, (k, got.dtype)
    assert _same(got, want[k]), k
  assert np.array_equal(f.state.cpu().numpy(), walker.state)
  assert np.array_equal(f.done.cpu().numpy(), walker.over.astype(np.uint8))
  assert _same(f.ret.cpu().numpy(), walker.ret)


def test_names_the_kernel_paths_the_games_take():
  """The docstring's claim: porter's table is past the LDS bound, the others' are not."""
  from campx_amd import _hip
  bound = _hip.config_get('wide_lds_max')
  sizes = {}
  for name in GAMES:
    f = _game(name, 1).fused
    S = f.n_states
    sizes[name] = (S * 5 * 8 + 15) // 16 * 16 + S * 16 + (S * 5 + 15) // 16 * 16 * f.has_perf + S * 20
  assert sizes['porter'] > bound and max(sizes[n] for n in GAMES if n != 'porter') <= bound, sizes


@pytest.mark.parametrize('padded', [True, False], ids=['padded', 'unpadded'])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('name', GAMES)
def test_policy_rollouts_against_the_reference_walk(name, B, padded, monkeypatch):
  """T = 1, 7, 8, 9, 20 one call after the other, the frame counter continuing: the calls start
  at frames 0, 1, 8, 16 and 25 - both sides of the 8-frame chunk and of the 4-frame Philox group.
  The calls at 1 and 25 start inside a Philox group (lead 1); the T = 20 call at 25 is long
  enough to run whole (plain) chunks behind a non-zero lead.  `reset_first` on (calls 0 and 3) and
  off.  Then an explicit `first_frame` of 2^40 + 6 (lead 2, the high counter word in use), then a
  call without 'states'."""
  from campx_amd import fused
  monkeypatch.setattr(fused, 'PAD_ROWS', padded)
  game = _game(name, B)
  f = game.fused
  traced = f.traced
  assert f.n_states == traced.n_states
  w = _policy(name, f.n_states)
  policy = torch.from_numpy(w).cuda()
  walker = ref.PolicyWalker(traced, B)
  first, frame = 0, 0
  for i, T in enumerate((1, 7, 8, 9, 20)):
    reset = i in (0, 3)
    out = game.rollout_policy(policy, T, seed=0x1234567890abcdef, reset_first=reset)
    want = walker.rollout(w, T, seed=0x1234567890abcdef, reset_first=reset)
    assert out['actions'].shape == (T, B) and out['states'].shape == (T, B)
    assert out['trace'].shape == (f._n_planes, T, B)
    pitch = (B + 15) // 16 * 16 if padded and T > 1 else None
    if pitch:
      assert out['actions'].stride(0) == pitch and out['states'].stride(0) == pitch
    elif T > 1:
      assert out['actions'].stride(0) == B
    _check_against_walk(f, out, want, walker)
    assert want['bad'] == 0
    first, frame = first + T, (T if reset else frame + T)
    assert f._policy_frame == first and f.frame == frame
  # an explicit first_frame that is no multiple of 4 is used as given and moves the counter
  out = game.rollout_policy(policy, 9, seed=3, first_frame=(1 << 40) + 6)
  want = walker.rollout(w, 9, seed=3, first_frame=(1 << 40) + 6)
  _check_against_walk(f, out, want, walker)
  assert f._policy_frame == (1 << 40) + 15
  # without 'states', into buffers allocated once; a policy that requires grad is detached
  bufs = game.rollout_policy_buffers(7, want_states=False)
  assert 'states' not in bufs
  out = game.rollout_policy(policy.clone().requires_grad_(), 7, seed=3, out=bufs, want_states=False)
  want = walker.rollout(w, 7, seed=3)
  assert out is bufs
  _check_against_walk(f, out, want, walker, want_states=False)
  f.check_actions()


@pytest.mark.parametrize('B', [65, 257])
@pytest.mark.parametrize('name', GAMES)
def test_policy_rollouts_against_the_existing_kernels(name, B):
  """The actions a policy rollout sampled, fed to `rollout_trace()` on an identically built game
  from the same start: the same trace in every plane, scalars and final state; and
  `render_frames()` on the policy rollout's trace is `rollout()`'s 'obs' at sampled pairs."""
  a, b = _game(name, B), _game(name, B)
  fa, fb = a.fused, b.fused
  policy = torch.from_numpy(_policy(name, fa.n_states)).cuda()
  for T, reset in ((20, True), (9, False)):
    out = a.rollout_policy(policy, T, seed=77, reset_first=reset)
    acts = out['actions'].contiguous()
    assert int(acts.min()) >= 0 and int(acts.max()) <= 4
    want = b.rollout_trace(acts, reset_first=reset)
    assert out['trace'].shape == want['trace'].shape and out['trace'].stride() == want['trace'].stride()
    for k in ('trace', 'reward', 'discount', 'done', 'perf'):
      if want[k] is None:
        assert out[k] is None, k
      else:
        assert _same(out[k].cpu().numpy(), want[k].cpu().numpy()), (T, k)
    for k in ('state', 'done', 'ret'):
      assert _same(getattr(fa, k).cpu().numpy(), getattr(fb, k).cpu().numpy()), (T, k)
    assert fa.frame == fb.frame
  if name == 'pickups':
    assert fa._n_planes == 2 and fa.spec.n_pieces > 0
    assert len(torch.unique(out['trace'][1])) > 1            # the mask plane changes
  # observations: the first rollout again, rendered in full by the existing kernels
  out = a.rollout_policy(policy, 20, seed=77, first_frame=0, reset_first=True)
  full = b.rollout(out['actions'].contiguous(), reset_first=True)
  gen = torch.Generator().manual_seed(B)
  t_idx = torch.randint(0, 20, (300,), generator=gen).cuda()
  e_idx = torch.randint(0, B, (300,), generator=gen).cuda()
  t_idx[:2], e_idx[:2] = torch.tensor([0, 19]), torch.tensor([0, B - 1])
  got = a.render_frames(out['trace'], t_idx, e_idx)
  assert torch.equal(got, full['obs'][t_idx, e_idx])
  assert _same(out['trace'].cpu().numpy(), full['trace'].cpu().numpy())
  a.fused.check_actions()
  b.fused.check_actions()


def test_one_hot_rows_along_the_shortest_way_solve_the_maze():
  """A deterministic policy: breadth-first search over `st_next` for the shortest way from the
  start to an entry that ends the episode, one-hot rows along it ('stay' everywhere else).  Every
  environment reaches the goal on the same frame, `done` fires, and the next frame samples from
  row 0 again: a second episode like the first."""
  B = 257
  game = _game('maze', B)
  f = game.fused
  g = f.traced
  S = g.n_states
  parent, queue, goal = {0: None}, [0], None
  while queue and goal is None:
    s = queue.pop(0)
    for a in range(4):
      if g.st_done[s, a]:
        goal = (s, a)
        break
      n = int(g.st_next[s, a])
      if n not in parent:
        parent[n] = (s, a)
        queue.append(n)
  assert goal is not None
  w = np.zeros((S, 5), np.float32)
  w[:, 4] = 1.0
  s, a = goal
  length = 0
  while True:
    w[s] = 0.0
    w[s, a] = 2.5                       # (not normalised)
    length += 1
    if parent[s] is None:
      break
    s, a = parent[s]
  assert length > 10
  T = 2 * length + 3
  out = game.rollout_policy(torch.from_numpy(w).cuda(), T, seed=5, reset_first=True)
  done = out['done'].cpu().numpy()
  states = out['states'].cpu().numpy()
  want_done = np.zeros(T, np.uint8)
  want_done[[length - 1, 2 * length - 1]] = 1
  assert np.array_equal(done, np.tile(want_done[:, None], (1, B)))
  assert (states[[0, length, 2 * length]] == 0).all()
  assert np.array_equal(states[:length], states[length:2 * length])
  assert (out['discount'].cpu().numpy()[length - 1] == 0).all()
  assert np.array_equal(states, np.tile(states[:, :1], (1, B)))
  want = ref.PolicyWalker(g, B).rollout(w, T, seed=5, reset_first=True)
  assert _same(states, want['states']) and _same(out['reward'].cpu().numpy(), want['reward'])
  f.check_actions()


@pytest.mark.parametrize('kind', ['nan', 'negative', 'all zero'])
def test_bad_policy_rows_raise_lazily_with_their_count(kind):
  B, T = 65, 20
  game = _game('boat_race', B)
  f = game.fused
  w = _policy('boat_race', f.n_states).copy()
  rows = {'nan': [np.nan, 1, 1, 1, 1], 'negative': [1, 1, -0.25, 1, 1], 'all zero': [0, 0, 0, 0, 0]}
  w[0] = rows[kind]
  w[3] = rows[kind]
  walker = ref.PolicyWalker(f.traced, B)
  want = walker.rollout(w, T, seed=9, reset_first=True)
  assert want['bad'] >= B                       # every environment starts from row 0
  bufs = game.rollout_policy_buffers(T)
  with pytest.raises(ValueError, match='bad policy rows') as e:
    game.rollout_policy(torch.from_numpy(w).cuda(), T, seed=9, reset_first=True, out=bufs)
    f.check_actions()
  count = int(re.match(r'(\d+) environment-frames of rollout_policy\(\) met bad policy rows',
                       str(e.value)).group(1))
  assert count == want['bad']
  torch.cuda.synchronize()
  _check_against_walk(f, bufs, want, walker)
  states, actions = bufs['states'].cpu().numpy(), bufs['actions'].cpu().numpy()
  met = (states == 0) | (states == 3)
  assert met.sum() == count and (actions[met] == 4).all()
  # cleared: nothing left to raise, and a good policy raises nothing
  f.check_actions()
  assert int(f._bad_rows.item()) == 0 and int(f._bad.item()) == 0 and int(f._bad_flag_view[0]) == 0
  game.rollout_policy(torch.from_numpy(_policy('boat_race', f.n_states)).cuda(), T)
  f.check_actions()


def test_error_cases_and_settings():
  from campx_amd import fused, shapes, tabulate
  from campx_amd.games import boat_race, hello_world, maze
  game = _game('boat_race', 64)
  S = game.fused.n_states
  good = torch.ones((S, 5), device='cuda')
  for bad, what in ((torch.ones((S + 1, 5), device='cuda'), 'shape'),
                    (torch.ones((S, 4), device='cuda'), 'shape'),
                    (torch.ones((S * 5,), device='cuda'), 'shape'),
                    (torch.ones((S, 5), device='cuda', dtype=torch.float64), 'dtype'),
                    (torch.ones((S, 5), device='cuda', dtype=torch.float16), 'dtype'),
                    (torch.ones((S, 5)), 'device'),
                    (torch.ones((5, S), device='cuda').t(), 'not contiguous'),
                    (np.ones((S, 5), np.float32), 'not a tensor')):
    with pytest.raises(ValueError, match=r'policy must be a contiguous float32 \[8, 5\] tensor'):
      game.rollout_policy(bad, 4)
  with pytest.raises(ValueError, match='at least one frame'):
    game.rollout_policy(good, 0)
  with pytest.raises(ValueError, match='first_frame'):
    game.rollout_policy(good, 4, first_frame=-1)
  with pytest.raises(ValueError, match='rollout_policy_buffers'):
    game.rollout_policy(good, 4, out=game.rollout_policy_buffers(5))
  with pytest.raises(ValueError, match='rollout_policy_buffers'):
    game.rollout_policy(good, 4, out=game.rollout_policy_buffers(4, want_states=False))
  with pytest.raises(ValueError, match='rollout_policy_buffers'):      # another batch size's buffers
    game.rollout_policy(good, 4, out=_game('boat_race', 65).rollout_policy_buffers(4))
  assert game.fused._policy_frame == 0                       # (nothing ran)
  # use_state_table() is a set-up call
  with pytest.raises(RuntimeError, match='use_state_table'):
    game.use_state_table()
  # an engine without the call still builds the tier it builds today, which refuses by name
  plain = boat_race.build(64, 'cuda')
  plain.its_showtime()
  assert type(plain.fused) is fused.FusedGame
  for call in (lambda: plain.rollout_policy(good, 4), lambda: plain.rollout_policy_buffers(4)):
    with pytest.raises(NotImplementedError, match=r'state-table tier.*use_state_table\(\)'):
      call()
  hello = hello_world.build(batch=16, device='cuda')
  hello.its_showtime()
  assert isinstance(hello.fused, shapes.ShapeGame)
  for call in (lambda: hello.rollout_policy(good, 4), lambda: hello.rollout_policy_buffers(4)):
    with pytest.raises(NotImplementedError, match=r'state-table tier.*use_state_table\(\)'):
      call()
  # a game that cannot be tabulated says so, unchanged (tests/lanes_probes.py: draws random numbers)
  import lanes_probes
  dice = lanes_probes.ascii_art_to_game(
      lanes_probes.ART, what_lies_beneath=' ',
      drapes={'A': lanes_probes.Rand, 'B': lanes_probes.Still, '#': lanes_probes.things.FixedDrape,
              'G': lanes_probes.things.FixedDrape},
      z_order='G#BA', update_schedule='AB#G', batch=16, device='cuda')
  dice.use_state_table()
  with pytest.raises(tabulate.TabulationError, match='draws random numbers'):
    dice.its_showtime()
  # the generic tier, and a batched engine before its_showtime()
  for engine in (maze.build(16, 16), maze.build(16, 16, batch=4, device='cuda')):
    with pytest.raises(RuntimeError, match='batched Engine'):
      engine.rollout_policy(good, 4)
    with pytest.raises(RuntimeError, match='batched Engine'):
      engine.rollout_policy_buffers(4)


def _op_args(f, policy, bufs, seed, first_frame, reset_first):
  return (f._spec_host, f._tables, f.state, f.done, f.ret, policy, seed, first_frame,
          bufs['reward'], bufs['discount'], bufs['done'], bufs['perf'], bufs['trace'],
          bufs['actions'], bufs.get('states'), f._bad_rows, None, reset_first)


def test_opcheck_and_schema():
  from campx_amd import _hip
  assert 'wide_policy_update' in _hip.OP_NAMES
  s = str(torch.ops.campx.wide_policy_update.default._schema)
  for part in ('Tensor policy', 'int seed', 'int first_frame', 'Tensor(h!) trace',
               'Tensor(i!) actions_out', 'Tensor(j!)? states_out', 'bool reset_first'):
    assert part in s, s
  f = _game('boat_race', 128).fused
  policy = torch.from_numpy(_policy('boat_race', f.n_states)).cuda()
  bufs = f.rollout_policy_buffers(9)
  torch.library.opcheck(torch.ops.campx.wide_policy_update.default,
                        _op_args(f, policy, bufs, 5, 6, True))          # all four checks
  # no CPU key
  cpu = [x.cpu() if torch.is_tensor(x) else x for x in _op_args(f, policy, bufs, 5, 6, True)]
  with pytest.raises((NotImplementedError, RuntimeError)):
    torch.ops.campx.wide_policy_update(*cpu)


def test_capture_in_a_hip_graph_replays_the_captured_frames():
  """`first_frame` is an argument of the captured launch: every replay samples the SAME frames.
  With `reset_first` both replays start alike too, so their outputs are identical - and equal to
  the reference walk of those frames.  (A graph that should continue is captured per frame
  range, or its `first_frame` changed through the graph's kernel-node parameters.)"""
  B, T = 257, 20
  game = _game('maze', B)
  f = game.fused
  f.validate_actions = False
  w = _policy('maze', f.n_states)
  policy = torch.from_numpy(w).cuda()
  bufs = game.rollout_policy_buffers(T)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    game.rollout_policy(policy, T, seed=21, first_frame=6, reset_first=True, out=bufs)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    game.rollout_policy(policy, T, seed=21, first_frame=6, reset_first=True, out=bufs)
  kept = []
  for _ in range(2):
    for k in ('actions', 'states', 'reward', 'trace'):
      bufs[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    kept.append({k: v.clone() for k, v in bufs.items() if v is not None})
    kept[-1]['state'] = f.state.clone()
  for k in kept[0]:
    assert _same(kept[0][k].cpu().numpy(), kept[1][k].cpu().numpy()), k
  walker = ref.PolicyWalker(f.traced, B)
  want = walker.rollout(w, T, seed=21, first_frame=6, reset_first=True)
  _check_against_walk(f, bufs, want, walker)
