"""What the state-table tier says once and the rest of the package takes from there: the names of
the methods it alone offers (`wide.STATE_TABLE_ONLY`), the format of a table entry's second word
(`_hip.ENTRY_*`, csrc/wide_table.hip.h), and the list of lazy error counters that `_raise_bad()`
words (`FusedGame._lazy_errors`)."""

import inspect

import pytest


def test_every_method_of_the_state_table_tier_alone_is_named_refused_and_forwarded():
  from campx_amd import engine, fused, shapes, wide
  own = {name for name, member in vars(wide.WideGame).items()
         if inspect.isfunction(member) and not name.startswith('_')
         and (name not in vars(fused.FusedGame)
              or getattr(vars(fused.FusedGame)[name], 'state_table_only', False))}
  assert own == set(wide.STATE_TABLE_ONLY), own ^ set(wide.STATE_TABLE_ONLY)
  assert len(set(wide.STATE_TABLE_ONLY)) == len(wide.STATE_TABLE_ONLY)
  for name in wide.STATE_TABLE_ONLY:
    assert inspect.isfunction(vars(engine.Engine).get(name)), 'Engine.{} is missing'.format(name)
    assert inspect.getdoc(vars(engine.Engine)[name]), name
    for tier in (fused.FusedGame, shapes.ShapeGame):
      game = object.__new__(tier)            # (a refusal reads nothing of the game)
      with pytest.raises(NotImplementedError, match=r'^{}\(\) is '.format(name)):
        getattr(game, name)()
      with pytest.raises(NotImplementedError, match=r'^{}\(\) is '.format(name)):
        getattr(game, name)(None, 0.5, 3, out=None)        # (whatever it is called with)
      with pytest.raises(NotImplementedError, match=r'^{}\(\) is '.format(name)):
        getattr(tier, name)(game)                          # a real method of the class
      assert name in dir(tier) and inspect.getdoc(getattr(tier, name))
  # the shape tier refuses the windows of a stored trace for the lack of one, the rest as the
  # one-cell tier does
  shape_game = object.__new__(shapes.ShapeGame)
  with pytest.raises(NotImplementedError, match='not offered by the shape tier'):
    shape_game.render_trace_windows()
  with pytest.raises(NotImplementedError, match='offered by the state-table tier only'):
    shape_game.sweep_buffers()
  assert not hasattr(shape_game, 'no_such_method')


def test_a_batchless_engine_names_the_method_it_cannot_forward():
  from campx_amd import engine
  e = engine.Engine(3, 3)
  with pytest.raises(RuntimeError, match=r'^sweep_buffers\(\) needs a batched Engine \(batch=B\) '
                                         r'that has been through its_showtime\(\)$'):
    e.sweep_buffers(4)


def test_the_entry_format_constants_take_a_hand_packed_word_apart():
  from campx_amd import _hip
  # next state 0x123456 in bits 0..23, done in bit 24, discount code 11 in bits 25..28
  word = 0x123456 | (1 << 24) | (11 << 25)
  assert word == 0x17123456
  assert word & _hip.ENTRY_NEXT_MASK == 0x123456
  assert (word >> _hip.ENTRY_DONE_SHIFT) & 1 == 1
  assert (word >> _hip.ENTRY_DCODE_SHIFT) & _hip.ENTRY_DCODE_MASK == 11
  # the fields do not reach into each other: the largest next state, not done, code 15 and back
  word = 0xffffff | (15 << 25)
  assert word & _hip.ENTRY_NEXT_MASK == 0xffffff
  assert (word >> _hip.ENTRY_DONE_SHIFT) & 1 == 0
  assert (word >> _hip.ENTRY_DCODE_SHIFT) & _hip.ENTRY_DCODE_MASK == 15


@pytest.mark.gpu
def test_three_counters_raised_at_once_come_out_in_one_error_and_are_cleared_together():
  """A rollout with one action id of 7, `evaluate_policy()` of a policy with three bad rows and
  `render_states()` of two ids outside the table, then ONE `check_actions()`: one ValueError whose
  text is the three messages, in the order of `_lazy_errors`, joined by '; '.

  Nothing may raise early.  `validate_actions=False` would see to that, but then `rollout()` and
  `evaluate_policy()` hand their launches no counter (only `render_states()` always counts) and the
  first and third message could never appear; so validation stays on and the three calls are
  captured in a graph: the capture runs nothing, the host's lazy look at the flags finds them
  down, and the replay counts."""
  import torch
  from campx_amd import wide
  from campx_amd.games import boat_race
  B = 16
  game = boat_race.build(B, 'cuda')
  game.use_state_table()
  game.its_showtime()
  f = game.fused
  assert isinstance(f, wide.WideGame) and f.n_states == 8 and f.validate_actions is True
  actions = torch.full((2, B), 4, dtype=torch.int8, device='cuda')
  policy = torch.ones((8, 5), device='cuda')
  ids = torch.tensor([0, 7, 1, 3], dtype=torch.int32, device='cuda')
  frames, sweeps = f.rollout_buffers(2), f.sweep_buffers(2, greedy=False)
  shown = torch.empty((4, f.n_layers, f.rows, f.cols), dtype=torch.int8, device='cuda')

  def calls():
    f.rollout(actions, out=frames)
    f.evaluate_policy(policy, 0.5, 2, out=sweeps)
    f.render_states(ids, out=shown)

  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    calls()                                     # warm up outside the capture: nothing is wrong yet
  torch.cuda.current_stream().wait_stream(side)
  f.check_actions()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):                 # one stream, no parallel branches
    calls()
  actions[1, 5] = 7
  policy[1, 0], policy[4, 2], policy[6, 4] = -1.0, float('nan'), float('inf')
  ids[1], ids[3] = 8, -1
  graph.replay()
  with pytest.raises(ValueError) as caught:
    f.check_actions()
  assert str(caught.value) == (
      '1 action ids are outside 0..4 (or came from rows that are not exactly one-hot); '
      '2 state ids of render_states() are outside the game\'s table (they were rendered as state 0); '
      '3 rows of the policy given to evaluate_policy() are bad (a weight that is negative or NaN, or '
      'a sum that is not a positive finite number); they were evaluated as taking action 4')
  f.check_actions()                             # every counter was cleared with the others
