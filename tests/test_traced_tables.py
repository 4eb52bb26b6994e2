"""`tabulate._fill_tables` - the one builder of the state table, the discount codes, the hidden
performance and the dense table behind both state-graph walkers - against their restatement one
edge at a time (tests/traced_tables_reference.py).

Both walkers call the same builder, so their agreement
(test_tabulate_batched.py::test_lane_walker_and_play_walker_produce_the_same_traced_game) checks
the walks, not the tables.  Here every tabulated game's tables are rebuilt from its own graph with
a Python statement per edge and must come out the same, field for field, dtype and bit pattern -
in the one-frame-per-play walker's mode, and in the many-states-per-call walker's where it takes
the game.  CPU only."""

import pytest
import torch

from campx_amd import gamespec, tabulate
from campx_amd.games import boat_race, wall_world
import lanes_games
import lanes_probes
import random_coins
import random_pickups
import traced_games
import traced_tables_reference as reference

PICKUPS = random_pickups.definitions()
ROADS = {'own': {}, 'dense': dict(PIECES_AS_THINGS_MAX=3), 'variants': dict(WIDE_MAX_PIECES=0),
         'things': dict(WIDE_MAX_PIECES=0, WIDE_MAX_VARIANTS=1)}


def penalty_warehouse():
  """The two-crate warehouse with a hidden PENALTY for where the crates stand (no game of the
  other suites that is tabulated from its classes declares one): -5 per crate in the floor's left
  column, -10 in its right column."""
  game = lanes_games.small_warehouse()
  columns = torch.zeros(2, 5, 6, dtype=torch.uint8)
  columns[0, 1:4, 1] = 1
  columns[1, 1:4, 4] = 1
  game.set_hidden_penalty('XY', list(columns), -5)
  return game


def _halves(game, ch):
  """`game` with a hidden performance that watches `ch` between the board's two halves."""
  left = torch.zeros(game.rows, game.cols, dtype=torch.uint8)
  left[:, :game.cols // 2] = 1
  game.set_hidden_performance(ch, [left, 1 - left])
  return game


# name -> (builder, the bounds of `gamespec` lowered for it)
GAMES = {'boat_race': (boat_race.build, {}), 'wall_world': (wall_world.build, {}),
         'small_warehouse': (lanes_games.small_warehouse, {}), 'penalty_warehouse': (penalty_warehouse, {}),
         'nothing_moves': (random_coins.library_builder(random_coins.definitions()[11], rebound=True), {})}
# the games the many-states-per-call walker takes: restated in both walkers' modes
ON_LANES = {'boat_race', 'wall_world', 'small_warehouse', 'penalty_warehouse',
            'ice_rink', 'mirror', 'toll_road', 'trio', 'vault'}
for _name in sorted(traced_games.GAMES) + sorted(traced_games.HIDDEN_STATE_GAMES):
  GAMES[_name] = (getattr(traced_games, _name), {})
for _a, _b, _how in lanes_probes.CASES:
  if not _how.startswith('REFUSED'):
    _name = 'probe-{}-{}'.format(_a.__name__, _b.__name__)
    GAMES[_name] = (lanes_probes.game(_a, _b), {})
    if _how.startswith('lanes: '):
      ON_LANES.add(_name)
# every game of tests/random_pickups.py down its own road, and down the other roads as
# tests/test_random_pickups.py sends them - but for game 15 (1 097 states: some 10 s of walking)
for _k, _road in ([(k, 'own') for k in range(15)] + [(k, 'variants') for k in (3, 5, 10)] +
                  [(k, 'things') for k in (3, 4, 9, 10)] + [(k, 'dense') for k in (0, 1, 7)]):
  GAMES['pickup{}-{}-{}'.format(_k, PICKUPS[_k]['kind'], _road)] = (random_pickups.builder(PICKUPS[_k]), ROADS[_road])
# (the plain warehouse takes the one-frame-per-play walker some 5-10 s; the one with the penalty is walked)
CASES = ([(name, 'walk') for name in GAMES if name != 'small_warehouse'] +
         [(name, 'batch') for name in GAMES if name in ON_LANES])
_TRACED = {}


def _traced(name, mode, monkeypatch):
  """The game tabulated by one walker (once per test process; read-only)."""
  if (name, mode) not in _TRACED:
    build, bounds = GAMES[name]
    with monkeypatch.context() as m:
      for bound, value in bounds.items():
        m.setattr(gamespec, bound, value)
      m.setenv('CAMPX_TABULATE', mode)
      m.setattr(tabulate, 'LAST_WALK', [''])
      _TRACED[name, mode] = tabulate.trace(build(), cache=False)
      assert tabulate.LAST_WALK[0].startswith('lanes: ') == (mode == 'batch')
  return _TRACED[name, mode]


def test_the_lane_walker_takes_no_other_game_of_the_list(monkeypatch):
  """`ON_LANES` is every game that can be restated in the many-states-per-call walker's mode."""
  monkeypatch.setenv('CAMPX_TABULATE', 'batch')
  for name, (build, bounds) in GAMES.items():
    if name not in ON_LANES:
      with monkeypatch.context() as m:
        for bound, value in bounds.items():
          m.setattr(gamespec, bound, value)
        with pytest.raises(Exception):      # (`TabulationError`: not this walker's game; NumpyWriter: its own ValueError)
          tabulate.trace(build(), cache=False)


@pytest.mark.parametrize('name,mode', CASES, ids=['{}-{}'.format(*c) for c in CASES])
def test_the_tables_are_what_one_edge_at_a_time_gives(name, mode, monkeypatch):
  game = _traced(name, mode, monkeypatch)
  assert reference.first_difference(game, reference.tables_of(game)) is None


def test_the_games_reach_every_branch_of_the_builder(monkeypatch):
  def walked(name):
    return _traced(name, 'walk', monkeypatch)

  burrow, dasher, vault = walked('burrow'), walked('dasher'), walked('vault')
  # modes (one more tracked value, in the dense table too): a z-order that changes, a hidden value
  assert len(burrow.mode_orders) > 1 and burrow.n_tracked == 2 and burrow.n == (5 * 9) ** 2 * 5
  assert dasher.hidden_paths and dasher.n_tracked == 2
  assert any(vault.absent_cells) and not vault.st_present.all()
  assert 'T' in walked('trio').movers                                     # (a Sprite)
  assert walked('toll_road').discount_list == [1.0, 0.5, 0.25, 0.75]
  assert walked('boat_race').perf_spec is not None and walked('boat_race').st_perf.any()
  penalty = _traced('penalty_warehouse', 'batch', monkeypatch)
  assert penalty.penalty_spec is not None and set(penalty.st_perf.reshape(-1).tolist()) >= {0, -5, -10}
  assert walked('pickup0-coins-own').pieces_as_mask
  dense = walked('pickup0-coins-dense')
  assert dense.movers == ['A', 'o', 'o'] and dense.n is not None          # pieces in the dense table
  assert all(sorted(m) == ['o'] for m in walked('pickup3-coins-variants').variant_masks)
  assert len(walked('pickup12-tide-own').variants) == 2 and len(walked('pickup13-seasons-own').variants) == 3
  assert any(walked('pickup9-lamps-things').in_backdrop) and any(walked('pickup9-lamps-own').in_backdrop)
  assert walked('nothing_moves').n_states == 1
  # a state the walk only ever saw ended: a row of edges never played, beside rows that were
  reached = walked('ice_rink').st_reached
  assert (~reached).all(axis=1).any() and reached.all(axis=1).any()


def test_the_refusals_of_a_hidden_performance(monkeypatch):
  for mode in ('walk', 'batch'):
    monkeypatch.setenv('CAMPX_TABULATE', mode)
    with pytest.raises(tabulate.TabulationError, match="hidden performance watches '#', which never moves"):
      tabulate.trace(_halves(traced_games.ice_rink(), '#'), cache=False)
    with pytest.raises(tabulate.TabulationError, match="hidden performance watches 'k', which leaves the board"):
      tabulate.trace(_halves(traced_games.vault(), 'k'), cache=False)
    game = traced_games.vault()
    game.set_hidden_penalty('Ak', [torch.ones(game.rows, game.cols, dtype=torch.uint8)], -5)
    with pytest.raises(tabulate.TabulationError, match="hidden penalty watches 'k', which leaves the board"):
      tabulate.trace(game, cache=False)
  monkeypatch.setenv('CAMPX_TABULATE', 'walk')
  with pytest.raises(tabulate.TabulationError, match="hidden performance watches 'o', a drape of several cells"):
    tabulate.trace(_halves(random_pickups.builder(PICKUPS[0])(), 'o'), cache=False)


def test_a_penalty_that_does_not_fit_the_tables_is_refused_by_both_walkers(monkeypatch):
  """`st_perf` is int8.  `Engine.set_hidden_penalty` keeps a declared penalty within 112; one put
  there behind its back (100 a class: 200 for the skater in the rink's right half, the class of the
  first edge that leaves the left) is the OverflowError the one-frame-per-play walker always gave,
  from either walker - not a value that wrapped."""
  for mode in ('walk', 'batch'):
    monkeypatch.setenv('CAMPX_TABULATE', mode)
    game = traced_games.ice_rink()
    left = torch.zeros(game.rows, game.cols, dtype=torch.uint8)
    left[:, :game.cols // 2] = 1
    game.set_hidden_penalty('A', [left, 1 - left], 16)
    who, masks, _ = game._hidden_penalty
    game._hidden_penalty = (who, masks, 100)
    with pytest.raises(OverflowError, match='Python integer 200 out of bounds for int8'):
      tabulate.trace(game, cache=False)


class NanDiscounter(lanes_probes.Mover):
  def update(self, actions, board, layers, backdrop, all_things, the_plot):
    super(NanDiscounter, self).update(actions, board, layers, backdrop, all_things, the_plot)
    if actions is not None:
      the_plot.change_default_discount(float('nan'))


def test_a_discount_that_is_not_a_number_never_reaches_the_tables(monkeypatch):
  """(the discount codes compare values: the Plot refuses a NaN before a walker sees it)"""
  for mode in ('walk', 'batch'):
    monkeypatch.setenv('CAMPX_TABULATE', mode)
    with pytest.raises(ValueError, match='Pcontinue must be in range'):
      tabulate.trace(lanes_probes.game(NanDiscounter)(), cache=False)
