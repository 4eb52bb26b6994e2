"""Run by tests/test_action_views.py in child processes (the library reads big_wgs once per
process), with the value of big_wgs as the argument:

  1  the library picks its 512-environment update workgroups from B = 512 up: the three table games
     around that size (`BIG_BATCHES`), T of 1, 3 and 65.  Only update_table_kernel and
     update_pair_kernel HAVE a 512-environment form; the tuple kernel (sokoban level 2) always runs
     256-environment workgroups and simply gets the larger batches here;
  0  512-environment workgroups at EVERY batch: the boat race and sokoban level 0 at the tiny shapes
     (`BIG_TINY_BATCHES` x `BIG_TINY_FRAMES`) where T * B < 16 and ActionLoader<512, .> goes byte by
     byte.

Clean and dirty streams at every offset between both fills - outputs on bits against the oracle,
the count of bad ids exactly; one `ok` line per (game, B)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from campx_amd import _hip               # noqa: E402

BIG_WGS = int(sys.argv[1])
assert BIG_WGS in (0, 1)
_hip.config_set('big_wgs', BIG_WGS)      # before anything is launched

import action_views as av                # noqa: E402
import test_action_views as tav          # noqa: E402


def main():
  assert _hip.config_get('big_wgs') == BIG_WGS
  games = tav.TABLE_GAMES if BIG_WGS else tav.BIG_FORM_GAMES
  batches, frames = ((av.BIG_BATCHES, av.FEW_FRAMES) if BIG_WGS else
                     (av.BIG_TINY_BATCHES, av.BIG_TINY_FRAMES))
  for name in games:
    for B in batches:
      for fill in av.FILLS:
        tav._table_game_cases(name, B, fill, frames)
      print('ok', name, B, flush=True)


if __name__ == '__main__':
  main()
