"""tests/action_views.py examined without a device: the views are where they say, the dirty streams
are dirty where they say, the reference needs `cleaned`, and the case lists that
tests/test_action_views.py runs reach every branch of csrc/k_update.hip's ActionLoader."""

import numpy as np
import pytest
import torch

from campx_amd import gamespec
from campx_amd.games import boat_race
from oracle import cpu

import action_views as av


@pytest.mark.parametrize('fill', av.FILLS)
@pytest.mark.parametrize('shape', [(3, 5), (1, 1), (65, 17), (257,)])
def test_action_view_is_where_it_says_between_its_guards(shape, fill):
  a = np.random.RandomState(len(shape)).randint(0, 5, size=shape).astype(np.int8)
  T, B = (1,) + shape if len(shape) == 1 else shape
  for offset in range(16):
    view, arena, start = av.action_view(a, offset, fill, 'cpu')
    assert view.dtype == torch.int8 and tuple(view.shape) == shape and view.is_contiguous()
    assert view.data_ptr() % 16 == offset
    assert view.data_ptr() == arena.data_ptr() + start
    assert np.array_equal(view.numpy(), a)
    assert start >= 4096 and arena.numel() - (start + a.size) >= 4096
    assert av.guards_hold(arena, start, a.size, fill)
    # both fills are really there, right up to the view on both sides
    assert int(arena[start - 1]) == fill and int(arena[start + a.size]) == fill
    assert int(arena[0]) == fill and int(arena[-1]) == fill
    # writing the view changes its own bytes and no others
    view.fill_(3)
    assert av.guards_hold(arena, start, a.size, fill)
    assert bool((arena[start:start + a.size] == 3).all())
  assert av.FILL_BAD - 256 == -91 and not 0 <= av.FILL_BAD - 256 <= 4 and 0 <= av.FILL_MOVE <= 3
  # the offset that puts the stream's end on a 16-byte boundary
  for offset in av.offsets_for(T, B):
    view, arena, start = av.action_view(a, offset, fill, 'cpu')
    assert view.data_ptr() % 16 == offset
  if B % 16:
    end = [o for o in av.offsets_for(T, B) if (o + T * B) % 16 == 0]
    assert len(end) == 1
    view, _, _ = av.action_view(a, end[0], fill, 'cpu')
    assert (view.data_ptr() + T * B) % 16 == 0
  assert set(av.OFFSETS) <= set(av.offsets_for(T, B))


def _shapes():
  grid = {(T, B) for T in av.FRAMES for B in av.BATCHES}
  grid |= {(T, B) for T in av.FEW_FRAMES for B in av.BIG_BATCHES}
  grid |= {(T, B) for T in av.STAGED_FRAMES for B in av.STAGED_BATCHES}
  grid |= {(T, B) for T in av.SHAPE_FRAMES for B in av.SHAPE_BATCHES}
  grid |= {(1, n) for n in av.CHECK_SIZES}
  return sorted(grid)


def test_dirty_streams_are_dirty_where_they_say():
  for T, B in _shapes():
    s = av.streams(T, B, 1000 * T + B)
    clean, dirty, cleaned = s['clean'], s['dirty'], s['cleaned']
    for x in (clean, dirty, cleaned):
      assert x.dtype == np.int8 and x.shape == (T, B)
    bad = (dirty < 0) | (dirty > 4)
    assert s['n_bad'] == int(bad.sum()) > 0
    assert clean.min() >= 0 and clean.max() <= 4 and cleaned.min() >= 0 and cleaned.max() <= 4
    forced = av.forced_positions(T, B)
    assert {(0, 0), (0, B - 1), (T - 1, 0), (T - 1, B - 1)} <= set(forced)
    if B % 16:
      assert {(t, e) for t in (0, T - 1) for e in range(B - B % 16, B)} <= set(forced)
    assert ((1, 0) in forced) == (T > 1)
    for t, e in forced:
      assert bad[t, e], (T, B, t, e)
    assert set(np.unique(dirty[bad]).tolist()) <= set(av.BAD_IDS)
    assert np.array_equal(dirty != cleaned, bad) and bool((cleaned[bad] == av.STAY).all())
    assert np.array_equal(dirty[~bad], clean[~bad])
    if T * B >= 4096:
      # bad ids lie over moves and over "stay" alike, and every one of the five occurs
      assert len(np.unique(clean[bad])) == 5 and len(np.unique(dirty[bad])) == 5
    again = av.streams(T, B, 1000 * T + B)
    assert all(np.array_equal(s[k], again[k]) for k in ('clean', 'dirty', 'cleaned'))


def _union(cases, envs):
  paths, shifts = set(), set()
  for T, B in cases:
    p, s = av.loader_paths(T, B, envs)
    paths |= p
    shifts |= s
  return paths, shifts


def test_the_case_lists_reach_every_branch_of_the_action_loader():
  """A condition on the case lists: a branch that is missing means a longer list, not a shorter
  assertion.  (loader_paths() also asserts, at every load, that it lies inside the T * B bytes.)"""
  small = [(T, B) for T in av.FRAMES for B in av.BATCHES]
  paths, shifts = _union(small, 256)
  assert paths == set(av.PATHS), set(av.PATHS) - paths
  # shift_down() has a dword part (bytes >> 2) and a byte part (bytes & 3): every dword count,
  # with and without a byte part
  assert {s >> 2 for s in shifts} == {0, 1, 2, 3} and {s & 3 for s in shifts} == {0, 1, 2, 3}
  assert min(shifts) < 4 < max(shifts) and min(shifts) < 8 < max(shifts)
  # ... with the three frame counts of the pair and tuple games alone, too
  paths, shifts = _union([(T, B) for T in av.FEW_FRAMES for B in av.BATCHES], 256)
  assert paths == set(av.PATHS)
  assert min(shifts) < 4 < max(shifts) and min(shifts) < 8 < max(shifts)
  # the 512-environment workgroups: what the child process really launches them with - from
  # B = 512 up under big_wgs=1, and the tiny batches under big_wgs=0, where T * B < 16 exists
  paths, shifts = _union(av.big_cases(), 512)
  assert paths == set(av.PATHS), set(av.PATHS) - paths
  assert min(shifts) < 4 < max(shifts) and min(shifts) < 8 < max(shifts)
  assert 'bytes' in _union([(T, B) for T in av.BIG_TINY_FRAMES for B in av.BIG_TINY_BATCHES], 512)[0]
  assert {15, 45} <= {T * B for T in av.BIG_TINY_FRAMES for B in av.BIG_TINY_BATCHES}
  # both sides of a workgroup, T * B of 15 and 16 exactly, one environment
  assert {255, 256, 257} <= set(av.BATCHES) and {511, 512, 513} <= set(av.BIG_BATCHES)
  assert {15, 16} <= {T * B for T, B in small} and 1 in av.BATCHES
  assert av.loader_paths(3, 5, 256)[0] == {'bytes', 'row_clamped', 'odd_T'}
  assert av.loader_paths(1, 16, 256)[0] == {'whole', 'row_clamped', 'odd_T'}


def test_single_launch_paths():
  assert av.loader_paths(64, 256, 256) == ({'whole'}, set())
  assert av.loader_paths(64, 512, 512) == ({'whole'}, set())
  assert av.loader_paths(65, 256, 256)[0] == {'whole', 'second_chunk', 'row_clamped', 'odd_T'}
  assert av.loader_paths(2, 17, 256) == ({'whole', 'partial', 'partial_shifted', 'row_clamped'}, {15})
  assert av.loader_paths(16, 1, 256)[1] == set(range(1, 16))


def test_the_oracle_refuses_a_dirty_stream_and_repeats_itself_on_the_cleaned_one():
  og = cpu.OracleGame.from_description(gamespec.describe(boat_race.build()))
  s = av.streams(17, 33, 5)
  with pytest.raises(ValueError, match='outside 0..4'):
    og.rollout(s['dirty'], reset_first=True)
  a = og.rollout(s['cleaned'], reset_first=True)
  b = og.rollout(s['cleaned'], reset_first=True)
  for k in ('obs', 'board', 'done', 'perf'):
    assert np.array_equal(a[k], b[k]), k
  for k in ('reward', 'discount'):
    assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
  # ... and the bad ids were not all laid over "stay": the clean stream plays another game
  c = og.rollout(s['clean'], reset_first=True)
  assert not np.array_equal(a['obs'], c['obs'])
