"""Output views at chosen addresses modulo a render window, with canaries on both sides.

The one-shot render kernels (csrc/k_gather.hip, k_window.hip, k_render.hip) cut their output into
windows of 2 KiB that are aligned in MEMORY; everything they do for the first window hangs on
`shift`, the distance from that window's start to the output's first byte.  A fresh allocation
only ever starts at a multiple of 512 bytes.  `arena_view()` puts a view at any residue modulo
2 048 inside a larger arena filled with 0xA5, so that a byte written outside the view - or one
inside it that was never written - shows: 0xA5 is neither 0 nor 1 as int8, and 0xA5A5 is neither
0, 0x3C00 (1.0 in float16) nor 0x3F80 (1.0 in bfloat16).

Importing this module needs no device; tests/test_offset_views_cpu.py checks that the case list
below reaches what it was written for, tests/test_offset_views.py runs it."""

import torch

CANARY = 0xA5
GUARD = 4096                 # bytes of the arena on either side of where a view may start / end
SPAN = 2048                  # bytes of one wave's window, in every format

# bytes modulo 2 048.  int8: shifts on both sides of the 1 KiB half-window, the smallest one that
# is not zero and the largest.  16-bit formats: 16, 48, 496, 1040 and 2032 are element shifts that
# are odd multiples of 8 - a 16-byte chunk of the image straddles the output's first element -,
# the others are multiples of 16.
RESIDUES = (0, 16, 32, 48, 496, 1024, 1040, 2016, 2032)
STRADDLING = tuple(r for r in RESIDUES if r % 32 == 16)
assert STRADDLING == (16, 48, 496, 1040, 2032)

FORMATS = ((0, torch.int8), (1, torch.float16), (2, torch.bfloat16))      # CAMPX_OBS_*
DTYPES = tuple(d for _, d in FORMATS)

# What the device tests render, restated here so that the case list can be examined without a
# device: (layers, rows, cols, states of the table) of each game - tests/test_offset_views.py asserts
# them of the games it builds - and every row count it asks for.
WIDE_GAMES = {'maze': (6, 16, 16, 159), 'pickups': (5, 4, 9, 470), 'variants': (6, 4, 8, 51)}
LONG_ROWS = {'maze_15x17': (6, 15, 17, 156)}         # rows of 1 530 bytes: longer than a 16-bit span
ONE_CELL_GAMES = {'boat_race': (7, 5, 5), 'sokoban': (5, 6, 6), 'wall_world': (5, 10, 10)}
WINDOW_ROWS = (1, 3, 65, 257)
GATHER_ROWS = (1, 3, 65)
STATE_ROWS = (1, 65)
BATCH = 257                  # tests/test_render_states.py's games
TRACE_FRAMES = 2

CORNER = (-1, -2)            # a fixed window that hangs off the board's top-left corner ...
CORNER_SHAPE = (3, 4)        # ... of this size


def odd_window(L, H, W):
  """tests/test_windows.py `_odd_window`: a window whose L*h*w is not a multiple of 16."""
  for h, w in ((3, 5), (1, 17), (5, 7), (3, 3)):
    if L * h * w >= 16 and (L * h * w) % 16 and h <= 2 * H - 1 and w <= 2 * W - 1:
      return h, w
  raise AssertionError('no such window for {} layers'.format(L))


def window_shapes(L, H, W):
  """(h, w) of the windows the device tests render for an L x H x W game."""
  return ((3, 3), odd_window(L, H, W), (2 * H - 1, 2 * W - 1), CORNER_SHAPE)


def plan_cases():
  """Every (plan, row length, rows) the device tests launch gather_kernel ('gather') or
  window_kernel ('windows') with; each in every format at every residue."""
  cases = set()
  for L, H, W, S in WIDE_GAMES.values():
    for h, w in window_shapes(L, H, W):
      for N in WINDOW_ROWS + (STATE_ROWS[-1], S, TRACE_FRAMES * BATCH):
        cases.add(('windows', L * h * w, N))
  for L, H, W, S in list(WIDE_GAMES.values()) + list(LONG_ROWS.values()):
    for N in GATHER_ROWS:
      cases.add(('gather', L * H * W, N))
  for L, H, W in ONE_CELL_GAMES.values():
    for N in GATHER_ROWS:
      cases.add(('gather', L * H * W, N))
  return sorted(cases)


def arena_view(shape, dtype, residue, device, skew=0):
  """(view, arena, start): `view` is `shape` x `dtype` over arena[start:start + nbytes], its
  address `residue` modulo 2 048 (plus `skew` bytes, for a view that is NOT 16-byte aligned);
  every byte of the arena is 0xA5."""
  assert 0 <= residue < SPAN and residue % 16 == 0 and 0 <= skew < 16
  numel = 1
  for n in shape:
    numel *= int(n)
  size = numel * torch.empty((), dtype=dtype).element_size()
  arena = torch.full((size + 2 * GUARD,), CANARY, dtype=torch.uint8, device=device)
  first = GUARD - SPAN
  start = first + (residue - (arena.data_ptr() + first)) % SPAN + skew
  assert first <= start < GUARD + 16
  view = arena[start:start + size].view(dtype).view(tuple(shape))
  assert view.data_ptr() == arena.data_ptr() + start
  assert view.data_ptr() % SPAN == residue + skew
  assert view.is_contiguous() and view.numel() == numel
  return view, arena, start


def untouched(arena, start, nbytes):
  """Every byte of the arena outside [start, start + nbytes) is still 0xA5."""
  return bool((arena[:start] == CANARY).all()) and bool((arena[start + nbytes:] == CANARY).all())


def all_canary(arena):
  return bool((arena == CANARY).all())


def nbytes(view):
  return view.numel() * view.element_size()
