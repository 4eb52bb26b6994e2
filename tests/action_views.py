"""int8 action streams at chosen BYTE addresses, between guards, with an exact count of bad ids.

The kernels that read an action stream do so with address-dependent code: csrc/k_update.hip's
`ActionLoader` with 16-byte loads at `actions + row * B + e` (aligned only when B % 16 == 0 AND the
tensor's base is), rows clamped past T, the batch's last partial group of 16 redirected to "the
buffer's last 16 bytes" and shifted down, byte loads when T * B < 16; `stage_actions()`, the step,
shape and state-table kernels and `check_actions_kernel` each in their own way.  A fresh allocation
is a multiple of 512 bytes followed by whatever the allocator left behind.  `action_view()` puts a
stream at any address modulo 16 inside an arena (tests/offset_views.py `arena_view(skew=)`) whose
other bytes all hold one of two fills:

  0xA5  -91 as int8, a bad id: a stray byte that is COUNTED shows in the count;
  0x01  "right", a legal move: a stray byte that is USED shows in positions, rewards, observations.

`streams()` makes a clean stream and a dirty one - bad ids forced where the loader's branches meet -
with the reference for "bad ids act as stay and are counted": `cleaned = where(bad, 4, dirty)` for
the oracle (which refuses a bad id outright) and numpy's count.  `loader_paths()` restates
`ActionLoader::issue()` / `land()`'s address arithmetic, so that tests/test_action_views_cpu.py can
assert, without a device, that the case lists below reach every branch.

Importing this module needs no device."""

import numpy as np
import torch

import offset_views as ov

FILL_BAD, FILL_MOVE = 0xA5, 0x01
FILLS = (FILL_BAD, FILL_MOVE)
OFFSETS = (0, 1, 7, 8, 15)
BAD_IDS = (5, 9, 127, -1, -128)
STAY = 4

# The smallest shapes at which each branch of the loader exists: T * B of 15 and 16 exactly (T = 3 or
# 1 at B = 5, 15, 16), a one-environment batch, both sides of a 16-group, of a 256-environment
# workgroup and of the 64-frame chunk.
FRAMES = (1, 2, 3, 63, 64, 65, 129)
BATCHES = (1, 5, 15, 16, 17, 31, 255, 256, 257, 271, 273)
FEW_FRAMES = (1, 3, 65)                       # what the pair and tuple games and the big workgroups run
BIG_BATCHES = (511, 512, 513, 527)            # around one 512-environment workgroup
# ... and, with big_wgs=0 (512-environment workgroups at EVERY batch), the shapes at which their
# loader goes byte by byte: T * B of 1, 3, 5 and 15, and 45 on the other side of 16
BIG_TINY_FRAMES = (1, 3)
BIG_TINY_BATCHES = (1, 5, 15)


def big_cases():
  """(T, B) of every launch tests/action_views_big_check.py runs on 512-environment workgroups."""
  return ([(T, B) for T in FEW_FRAMES for B in BIG_BATCHES if B >= 512] +
          [(T, B) for T in BIG_TINY_FRAMES for B in BIG_TINY_BATCHES])
# rollout_deferred(): the issue's batches, none of which the shared launch takes (it wants a batch's
# frame - 175 bytes an environment for the boat race, 180 for sokoban - to be whole 16-byte chunks),
# and the smallest that it does take: with a partial group of 4 on either side of a workgroup for
# sokoban; the boat race's are multiples of 16, whose groups are all whole
DEFERRED_BATCHES = (17, 257, 273)
DEFERRED_SHARED = {'boat_race': (272,), 'sokoban': (20, 260)}
# the other readers
STAGED_FRAMES = (1, 15, 16, 17, 65)           # both sides of stage_actions()'s 16-row split
STAGED_BATCHES = (1, 63, 65, 257)
# Hello World: the issue's 1, 5, 65, 130 give frames that are no whole 16-byte chunks, which the
# frame-major path does not take (tests/test_shape_parity.py); 4 and 68 are the smallest that do,
# with one wave and with two
SHAPE_BATCHES = (1, 4, 5, 65, 68, 130)
SHAPE_FRAME_MAJOR = (4, 68)
SHAPE_FRAMES = (1, 17, 65)
CHECK_SIZES = (1, 15, 16, 4099)

K_CHUNK = 64                                  # csrc/campx_common.hip.h kChunk
PATHS = ('whole', 'partial', 'partial_shifted', 'bytes', 'row_clamped', 'odd_T', 'second_chunk')


def offsets_for(T, B, offsets=OFFSETS):
  """`offsets`, and for a batch that is no multiple of 16 the one that makes `data_ptr() + T * B` a
  multiple of 16: the stream's last byte is then the last of an aligned 16, the guard starts on
  the next - where a 16-byte load one byte too far would still be "aligned"."""
  if B % 16 == 0:
    return tuple(offsets)
  return tuple(sorted(set(offsets) | {(-T * B) % 16}))


def action_view(a, byte_offset, fill, device):
  """(view, arena, start): the numpy stream `a` (int8 [T, B] or [B]) as a contiguous int8 tensor
  with `data_ptr() % 16 == byte_offset` inside a uint8 arena, at least 4 096 bytes on both sides,
  every byte of which outside the view is `fill`."""
  a = np.ascontiguousarray(a, dtype=np.int8)
  # arena_view() may start a view 2 048 bytes into its arena: ask for one a window longer on both
  # sides and take the middle
  _, arena, first = ov.arena_view((a.size + 2 * ov.SPAN,), torch.int8, 0, device, skew=byte_offset)
  start = first + ov.SPAN
  arena.fill_(fill)
  view = arena[start:start + a.size].view(torch.int8).view(a.shape)
  view.copy_(torch.from_numpy(a))
  assert view.data_ptr() == arena.data_ptr() + start and view.data_ptr() % 16 == byte_offset
  assert view.is_contiguous()
  assert start >= ov.GUARD and arena.numel() - (start + a.size) >= ov.GUARD
  return view, arena, start


def guards_hold(arena, start, nbytes, fill):
  """Every byte of the arena outside [start, start + nbytes) is `fill`."""
  return bool((arena[:start] == fill).all()) and bool((arena[start + nbytes:] == fill).all())


def forced_positions(T, B):
  """(t, e) of the bad ids `streams()` forces: the four corners, every environment of the batch's
  last partial group of 16 in the last row and in row 0, and the first environment of row 1 - the
  byte right behind a partial group's load of row 0."""
  at = {(0, 0), (0, B - 1), (T - 1, 0), (T - 1, B - 1)}
  if B % 16:
    for e in range(B - B % 16, B):
      at |= {(T - 1, e), (0, e)}
  if T > 1:
    at.add((1, 0))
  return sorted(at)


def streams(T, B, seed):
  """dict(clean, dirty, cleaned, n_bad) of int8 [T, B] streams: uniform ids 0..4; the same with
  bad ids at `forced_positions()` and at about 3 % of the rest, laid over "stay" and moves alike;
  the dirty one with every bad id replaced by 4; how many there are."""
  rng = np.random.RandomState(seed)
  clean = rng.randint(0, 5, size=(T, B)).astype(np.int8)
  where = rng.random_sample((T, B)) < 0.03
  for t, e in forced_positions(T, B):
    where[t, e] = True
  ids = rng.choice(np.array(BAD_IDS, dtype=np.int8), size=(T, B))
  dirty = np.where(where, ids, clean).astype(np.int8)
  bad = (dirty < 0) | (dirty > 4)
  assert np.array_equal(bad, where)
  cleaned = np.where(bad, STAY, dirty).astype(np.int8)
  return dict(clean=clean, dirty=dirty, cleaned=cleaned, n_bad=int(bad.sum()))


def loader_paths(T, B, envs):
  """(paths, shifts): which branches of `ActionLoader<envs, .>::issue()` / `land()` a launch of T
  frames of B environments reaches (names of `PATHS`), and the distances `shift_down()` is called
  with.  Asserts on the way the loader's own contract: every load lies inside the stream's T * B
  bytes."""
  assert envs in (256, 512) and T >= 1 and B >= 1
  vec_per_row = envs // 16
  last = T * B - 16
  paths, shifts = set(), set()

  def inside(at, n):
    assert 0 <= at and at + n <= T * B, (T, B, envs, at, n)

  for wg in range((B + envs - 1) // envs):
    env0 = wg * envs
    for t0 in range(0, T, K_CHUNK):          # the prologue's chunk, then every `t_next < T`
      if t0:
        paths.add('second_chunk')
      for rp in range(K_CHUNK // 2):
        for q in range(vec_per_row):
          e = env0 + 16 * q
          here = e + 16 <= B
          rows = (t0 + 2 * rp, t0 + 2 * rp + 1)
          if last >= 0:                      # issue(): every lane loads, clamped
            for row in rows:
              at = min(min(row, T - 1) * B + (e if here else 0), last)
              inside(at, 16)
          if not here and e >= B:
            continue                         # no environment: neutral bytes, nothing counted
          if rows[0] < T <= rows[1]:
            paths.add('odd_T')
          for row in rows:
            if row >= T:
              paths.add('row_clamped')
              continue
            if here:
              paths.add('whole')
              continue
            at = row * B + e
            if last < 0:
              paths.add('bytes')
              inside(at, B - e)
            elif at > last:
              paths.add('partial_shifted')
              shifts.add(at - last)
              assert 0 < at - last < 16 and at - last + (B - e) <= 16
              inside(last, 16)
            else:
              paths.add('partial')
              inside(at, 16)
  return paths, shifts
