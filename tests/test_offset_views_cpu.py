"""tests/offset_views.py without a device: that its case list reaches what it was written for -
through the two plan entry points, at every (row length, rows, format, residue) that
tests/test_offset_views.py launches gather_kernel and window_kernel with - and that `arena_view()`
delivers the address it is asked for between intact canaries."""

import ctypes

import pytest
import torch

from campx_amd import _hip

import offset_views as ov

BASE = 1 << 20               # a "device address" that is a multiple of every window span
PLANS = {'gather': 'campx_render_gather_plan', 'windows': 'campx_wide_render_windows_plan'}


def _planned():
  """(plan, R, N, fmt, residue) -> the library's plan_out, for the whole case list."""
  out = (ctypes.c_int64 * 8)()
  got = {}
  for plan, R, N in ov.plan_cases():
    for fmt, _ in ov.FORMATS:
      for residue in ov.RESIDUES:
        assert getattr(_hip.lib, PLANS[plan])(N, R, fmt, BASE + residue, out) == 0, (plan, R, N, fmt, residue)
        got[(plan, R, N, fmt, residue)] = list(out)
  return got


def test_the_case_list_is_what_the_device_file_needs():
  assert ov.RESIDUES == (0, 16, 32, 48, 496, 1024, 1040, 2016, 2032)
  assert all(r % 16 == 0 and 0 <= r < ov.SPAN for r in ov.RESIDUES)
  assert [d for _, d in ov.FORMATS] == [torch.int8, torch.float16, torch.bfloat16]
  assert [f for f, _ in ov.FORMATS] == [0, 1, 2]           # CAMPX_OBS_INT8, _F16, _BF16
  cases = ov.plan_cases()
  assert {p for p, _, _ in cases} == set(PLANS)
  assert all(R >= 16 and N >= 1 for _, R, N in cases)
  # a canary is no value a kernel writes
  assert ov.CANARY not in (0, 1) and ov.CANARY * 257 not in (0, 0x3C00, 0x3F80)


def test_shift_is_the_restated_one_at_every_case():
  for (plan, R, N, fmt, residue), out in _planned().items():
    wspan = 1024 if fmt else 2048
    assert out[6] == wspan and out[3] == N * R
    assert out[4] == (residue >> (1 if fmt else 0)) & (wspan - 1), (plan, R, N, fmt, residue, out)


@pytest.mark.parametrize('plan', sorted(PLANS))
@pytest.mark.parametrize('fmt', [f for f, _ in ov.FORMATS])
def test_the_cases_reach_every_path_of_the_first_window(plan, fmt):
  """Per kernel and format.  "One chunk in the first window": the output is 16-byte aligned, so
  the first window never holds fewer than 16 bytes (8 elements of a 16-bit format) of it; the
  case asked for is the one where it holds exactly that, and the rest lies in the next window."""
  wspan = 1024 if fmt else 2048
  chunk = 8 if fmt else 16               # image bytes of one 16-byte store
  seen = set()
  for (p, R, N, f, residue), out in _planned().items():
    if p != plan or f != fmt:
      continue
    total, shift = out[3], out[4]
    if total + shift < wspan:
      seen.add('inside one window')
    if wspan < total + shift <= 2 * wspan and wspan - shift == chunk:
      seen.add('one chunk in the first window')
    if total + shift > 2 * wspan:
      seen.add('three or more windows')
    if total % 16:
      seen.add('last chunk byte by byte')
    if fmt and total % 8:
      seen.add('last store element by element')
    if fmt and shift % 16 == 8:
      seen.add('straddling chunk')
      assert residue in ov.STRADDLING
    elif fmt:
      assert residue not in ov.STRADDLING
    if R > wspan:
      seen.add('a row longer than a span')
  want = {'inside one window', 'one chunk in the first window', 'three or more windows',
          'last chunk byte by byte'}
  if fmt:
    want |= {'straddling chunk', 'last store element by element'}
  # (gather_kernel's rows are whole boards: the longest here, 1 536 bytes, is past a 16-bit span
  # only; window_kernel's largest window is past both)
  if fmt or plan == 'windows':
    want.add('a row longer than a span')
  assert seen >= want, (plan, fmt, sorted(want - seen))


@pytest.mark.parametrize('dtype', ov.DTYPES)
def test_arena_view_on_cpu_tensors(dtype):
  size = torch.empty((), dtype=dtype).element_size()
  for residue in ov.RESIDUES:
    for shape in ((1, 3, 3, 3), (65, 5, 3, 5), (3, 2, 6, 31, 31)):
      view, arena, start = ov.arena_view(shape, dtype, residue, 'cpu')
      assert view.data_ptr() % ov.SPAN == residue and view.data_ptr() % 16 == 0
      assert view.dtype == dtype and tuple(view.shape) == shape and view.is_contiguous()
      assert arena.dtype == torch.uint8 and arena.numel() == view.numel() * size + 2 * 4096
      assert ov.nbytes(view) == view.numel() * size
      assert ov.all_canary(arena) and ov.untouched(arena, start, ov.nbytes(view))
      bits = view.view(torch.int16) if size == 2 else view
      assert bool((bits == (-0x5a5b if size == 2 else -0x5b)).all())       # 0xA5A5 / 0xA5, signed
      # the view IS the arena's bytes: writing it leaves the canaries, and only them
      view.zero_()
      assert ov.untouched(arena, start, ov.nbytes(view)) and not ov.all_canary(arena)
      assert int((arena != ov.CANARY).sum()) == ov.nbytes(view)
      # ... and a byte on either side of it is noticed
      for at in (start - 1, start + ov.nbytes(view), 0, arena.numel() - 1):
        arena[at] = 0
        assert not ov.untouched(arena, start, ov.nbytes(view)), at
        arena[at] = ov.CANARY
      assert ov.untouched(arena, start, ov.nbytes(view))


def test_a_skewed_view_is_not_16_byte_aligned():
  view, arena, start = ov.arena_view((65, 5, 3, 3), torch.int8, 16, 'cpu', skew=8)
  assert view.data_ptr() % 16 == 8 and ov.all_canary(arena)
  view, arena, start = ov.arena_view((65, 5, 3, 3), torch.float16, 2032, 'cpu', skew=2)
  assert view.data_ptr() % 16 == 2 and view.data_ptr() % ov.SPAN == 2034 and ov.all_canary(arena)
  # the plan entry points refuse such an address, as the launches do
  out = (ctypes.c_int64 * 8)()
  for name in PLANS.values():
    assert getattr(_hip.lib, name)(65, 45, 0, BASE + 16 + 8, out) == -1
    assert getattr(_hip.lib, name)(65, 45, 1, BASE + 16 + 2, out) == -1
