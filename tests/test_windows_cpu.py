"""Observation windows, the parts that need no device: the tests' reference against a hand-worked
case, the launch arithmetic, every refusal of the launch validator, and `Window`'s resolution of
characters."""

import ctypes
import os

import numpy as np
import pytest
import torch

from campx_amd import _hip, gamespec
from campx_amd.windows import Window

import windows_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
P = 4096           # a non-NULL, 16-byte aligned "device address" nothing on the host ever follows


# ------------------------------------------------------------------ the reference itself

def test_reference_on_a_hand_worked_board():
  """A 2 x 3 board, two layers; layer 1 is the complement of layer 0.  A 3 x 3 window centred on
  each of the six cells: written out cell by cell from the rule."""
  board0 = [[1, 0, 1],
            [0, 1, 1]]
  full = torch.zeros((6, 2, 2, 3), dtype=torch.int8)
  full[:, 0] = torch.tensor(board0, dtype=torch.int8)
  full[:, 1] = 1 - full[:, 0]
  entries = torch.arange(6) | 0x8000              # (a `shows` bit changes nothing)
  r0, c0 = ref.centres(entries, 3, 6, 3, 3)
  assert r0.tolist() == [-1, -1, -1, 0, 0, 0] and c0.tolist() == [-1, 0, 1, -1, 0, 1]
  for pad in (None, 1, 0):
    got = ref.crop(full, r0, c0, 3, 3, pad)
    assert got.shape == (6, 2, 3, 3)
    for i in range(6):
      cy, cx = divmod(i, 3)
      for l in range(2):
        for y in range(3):
          for x in range(3):
            by, bx = cy - 1 + y, cx - 1 + x
            if 0 <= by < 2 and 0 <= bx < 3:
              want = board0[by][bx] if l == 0 else 1 - board0[by][bx]
            else:
              want = 1 if pad == l else 0
            assert int(got[i, l, y, x]) == want, (pad, i, l, y, x)
  # spelled out: the window round the top-left cell, layer 0, no padding
  assert ref.crop(full, r0, c0, 3, 3)[0, 0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 1]]
  # ... and the wall's layer set off the board
  assert ref.crop(full, r0, c0, 3, 3, 0)[0, 0].tolist() == [[1, 1, 1], [1, 1, 0], [1, 0, 1]]
  # a fixed window that is the board is the board; one far outside is padding
  assert torch.equal(ref.crop(full, 0, 0, 2, 3), full)
  assert torch.equal(ref.crop(full, -9, 7, 2, 2, 1)[:, 1], torch.ones((6, 2, 2), dtype=torch.int8))
  # the cell is clamped to the board's last one
  r0, c0 = ref.centres(torch.tensor([0x3ff, 5]), 3, 6, 3, 3)
  assert r0.tolist() == [0, 0] and c0.tolist() == [1, 1]


# ------------------------------------------------------------------ launch arithmetic

WAVES = 2
ROW_CAP = {0: 192, 1: 128, 2: 128}     # rows a wave can stage (k_window.hip kRowIter * 64)


def _restated(N, R, fmt, addr):
  l = 0
  while (1 << l) < R:
    l += 1
  m = ((1 << 32) * ((1 << l) - R)) // R + 1
  wspan = 1024 if fmt else 2048
  total = N * R
  shift = (addr >> (1 if fmt else 0)) & (wspan - 1)
  span = wspan * WAVES
  grid = ((total + shift + span - 1) // span + 7) & ~7
  return [m & 0xffffffff, min(l, 1), max(l - 1, 0), total, shift, grid, wspan, WAVES]


def _row_lengths():
  """Every L*h*w from 16 to 16 * 63 * 63 that some (L <= 16, h <= 63, w <= 63) produces."""
  hw = np.unique(np.outer(np.arange(1, 64), np.arange(1, 64)))
  rw = np.unique(np.outer(np.arange(1, 17), hw))
  return [int(r) for r in rw if r >= 16]


def test_windows_plan_is_the_restated_division_for_every_row_length():
  lengths = _row_lengths()
  assert lengths[0] == 16 and lengths[-1] == 16 * 63 * 63 and len(lengths) > 5000
  out = (ctypes.c_int64 * 8)()
  addrs = (4096, 4096 + 16, 4096 + 2032, 4096 + 1008)
  for j, R in enumerate(lengths):
    most = ((1 << 32) - 65536 - 1) // R
    for k, N in enumerate((1, 1237, most)):
      fmt, addr = (j + k) % 3, addrs[(j + k) % 4]
      assert _hip.lib.campx_wide_render_windows_plan(N, R, fmt, addr, out) == 0
      want = _restated(N, R, fmt, addr)
      assert list(out) == want, (N, R, fmt, addr, list(out), want)
    m, sh1, sh2, total, shift, grid, wspan, waves = want
    assert total <= (1 << 32) - 65536 - 1 and total + shift + wspan * waves < (1 << 32)
    assert grid % 8 == 0 and grid * waves * wspan >= total + shift > (grid - 8) * waves * wspan
    # the division wherever the kernel divides: round every multiple of R near both ends
    q = np.concatenate([np.arange(0, 20), np.arange(most - 20, most + 2)]).astype(np.uint64)
    n = np.concatenate([q * np.uint64(R), q * np.uint64(R) + np.uint64(R - 1),
                        (q * np.uint64(R))[1:] - np.uint64(1),
                        np.array([(1 << 32) - 1, (1 << 32) - 65536], dtype=np.uint64)])
    n = n[n < (1 << 32)]
    hi = (n * np.uint64(m)) >> np.uint64(32)
    quot = (((n - hi) >> np.uint64(sh1)) + hi) >> np.uint64(sh2)
    assert np.array_equal(quot, n // np.uint64(R)), R
    for f, span in ((0, 2048), (1, 1024), (2, 1024)):
      assert (span - 1) // R + 2 + 1 <= ROW_CAP[f], (R, f)


def test_windows_plan_refusals():
  out = (ctypes.c_int64 * 8)()
  plan = _hip.lib.campx_wide_render_windows_plan
  assert plan(10, 245, 0, 4096, None) == EINVAL
  for N, R, fmt, addr in ((0, 245, 0, 4096), (10, 15, 0, 4096), (10, 245, 3, 4096), (10, 245, -1, 4096),
                          (10, 245, 0, 4100), (((1 << 32) - 65536 - 1) // 245 + 1, 245, 0, 4096)):
    assert plan(N, R, fmt, addr, out) == EINVAL, (N, R, fmt, addr)
  assert plan(((1 << 32) - 65536 - 1) // 245, 245, 0, 4096, out) == 0


# ------------------------------------------------------------------ the launch validator

def _wide_spec():
  spec = gamespec.CampxWideSpec()
  spec.magic, spec.version = 0x58504d43, 1
  spec.rows = spec.cols = 16
  spec.n_layers, spec.n_dyn, spec.n_states = 3, 2, 7
  spec.dyn_layer[0], spec.dyn_layer[1] = 1, 2
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0
  return spec


def _request(kind, B, **changes):
  source = kind
  q = _hip.CampxWindows()
  q.source, q.idx64 = source, 1
  if source != _hip.WINDOWS_STATES:
    q.trace, q.n_planes, q.T, q.pitch, q.plane = P, 2, 10, B, 10 * B
  if source == _hip.WINDOWS_PAIRS:
    q.t_idx = q.e_idx = P
  if source == _hip.WINDOWS_STATES:
    q.state_ids = P
  q.N = 10 * B if source == _hip.WINDOWS_TRACE else 100
  q.h, q.w, q.anchor, q.thing, q.pad_layer = 5, 5, _hip.WINDOW_ON_THING, 1, 0
  q.obs_format, q.obs = 0, P
  for k, v in changes.items():
    setattr(q, k, v)
  return q


@pytest.mark.parametrize('source', [_hip.WINDOWS_PAIRS, _hip.WINDOWS_TRACE, _hip.WINDOWS_STATES])
def test_launch_checks_every_argument_before_any_device_call(source):
  """Every call below is refused: none reaches a device (there is none; `P` is no address)."""
  spec, B = _wide_spec(), 64
  call = _hip.lib.campx_wide_render_windows_launch
  ok = _request(source, B)

  def run(q, spec_p=ctypes.byref(spec), tables=P, loc=P):
    return call(spec_p, tables, loc, ctypes.byref(q) if q is not None else None, B, None)
  assert run(ok, spec_p=None) == EINVAL and run(ok, tables=None) == EINVAL
  assert run(ok, loc=None) == EINVAL and run(None) == EINVAL
  assert run(ok, loc=P + 8) == EINVAL
  Rw = 3 * 5 * 5
  most = ((1 << 32) - 65536 - 1) // Rw
  bad = dict(
      null_obs=dict(obs=None), misaligned_obs=dict(obs=P + 8), misaligned_counter=dict(bad_count=P + 2),
      misaligned_flag=dict(bad_flag=P + 1),
      no_rows=dict(N=0), negative_rows=dict(N=-3), past_the_32_bit_bound=dict(N=most + 1),
      h_zero=dict(h=0), w_zero=dict(w=0), h_negative=dict(h=-1), h_past=dict(h=2 * 16), w_past=dict(w=2 * 16),
      row_below_16=dict(h=1, w=5), thing_past=dict(thing=2), thing_negative=dict(thing=-1),
      pad_past=dict(pad_layer=3), pad_below=dict(pad_layer=-2), anchor=dict(anchor=2),
      corner_far=dict(anchor=_hip.WINDOW_FIXED, r0=256), corner_far_left=dict(anchor=_hip.WINDOW_FIXED, c0=-256),
      format=dict(obs_format=3), source=dict(source=3), source_negative=dict(source=-1))
  if source == _hip.WINDOWS_STATES:
    bad.update(misaligned_ids=dict(state_ids=P + 4))
  else:
    bad.update(null_trace=dict(trace=None), misaligned_trace=dict(trace=P + 1), no_frames=dict(T=0),
               pitch_below_batch=dict(pitch=B - 1), planes_too_few=dict(n_planes=1),
               planes_too_many=dict(n_planes=3), planes_overlap=dict(plane=10 * B - 1),
               frames_past=dict(T=(1 << 40) // B + 1, plane=1 << 50))
  if source == _hip.WINDOWS_PAIRS:
    bad.update(null_t=dict(t_idx=None), null_e=dict(e_idx=None), misaligned_idx=dict(t_idx=P + 4))
  if source == _hip.WINDOWS_TRACE:
    bad.update(rows_not_the_trace=dict(N=10 * B - 1))
  for what, changes in bad.items():
    assert run(_request(source, B, **changes)) == EINVAL, what
  if source != _hip.WINDOWS_STATES:
    assert call(ctypes.byref(spec), P, P, ctypes.byref(ok), 0, None) == EINVAL
  # the largest window and the bound itself pass every check: only the missing device is left, so
  # they are not launched here - the plan call takes the same arithmetic
  out = (ctypes.c_int64 * 8)()
  assert _hip.lib.campx_wide_render_windows_plan(most, Rw, 0, P, out) == 0
  # a spec that is no spec is refused as one
  broken = _wide_spec()
  broken.magic = 0
  assert run(ok, spec_p=ctypes.byref(broken)) == -2


def test_the_new_entry_points_are_declared_bound_and_documented():
  with open(os.path.join(REPO, 'include', 'campx_hip.h')) as f:
    header = f.read()
  with open(os.path.join(REPO, 'INTEGRATION.md')) as f:
    guide = f.read()
  for name in ('campx_wide_render_windows_launch', 'campx_wide_render_windows_plan'):
    assert name in _hip.EXPORTS and hasattr(_hip.lib, name)
    assert name + '(' in header and name in guide
  assert 'typedef struct CampxWindows' in header
  assert 'wide_render_windows' in _hip.OP_NAMES
  assert torch.ops.campx.wide_render_windows.default._schema.returns == []
  from campx_amd import build
  assert 'k_window' in build.UNITS


# ------------------------------------------------------------------ Window

def _hand_built():
  spec = gamespec.CampxWideSpec()
  spec.rows, spec.cols, spec.n_layers, spec.n_dyn = 16, 12, 5, 2
  spec.dyn_layer[0], spec.dyn_layer[1] = 3, 1
  return [' ', 'B', '#', 'P', '@'], spec


def test_window_resolves_characters_against_the_game():
  chars, spec = _hand_built()
  assert Window(5, 5, 'P').resolve(chars, spec) == (0, 0, 0, -1)
  assert Window(5, 7, 'B', pad='#').resolve(chars, spec) == (1, 0, 0, 2)
  assert Window(3, 4, (-1, 2), pad=' ').resolve(chars, spec) == (-1, -1, 2, 0)
  assert Window(31, 23, (0, 0)).resolve(chars, spec).thing == -1
  with pytest.raises(ValueError, match="no character 'Q'"):
    Window(5, 5, 'Q').resolve(chars, spec)
  with pytest.raises(ValueError, match=r"'@' is scenery.*tracked things are 'P' 'B'"):
    Window(5, 5, '@').resolve(chars, spec)
  with pytest.raises(ValueError, match=r"'#' is scenery"):
    Window(5, 5, '#').resolve(chars, spec)
  with pytest.raises(ValueError, match="no character 'Q' to pad with"):
    Window(5, 5, 'P', pad='Q').resolve(chars, spec)
  with pytest.raises(ValueError, match='at most 31 x 23'):
    Window(32, 5, 'P').resolve(chars, spec)
  with pytest.raises(ValueError, match='at most 31 x 23'):
    Window(5, 24, 'P').resolve(chars, spec)
  with pytest.raises(ValueError, match='below the 16'):
    Window(1, 3, 'P').resolve(chars, spec)
  for bad in (dict(height=0, width=3, centre='P'), dict(height=3, width=True, centre='P'),
              dict(height=3, width=3, centre='PP'), dict(height=3, width=3, centre=(1,)),
              dict(height=3, width=3, centre=(1.5, 2)), dict(height=3, width=3, centre=(0, 300)),
              dict(height=3, width=3, centre='P', pad='##'), dict(height=3, width=3, centre=None)):
    with pytest.raises(ValueError, match='Window'):
      Window(**bad)
