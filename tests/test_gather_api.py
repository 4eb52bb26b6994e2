"""Trace-only rollouts and the gather render, as far as they can be checked without a GPU: the
ops' registration, the C entries' argument checks (every one returns before any device call),
and the gather launcher's window / row arithmetic restated and checked over every row length."""

import ctypes
import os

import numpy as np
import pytest
import torch

from campx_amd import _hip, gamespec
from campx_amd.games import boat_race, sokoban

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ('wide_update', 'render_gather', 'wide_render_gather')
NEW_ENTRIES = ('campx_wide_update_launch', 'campx_render_gather_launch',
               'campx_wide_render_gather_launch', 'campx_render_gather_plan')
EINVAL = -1


def _spec_tensor():
  spec = gamespec.lower(gamespec.describe(boat_race.build()))
  return torch.frombuffer(bytearray(gamespec.spec_bytes(spec)), dtype=torch.uint8)


def test_new_ops_are_registered_with_in_place_schemas():
  for name in NEW_OPS:
    assert name in _hip.OP_NAMES
    op = getattr(torch.ops.campx, name).default
    assert op._schema.returns == []
  s = str(torch.ops.campx.render_gather.default._schema)
  for part in ('Tensor trace', 'Tensor t_idx', 'Tensor e_idx', 'Tensor(a!) obs', 'Tensor(b!)? bad_count',
               'Tensor(c!)? bad_flag'):
    assert part in s, s
  s = str(torch.ops.campx.wide_render_gather.default._schema)
  assert 'Tensor tables' in s and 'Tensor(a!) obs' in s
  s = str(torch.ops.campx.wide_update.default._schema)
  for part in ('Tensor(a!) state', 'Tensor(b!) done', 'Tensor(h!) trace', 'bool reset_first'):
    assert part in s, s
  assert 'obs' not in s and 'board' not in s


def test_cpu_tensors_fail_loudly():
  spec = _spec_tensor()
  trace = torch.zeros((1, 3, 8), dtype=torch.uint8)
  idx = torch.zeros((4,), dtype=torch.int64)
  obs = torch.zeros((4, 7, 5, 5), dtype=torch.int8)
  with pytest.raises((NotImplementedError, RuntimeError)) as e:
    torch.ops.campx.render_gather(spec, spec, trace, idx, idx, obs, None, None)
  assert 'CPU' in str(e.value)
  with pytest.raises((NotImplementedError, RuntimeError)) as e:
    torch.ops.campx.wide_render_gather(spec, spec, trace.to(torch.int16), idx, idx, obs, None, None)
  assert 'CPU' in str(e.value)
  state = torch.zeros((8,), dtype=torch.int32)
  done = torch.zeros((8,), dtype=torch.uint8)
  acts = torch.zeros((3, 8), dtype=torch.int8)
  with pytest.raises((NotImplementedError, RuntimeError)) as e:
    torch.ops.campx.wide_update(spec, spec, state, done, None, acts, None, None, None, None,
                                trace.to(torch.int16), None, None, False)
  assert 'CPU' in str(e.value)


def test_meta_kernels_trace_without_a_device():
  spec = _spec_tensor().to('meta')
  trace = torch.zeros((1, 3, 8), dtype=torch.uint8, device='meta')
  idx = torch.zeros((4,), dtype=torch.int64, device='meta')
  obs = torch.zeros((4, 7, 5, 5), dtype=torch.int8, device='meta')
  assert torch.ops.campx.render_gather(spec, spec, trace, idx, idx, obs, None, None) is None
  assert torch.ops.campx.wide_render_gather(spec, spec, trace.to(torch.int16), idx, idx, obs, None,
                                            None, True) is None
  state = torch.zeros((8,), dtype=torch.int32, device='meta')
  done = torch.zeros((8,), dtype=torch.uint8, device='meta')
  acts = torch.zeros((3, 8), dtype=torch.int8, device='meta')
  assert torch.ops.campx.wide_update(spec, spec, state, done, None, acts, None, None, None, None,
                                     trace.to(torch.int16), None, None, False) is None


def test_the_new_entries_are_in_the_library_the_header_and_the_integration_guide():
  with open(os.path.join(REPO, 'include', 'campx_hip.h')) as f:
    header = f.read()
  with open(os.path.join(REPO, 'INTEGRATION.md')) as f:
    guide = f.read()
  for name in NEW_ENTRIES:
    assert name in _hip.EXPORTS
    assert hasattr(_hip.lib, name)
    assert name + '(' in header
    assert name in guide
  assert 'typedef struct CampxGather' in header


# ------------------------------------------------------------------ argument checks

P = 4096           # a non-NULL, 16-byte aligned "device address" nothing on the host ever follows


def _one_cell_spec():
  spec = gamespec.lower(gamespec.describe(sokoban.build()))     # two movers
  assert _hip.lib.campx_spec_validate(ctypes.byref(spec)) == 0
  spec.render_valid = 1       # (what campx_spec_compile() sets once the render tables are filled)
  return spec


def _wide_spec():
  spec = gamespec.CampxWideSpec()
  spec.magic, spec.version = 0x58504d43, 1
  spec.rows = spec.cols = 16
  spec.n_layers, spec.n_dyn, spec.n_states = 3, 1, 1
  spec.dyn_layer[0] = 1
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0
  return spec


def _request(planes, B, R, **changes):
  g = _hip.CampxGather()
  g.trace, g.n_planes, g.T, g.pitch, g.plane = P, planes, 10, B, 10 * B
  g.t_idx = g.e_idx = P
  g.idx64, g.obs_format, g.N, g.obs = 1, 0, 100, P
  for k, v in changes.items():
    setattr(g, k, v)
  return g


def _bad_requests(planes, B, R):
  most = ((1 << 32) - 65536 - 1) // R
  return dict(
      null_trace=dict(trace=None), null_t=dict(t_idx=None), null_e=dict(e_idx=None), null_obs=dict(obs=None),
      no_rows=dict(N=0), negative_rows=dict(N=-3), no_frames=dict(T=0),
      misaligned_obs=dict(obs=P + 8), misaligned_idx=dict(t_idx=P + 4),
      pitch_below_batch=dict(pitch=B - 1),
      planes_too_few=dict(n_planes=planes - 1), planes_too_many=dict(n_planes=planes + 1),
      planes_overlap=dict(n_planes=planes, plane=10 * B - 1) if planes > 1 else dict(N=0),
      past_the_32_bit_bound=dict(N=most + 1),
      format=dict(obs_format=3))


def test_render_gather_checks_every_argument_before_any_device_call():
  spec, B = _one_cell_spec(), 64
  R = spec.n_layers * spec.rows * spec.cols
  call = _hip.lib.campx_render_gather_launch
  ok = _request(2, B, R)
  assert call(None, P, ctypes.byref(ok), B, None) == EINVAL
  assert call(ctypes.byref(spec), None, ctypes.byref(ok), B, None) == EINVAL
  assert call(ctypes.byref(spec), P, None, B, None) == EINVAL
  assert call(ctypes.byref(spec), P, ctypes.byref(ok), 0, None) == EINVAL
  for what, changes in _bad_requests(2, B, R).items():
    assert call(ctypes.byref(spec), P, ctypes.byref(_request(2, B, R, **changes)), B, None) == EINVAL, what
  # a spec whose render tables were never filled: refused as a spec, not as an argument
  small = gamespec.lower(gamespec.describe(boat_race.build()))
  small.render_valid = 0
  assert call(ctypes.byref(small), P, ctypes.byref(_request(1, B, R)), B, None) == -2   # CAMPX_ESPEC: no tables


def test_wide_render_gather_checks_every_argument_before_any_device_call():
  spec, B = _wide_spec(), 64
  R = spec.n_layers * spec.rows * spec.cols
  call = _hip.lib.campx_wide_render_gather_launch
  ok = _request(1, B, R)
  assert call(None, P, ctypes.byref(ok), B, None) == EINVAL
  assert call(ctypes.byref(spec), None, ctypes.byref(ok), B, None) == EINVAL
  assert call(ctypes.byref(spec), P, None, B, None) == EINVAL
  assert call(ctypes.byref(spec), P, ctypes.byref(ok), -1, None) == EINVAL
  for what, changes in _bad_requests(1, B, R).items():
    assert call(ctypes.byref(spec), P, ctypes.byref(_request(1, B, R, **changes)), B, None) == EINVAL, what
  assert call(ctypes.byref(spec), P, ctypes.byref(_request(1, B, R, trace=P + 1)), B, None) == EINVAL
  # a piece mask is one more plane: the things' planes alone are then not the game's count
  spec.n_pieces = 2
  spec.piece_cell[0], spec.piece_cell[1] = 17, 18
  spec.piece_layer[0] = spec.piece_layer[1] = 2
  assert call(ctypes.byref(spec), P, ctypes.byref(ok), B, None) == EINVAL


def test_wide_update_checks_every_argument_before_any_device_call():
  spec, B, T = _wide_spec(), 64, 5
  call = _hip.lib.campx_wide_update_launch

  def run(spec_p=True, tables=P, pos=P, done=P, actions=P, trace=P, B=B, T=T, pitch=0, perf=None):
    st = _hip.CampxState(pos, done, None, None)
    out = _hip.CampxOutputs()
    out.trace, out.scalar_pitch, out.perf = trace, pitch, perf
    return call(ctypes.byref(spec) if spec_p else None, tables, st, actions, out, B, T, 0, None)
  assert run(spec_p=False) == EINVAL
  for name in ('tables', 'pos', 'done', 'actions', 'trace'):
    assert run(**{name: None}) == EINVAL, name
  assert run(B=0) == EINVAL and run(T=0) == EINVAL and run(T=-1) == EINVAL
  assert run(trace=P + 1) == EINVAL and run(pos=P + 2) == EINVAL
  assert run(pitch=B - 1) == EINVAL
  assert run(perf=P) == EINVAL            # a game without a hidden performance


# ------------------------------------------------------------------ launch arithmetic

WAVES = 2
ROW_CAP = {0: 192, 1: 128, 2: 128}     # rows whose indices a wave can stage (k_gather.hip kRowIter * 64)


def _plan(N, R, fmt, addr):
  out = (ctypes.c_int64 * 8)()
  rc = _hip.lib.campx_render_gather_plan(N, R, fmt, addr, out)
  return rc, list(out)


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


def test_gather_plan_refuses_what_the_kernel_cannot_take():
  out = (ctypes.c_int64 * 8)()
  assert _hip.lib.campx_render_gather_plan(10, 175, 0, 4096, None) == EINVAL
  for N, R, fmt, addr in ((0, 175, 0, 4096), (10, 15, 0, 4096), (10, 16 * 1024 + 1, 0, 4096),
                          (10, 175, 3, 4096), (10, 175, 0, 4100),
                          (((1 << 32) - 65536 - 1) // 175 + 1, 175, 0, 4096)):
    assert _hip.lib.campx_render_gather_plan(N, R, fmt, addr, out) == EINVAL, (N, R, fmt, addr)
  assert _hip.lib.campx_render_gather_plan(((1 << 32) - 65536 - 1) // 175, 175, 0, 4096, out) == 0


def test_gather_window_and_row_arithmetic_is_exact_for_every_row_length():
  """For every row length the kernels are launched for (16 bytes to 16 layers x 1 024 cells):
  the library's plan is the restated one; n / R by multiply-and-shift is exact wherever the
  kernel divides (window starts and ends, chunk offsets: any n below N * R + a window); the
  windows cover the output; and the rows a window overlaps fit the wave's staging area."""
  addrs = (4096, 4096 + 16, 4096 + 2032, 4096 + 1008)
  for R in range(16, 16 * 1024 + 1):
    most = ((1 << 32) - 65536 - 1) // R
    for k, N in enumerate((1, 1237, most)):
      fmt, addr = (R + k) % 3, addrs[(R + k) % 4]
      rc, got = _plan(N, R, fmt, addr)
      want = _restated(N, R, fmt, addr)
      assert rc == 0 and got == want, (N, R, fmt, addr, got, want)
    m, sh1, sh2, total, shift, grid, wspan, waves = want
    assert total < (1 << 32) - 65536 and total + shift + wspan * waves < (1 << 32)
    assert grid % 8 == 0 and grid * waves * wspan >= total + shift > (grid - 8) * waves * wspan
    # the division: around every multiple of R near both ends of the range, and at window edges
    q = np.concatenate([np.arange(0, 40), np.arange(most - 40, most + 2)]).astype(np.uint64)
    n = np.concatenate([q * np.uint64(R), q * np.uint64(R) + np.uint64(R - 1),
                        (q * np.uint64(R))[1:] - np.uint64(1),
                        np.arange(0, 1 << 32, 2048 * 4093, dtype=np.uint64),
                        np.array([(1 << 32) - 1, (1 << 32) - 65536], dtype=np.uint64)])
    n = n[n < (1 << 32)]
    hi = (n * np.uint64(m)) >> np.uint64(32)
    quot = (((n - hi) >> np.uint64(sh1)) + hi) >> np.uint64(sh2)
    assert np.array_equal(quot, n // np.uint64(R)), R
    # rows a window of `wspan` bytes overlaps, plus the one after it
    for f, span in ((0, 2048), (1, 1024), (2, 1024)):
      assert (span - 1) // R + 2 + 1 <= ROW_CAP[f], (R, f)
