"""`campx_wide_policy_update_launch` (include/campx_hip.h) checks every argument on the host before
any device call: the refusals the header documents, through ctypes, without a GPU - no call here
gets as far as a launch."""

import ctypes

from campx_amd import _hip, gamespec

EINVAL, ESPEC = -1, -2
P = 0x7f0000001000          # a plausible, aligned, never dereferenced device address
INT64_MAX = (1 << 63) - 1


def _wide_spec():
  spec = gamespec.CampxWideSpec()
  spec.magic, spec.version = gamespec.SPEC_MAGIC, gamespec.SPEC_VERSION
  spec.rows = spec.cols = 16
  spec.n_layers, spec.n_dyn, spec.n_states = 3, 1, 1
  spec.dyn_layer[0] = 1
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == 0
  return spec


def test_the_entry_is_exported_and_bound():
  assert 'campx_wide_policy_update_launch' in _hip.EXPORTS
  assert _hip.lib.campx_wide_policy_update_launch.restype is ctypes.c_int32


def test_policy_update_checks_every_argument_before_any_device_call():
  spec, B, T = _wide_spec(), 64, 5
  call = _hip.lib.campx_wide_policy_update_launch

  def run(spec_p=True, tables=P, pos=P, done=P, policy=P, trace=P, actions=P, states=P, B=B, T=T,
          pitch=0, perf=None, seed=7, first_frame=0):
    st = _hip.CampxState(pos, done, None, None)
    out = _hip.CampxOutputs()
    out.trace, out.scalar_pitch, out.perf = trace, pitch, perf
    return call(ctypes.byref(spec) if spec_p else None, tables, st, policy, seed, first_frame, out,
                actions, states, B, T, 0, None)
  assert run(spec_p=False) == EINVAL
  for name in ('tables', 'pos', 'done', 'policy', 'trace', 'actions'):
    assert run(**{name: None}) == EINVAL, name
  assert run(B=0) == EINVAL and run(B=-4) == EINVAL and run(B=1 << 32) == EINVAL
  assert run(T=0) == EINVAL and run(T=-1) == EINVAL
  assert run(first_frame=-1) == EINVAL
  assert run(first_frame=INT64_MAX) == EINVAL and run(first_frame=INT64_MAX - T + 1) == EINVAL
  assert run(trace=P + 1) == EINVAL and run(pos=P + 2) == EINVAL
  assert run(policy=P + 2) == EINVAL and run(states=P + 1) == EINVAL and run(states=P + 2) == EINVAL
  assert run(pitch=B - 1) == EINVAL
  assert run(perf=P) == EINVAL            # a game without a hidden performance
  spec.magic ^= 1
  assert run() == ESPEC
  spec.magic ^= 1
  spec.n_states = 0
  assert run() == ESPEC
