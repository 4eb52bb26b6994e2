"""What `campx_wide_reset_launch()`, `campx_wide_rollout_launch()` and `campx_wide_update_launch()`
refuse before they touch a device, and with which code: one argument wrong at a time on an
otherwise valid call, then two at once to say which check comes first.  The spec is a real one (a
synthetic table of three states on a 4x4 board, one thing); the device pointers are made-up
addresses that no host code reads.  No kernel is launched here."""

import ctypes

import pytest

import wide_table_reference as ref

OK, EINVAL, ESPEC = 0, -1, -2            # include/campx_hip.h
FAKE = 0x1000                            # 16-byte aligned, never read
B, L, HW = 8, 2, 16
R = L * HW
INT8, F16, BF16 = 0, 1, 2


@pytest.fixture(scope='module')
def table():
  from campx_amd import _hip, tabulate
  spec, arrays = tabulate.to_wide_spec(ref.make_table(4001, 4, 4, L, 1, 3))
  assert _hip.lib.campx_wide_spec_validate(ctypes.byref(spec)) == OK
  assert (spec.rows, spec.cols, spec.n_dyn, spec.n_states, spec.has_perf) == (4, 4, 1, 3, 0)
  return spec, arrays


def _changed(spec, **fields):
  from campx_amd import gamespec
  copy = gamespec.CampxWideSpec()
  ctypes.memmove(ctypes.byref(copy), ctypes.byref(spec), ctypes.sizeof(copy))
  for k, v in fields.items():
    setattr(copy, k, v)
  return copy


class _Calls(object):
  """The three entry points with every argument valid unless named."""

  def __init__(self, spec):
    self.spec = spec

  def _args(self, kw):
    from campx_amd import _hip
    spec = kw.pop('spec', self.spec)
    st = _hip.CampxState(pos=kw.pop('pos', FAKE), done=kw.pop('state_done', FAKE), ret=None, pair_table=None)
    out = dict(obs=FAKE, obs_t_stride=B * R, board=None, board_t_stride=0, reward=FAKE, discount=FAKE,
               done=FAKE, perf=None, trace=FAKE, obs_format=INT8, scalar_pitch=0)
    batch, tables = kw.pop('B', B), kw.pop('tables', FAKE)
    call = {k: kw.pop(k) for k in ('T', 'actions', 'reset_first') if k in kw}
    out.update(kw)
    by = ctypes.byref(spec) if spec is not None else None
    return by, ctypes.c_void_p(tables), st, _hip.CampxOutputs(**out), batch, call

  def reset(self, **kw):
    from campx_amd import _hip
    spec, tables, st, out, batch, call = self._args(kw)
    assert not call
    return _hip.lib.campx_wide_reset_launch(spec, tables, st, out, batch, None)

  def _play(self, f, kw):
    spec, tables, st, out, batch, call = self._args(kw)
    return f(spec, tables, st, ctypes.c_void_p(call.get('actions', FAKE)), out, batch, call.get('T', 2),
             call.get('reset_first', 0), None)

  def rollout(self, **kw):
    from campx_amd import _hip
    return self._play(_hip.lib.campx_wide_rollout_launch, kw)

  def update(self, **kw):
    from campx_amd import _hip
    return self._play(_hip.lib.campx_wide_update_launch, kw)


@pytest.fixture(scope='module')
def calls(table):
  return _Calls(table[0])


def test_the_call_that_the_cases_spoil_is_a_valid_one(calls):
  """T = 0 is the one valid call that launches nothing: every check of wide_check() has passed."""
  assert calls.rollout(T=0) == OK
  assert calls.rollout(T=0, obs_t_stride=0) == OK               # the last frame only
  assert calls.rollout(T=0, board=FAKE, board_t_stride=B * HW) == OK
  assert calls.rollout(T=0, scalar_pitch=B) == OK and calls.rollout(T=0, scalar_pitch=B + 8) == OK
  assert calls.rollout(T=0, obs_format=F16) == OK and calls.rollout(T=0, obs_format=BF16) == OK
  # ... which is not campx_wide_update_launch()'s reading of T = 0
  assert calls.update(T=0) == EINVAL


# (name, keyword arguments, code of reset / rollout / update; None: the call does not take the
# argument, or would reach its launch)
ONE_FAULT = [
    ('null spec', dict(spec=None), EINVAL, EINVAL, EINVAL),
    ('null table', dict(tables=None), EINVAL, EINVAL, EINVAL),
    ('null pos', dict(pos=None), EINVAL, EINVAL, EINVAL),
    ('null done', dict(state_done=None), EINVAL, EINVAL, EINVAL),
    ('null obs', dict(obs=None), EINVAL, EINVAL, None),          # (the update pass writes no frame)
    ('null trace', dict(trace=None), EINVAL, EINVAL, EINVAL),
    ('odd trace', dict(trace=FAKE + 1), EINVAL, EINVAL, EINVAL),
    ('pos off by two', dict(pos=FAKE + 2), EINVAL, EINVAL, EINVAL),
    ('obs off by eight', dict(obs=FAKE + 8), EINVAL, EINVAL, None),
    ('B = 0', dict(B=0), EINVAL, EINVAL, EINVAL),
    ('B = -1', dict(B=-1), EINVAL, EINVAL, EINVAL),
    ('T = -1', dict(T=-1), None, EINVAL, EINVAL),
    ('T = 0', dict(T=0), None, OK, EINVAL),
    ('null actions, T = 1', dict(T=1, actions=None), None, EINVAL, EINVAL),
    ('scalar_pitch = B - 1', dict(scalar_pitch=B - 1), EINVAL, EINVAL, EINVAL),
    ('obs_format 3', dict(obs_format=3), EINVAL, EINVAL, None),
    ('obs_format -1', dict(obs_format=-1), EINVAL, EINVAL, None),
    ('a 16-bit first frame', dict(obs_format=F16), EINVAL, None, None),
    ('perf from a spec without', dict(perf=FAKE), EINVAL, EINVAL, EINVAL),
    ('time stride B*R + 16', dict(obs_t_stride=B * R + 16), None, EINVAL, None),
    ('board time stride', dict(board=FAKE, board_t_stride=B * HW + 16), None, EINVAL, None),
    ('last frame only in 16 bits', dict(obs_t_stride=0, obs_format=BF16), None, EINVAL, None),
    ('a frame of 4 GiB', dict(B=1 << 27, obs_t_stride=R << 27), EINVAL, EINVAL, None),
]


@pytest.mark.parametrize('case', ONE_FAULT, ids=[c[0].replace(' ', '-') for c in ONE_FAULT])
def test_one_argument_wrong(calls, case):
  _, kw, reset, rollout, update = case
  for f, want in ((calls.reset, reset), (calls.rollout, rollout), (calls.update, update)):
    if want is not None:
      assert f(**dict(kw)) == want, f.__name__


def _bad_specs(spec):
  return [('bad magic', _changed(spec, magic=spec.magic ^ 1)),
          ('bad version', _changed(spec, version=spec.version + 1)),
          ('n_states = 0', _changed(spec, n_states=0)),
          ('fifteen cells', _changed(spec, rows=3, cols=5)),
          ('n_dyn = 0', _changed(spec, n_dyn=0))]


def test_a_spec_that_does_not_validate(table, calls):
  for name, bad in _bad_specs(table[0]):
    assert calls.reset(spec=bad) == ESPEC, name
    assert calls.rollout(spec=bad) == ESPEC, name
    assert calls.rollout(spec=bad, T=0) == ESPEC, name          # (refused before T = 0 returns)
    assert calls.update(spec=bad) == ESPEC, name


def test_of_two_faults_the_earlier_check_wins(table, calls):
  """The order, in all three: null pointers and counts, alignment, scalar_pitch, (obs_format,) the
  spec, perf, (the frame's size and strides; then reset's format, rollout's T = 0 and actions)."""
  bad = _changed(table[0], magic=0)
  for f in (calls.reset, calls.rollout, calls.update):
    # everything in front of the spec's own checks is EINVAL whatever the spec says
    assert f(spec=bad, pos=None) == EINVAL and f(spec=bad, trace=None) == EINVAL, f.__name__
    assert f(spec=bad, B=0) == EINVAL and f(spec=bad, trace=FAKE + 1) == EINVAL, f.__name__
    assert f(spec=bad, pos=FAKE + 2) == EINVAL and f(spec=bad, scalar_pitch=B - 1) == EINVAL, f.__name__
    # ... and what comes after them is not looked at
    assert f(spec=bad, perf=FAKE) == ESPEC, f.__name__
  for f in (calls.reset, calls.rollout):
    assert f(spec=bad, obs=None) == EINVAL and f(spec=bad, obs=FAKE + 8) == EINVAL, f.__name__
    assert f(spec=bad, obs_format=3) == EINVAL, f.__name__
  assert calls.reset(spec=bad, obs_format=F16) == ESPEC         # reset's own format rule comes last
  assert calls.reset(perf=FAKE, obs_format=F16) == EINVAL
  assert calls.rollout(spec=bad, obs_t_stride=B * R + 16) == ESPEC
  assert calls.rollout(spec=bad, T=1, actions=None) == ESPEC
  assert calls.update(spec=bad, T=1, actions=None) == EINVAL    # (here the actions are among the first)
  assert calls.update(spec=bad, T=0) == EINVAL
  # T = 0 asks for nothing: no actions, any strides - but only once everything else has passed
  assert calls.rollout(T=0, actions=None) == OK
  assert calls.rollout(T=0, obs_t_stride=B * R + 16) == OK
  assert calls.rollout(T=0, perf=FAKE) == EINVAL
  assert calls.rollout(T=0, obs_format=3) == EINVAL
  assert calls.rollout(T=0, scalar_pitch=B - 1) == EINVAL
  assert calls.rollout(T=0, B=1 << 27) == EINVAL
  # a bad stride is found before the missing actions are (both EINVAL; T = -1 before either)
  assert calls.rollout(T=-1, actions=None, obs_t_stride=B * R + 16) == EINVAL
