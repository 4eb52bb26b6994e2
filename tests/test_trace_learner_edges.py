"""`WideGame.learn_traces()` at the edges of float32, against tests/trace_learner_reference.py with
tests/float_edges.py's NaN-aware equality (the bits of every number, NaN where NaN): traces that
decay through the subnormals to 0, -0.0 entries of q that keep their sign under a zero trace, and a
`step` of +-inf or NaN that spreads to the entries with a trace and to no other.  The table, the
tables q and the hyper-parameters are tests/test_float_edges.py's learners': seven states, 257
learners, a third of q an edge constant, subnormal alphas, gammas of 0, 2 and -1."""

import functools
import types

import numpy as np
import pytest
import torch

import float_edges as fe
import trace_learner_reference as trace_ref

pytestmark = pytest.mark.gpu

F = np.float32
B, S, T = fe.LEARN_B, fe.LEARN_S, fe.LEARN_T
# one lane per learner in LDS (planned), teams in LDS, teams through L1 / L2
SHAPES = ((0, 0), (1, 8), (2, 64))


def _game():
  from campx_amd import wide
  f = wide.WideGame(types.SimpleNamespace(rows=4, cols=5), B, 'cuda', fe.learner_table())
  f.showtime()
  return f


def _cuda(*arrays):
  return [torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda() for a in arrays]


@functools.lru_cache(maxsize=None)
def _edge_traces():
  """[B, S, 5]: half zeros - a quarter of them -0.0 -, the rest subnormals, ordinary numbers and
  some NaN."""
  rng = np.random.RandomState(5)
  values = np.array([0.0, 0.0, 0.0, -0.0, fe.SUB_MIN, 2.0 ** -140, fe.SUB_MAX, fe.NORM_MIN, 0.5, 1.0,
                     -1.0, np.nan], F)
  return values[rng.randint(0, len(values), size=(B, S, 5))]


@functools.lru_cache(maxsize=None)
def _want(rule, kind):
  x = fe.learner_inputs()
  lam = np.array([0.0, 1.0, 0.5, 2.0 ** -20], F)[np.arange(B) % 4]
  L = trace_ref.TraceLearners(fe.learner_table(), B, x['q'], _edge_traces())
  want = L.learn_traces(T, lam, kind, x['alpha'], x['gamma'], x['epsilon'], rule, fe.LEARN_SEED,
                        fe.LEARN_FIRST, window=fe.LEARN_WINDOW, record=True)
  return L, want, lam


@pytest.mark.parametrize('path,team', SHAPES)
@pytest.mark.parametrize('kind', trace_ref.KINDS)
@pytest.mark.parametrize('rule', trace_ref.RULES)
def test_edge_tables_and_edge_traces_against_the_reference(rule, kind, path, team):
  assert fe.host_keeps_subnormals()
  x = fe.learner_inputs()
  L, want, lam = _want(rule, kind)
  assert want['bad'] == 0
  f = _game()
  q, z = _cuda(x['q'], _edge_traces())
  res = f.learn_traces(T, q, z, *_cuda(lam), kind, *_cuda(x['alpha'], x['gamma'], x['epsilon']), rule,
                       fe.LEARN_SEED, fe.LEARN_FIRST, window=fe.LEARN_WINDOW, path=path, team=team)
  got_q, got_z = q.cpu().numpy(), z.cpu().numpy()
  assert fe.same_bits_or_nan(got_q, L.q) and fe.same_bits_or_nan(got_z, L.z)
  assert fe.same_bits_or_nan(res['reward_sum'].cpu().numpy(), want['reward_sum'])
  assert np.array_equal(res['episodes'].cpu().numpy(), want['episodes'])
  assert np.array_equal(f.state.cpu().numpy(), L.state)
  assert fe.same_bits_or_nan(f.ret.cpu().numpy(), L.ret)
  # the cases are there: steps that are +-inf and NaN, and entries no sweep wrote - they hold the
  # bits they came with, the -0.0 among them too, whatever the learner's steps were
  step = want['step']
  assert np.isposinf(step).any() and np.isneginf(step).any() and np.isnan(step).any()
  wild = ~np.isfinite(step).all(axis=0)                          # learners with such a step
  kept = ~want['touched'].reshape(B, S, 5)
  assert (kept[wild] & fe.negative_zero(x['q'])[wild]).any() and (~kept[wild]).any()
  assert np.array_equal(got_q.view(np.uint32)[kept], x['q'].view(np.uint32)[kept])
  # ... and what a wild step touched is no longer finite where the trace was not zero
  assert (~np.isfinite(got_q[wild]) & ~kept[wild]).any()
  f.check_actions()


@pytest.mark.parametrize('path,team', SHAPES)
def test_traces_decay_through_the_subnormals_to_zero(path, team):
  """Expected SARSA never cuts and the synthetic table's learners rarely end an episode: with
  c = (0.5 * D) * 2^-20 a trace of 1 is 2^-21k after k frames, subnormal from k = 7 on (D = 1) and
  0 after that; the reference is walked a frame at a time to see them pass."""
  x = fe.learner_inputs()
  q0 = np.random.RandomState(3).uniform(-1, 1, size=(B, S, 5)).astype(F)
  hyper = dict(lam=2.0 ** -20, alpha=0.5, gamma=0.5, epsilon=0.25, rule='expected_sarsa',
               seed=fe.LEARN_SEED)
  L = trace_ref.TraceLearners(fe.learner_table(), B, q0)
  seen_subnormal = np.zeros((B, S, 5), bool)
  for t in range(12):
    L.learn_traces(1, reset_first=t == 0, **hyper)
    seen_subnormal |= fe.subnormal(L.z)
  gone = seen_subnormal & (L.z == 0)
  assert seen_subnormal.any() and gone.any()
  f = _game()
  q, z = _cuda(q0, np.zeros_like(q0))
  f.learn_traces(12, q, z, reset_first=True, path=path, team=team, **hyper)
  got_z = z.cpu().numpy()
  assert fe.same_bits_or_nan(got_z, L.z) and fe.same_bits_or_nan(q.cpu().numpy(), L.q)
  assert fe.subnormal(got_z).any() and (got_z[gone] == 0).all()
  f.check_actions()
