"""What the sequences of tests/test_state_table_sequences.py can see, shown from the plans and the
host model alone (tests/sequence_model.py): no device, no kernel.  Conditions, not measurements -
`sequence_model.OFFSETS` holds the seed offsets at which they hold."""

import collections
import functools

import numpy as np
import pytest

import learner_reference as lref
import policy_reference as pref
import sequence_model as sm

SEEDS = range(sm.DEFAULT_SEEDS)
CASES = [(name, seed) for name in sm.GAMES for seed in SEEDS]
OPEN = ('play', 'rollout', 'trace', 'deferred', 'graph')


def _bits(a):
  a = np.asarray(a)
  return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
  if isinstance(a, dict):
    return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
  a, b = _bits(a), _bits(b)
  return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def steps(name, seed, defect=None):
  try:
    return sm.run_plan(name, seed, defect=defect)
  except AssertionError:                 # (a defective walk may leave the table's reachable entries)
    assert defect is not None
    return None


def differs(name, seed, defect):
  """Whether the defective model shows in anything the GPU test compares, at any operation."""
  if steps(name, seed, defect) is None:
    return True
  for (op, out, after, _), (_, out_d, after_d, _) in zip(steps(name, seed), steps(name, seed, defect)):
    if not same(out, out_d) or not all(same(x, y) for x, y in zip(after, after_d)):
      return True
  return False


def hand_overs(name):
  """The kinds that some case of the game begins with some environments over and some not, left
  that way by a call of another kind."""
  seen = set()
  for seed in SEEDS:
    prev = None
    for op, _, _, (over, _) in steps(name, seed):
      if (prev is not None and prev != op['kind'] and not op.get('reset_first')
          and over.any() and not over.all()):
        seen.add(op['kind'])
      prev = op['kind']
  return seen


def test_the_facts_the_plan_uses_are_the_tables():
  for name in sm.GAMES:
    g = sm.table(name)
    assert (g.n_states, int(g.has_perf)) == sm.FACTS[name], name
    assert g.any_reward
  for name in sm.SYNTHETIC:
    assert (sm.table(name).st_dcode != 0).any()
  assert sm.learn_fits(28, 1, 256) and not sm.learn_fits(29, 1, 256) and not sm.learn_fits(159, 0, 64)


@pytest.mark.parametrize('name,seed', CASES)
def test_shape_of_a_case(name, seed):
  ops = sm.plan(name, seed)
  assert ops == sm.plan(name, seed)                       # a pure function
  kinds = [op['kind'] for op in ops]
  assert len(ops) == sm.N_OPS == 14 and set(kinds) <= set(sm.KINDS)
  assert len(set(kinds)) >= 6 and sum(k in sm.CLOSED for k in kinds) >= 4
  S, perf = sm.FACTS[name]
  B = ops[0]['B']
  assert B in sm.BATCHES and all(op['B'] == B for op in ops)
  for op in ops:                                          # nothing the game cannot take
    if op['kind'] == 'population':
      assert B % op['P'] == 0 and (op['P'] <= 16 or op['P'] == B)
      assert op['path'] != 1 or sm.population_fits(S, perf, B, op['P'])
    if op['kind'] == 'learn':
      assert op['path'] != 1 or sm.learn_fits(S, perf, B)
  assert len(steps(name, seed)) == 14                     # the model ran every one of them


def test_every_ordered_pair_of_adjacent_kinds_occurs():
  seen = set()
  for name, seed in CASES:
    kinds = [op['kind'] for op in sm.plan(name, seed)]
    seen |= set(zip(kinds, kinds[1:]))
  missing = [p for p in sm.PAIRS if p not in seen]
  assert len(sm.PAIRS) == 64 and not missing, missing


def test_batches_and_forms_are_all_drawn():
  ops = [op for name, seed in CASES for op in sm.plan(name, seed)]
  assert {op['B'] for op in ops} == set(sm.BATCHES)
  assert {op['form'] for op in ops if op['kind'] == 'rollout'} == {'full', 'board', 'last', 'f16', 'bf16', 'out'}
  assert {op['path'] for op in ops if op['kind'] == 'population'} == {0, 1, 2}
  assert {op['path'] for op in ops if op['kind'] == 'learn'} == {0, 1, 2}
  assert {op['rule'] for op in ops if op['kind'] == 'learn'} == set(lref.RULES)
  assert {op['first_frame'] for op in ops if op['kind'] in ('policy', 'population')} == {None, 0, 6, sm.FAR}
  assert {op['what'] for op in ops if op['kind'] == 'bad'} == {'policy', 'rollout'}
  assert {op['n'] for op in ops if op['kind'] == 'graph'} == {1, 4}


@pytest.mark.parametrize('name', [n for n in sm.GAMES if n != 'boat_race'])
def test_ended_and_running_episodes_are_handed_over_to_every_kind(name):
  assert (sm.table(name).st_done != 0).any()
  assert hand_overs(name) >= set(sm.CARRYING), set(sm.CARRYING) - hand_overs(name)


def test_the_boat_race_has_no_entry_that_ends_an_episode():
  assert not (sm.table('boat_race').st_done != 0).any()


def test_start_frames_of_sampling_calls():
  residues = collections.defaultdict(set)
  after_open = set()
  for name, seed in CASES:
    prev = None
    for op, _, _, (_, policy_frame) in steps(name, seed):
      if op['kind'] in sm.CLOSED:
        first = op.get('first_frame')
        residues[op['kind']].add((policy_frame if first is None else first) % 4)
        if prev in OPEN and first is None:
          after_open.add(op['kind'])
      prev = op['kind']
  assert residues['policy'] == residues['population'] == {0, 1, 2, 3}, dict(residues)
  assert {r % 2 for r in residues['learn']} == {0, 1}
  assert after_open == set(sm.CLOSED)


@pytest.mark.parametrize('defect', sorted(sm.DEFECTS))
@pytest.mark.parametrize('name', sm.GAMES)
def test_a_defective_model_differs_in_some_case_of_every_game(name, defect):
  assert any(differs(name, seed, defect) for seed in SEEDS), sm.DEFECTS[defect]


def test_the_model_is_the_references():
  """Plans of `policy` only and of `learn` only give through the model what the walker gives alone."""
  name, B = 'syn28p5', 65
  g = sm.table(name)
  ops = [op for seed in range(8) for op in sm.plan(name, seed)]
  m, w = sm.SequenceModel(g, B, render=False), pref.PolicyWalker(g, B)
  for op in [op for op in ops if op['kind'] == 'policy'][:6]:
    got = m.run(op)
    want = w.rollout(sm.policy(g, op['salt']), op['T'], seed=op['seed'], first_frame=op['first_frame'],
                     reset_first=op['reset_first'])
    assert all(same(got[k], want[k]) for k in want)
    assert same(m.state, w.state) and same(m.over, w.over) and same(m.ret, w.ret)
    assert m.policy_frame == w.frame
  m = sm.SequenceModel(g, B, q_salt=3, render=False)
  L = lref.Learners(g, B, sm.first_q(g, B, 3))
  alpha, gamma, epsilon = sm.hyper(B)
  for op in [op for op in ops if op['kind'] == 'learn'][:6]:
    got = m.run(op)
    want = L.learn(op['T'], alpha, gamma, epsilon, rule=op['rule'], seed=op['seed'],
                   reset_first=op['reset_first'], window=op['window'])
    assert all(same(got[k], want[k]) for k in ('reward_sum', 'episodes', 'perf_sum')) and same(got['q'], L.q)
    assert same(m.state, L.state) and same(m.over, L.over) and same(m.ret, L.ret)
    assert m.policy_frame == L.frame
  assert not same(L.q, sm.first_q(g, B, 3))


def test_one_cell_plans_put_trace_and_graph_in_front_of_pipelined_and_deferred():
  for name in sm.ONE_CELL_GAMES:
    seen = set()
    for seed in range(2):
      kinds, B, _ = sm.one_cell_plan(name, seed)
      assert (kinds, B) == sm.one_cell_plan(name, seed)[:2] and len(kinds) == 14
      assert B in sm.ONE_CELL_BATCHES and set(kinds) <= set(sm.ONE_CELL_KINDS)
      seen |= {(x, y[:8]) for x, y in zip(kinds, kinds[1:])}
    assert {(x, y) for x in ('trace', 'graph') for y in ('pipeline', 'deferred')} <= seen, (name, seen)
