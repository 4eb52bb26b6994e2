"""The sampling rule of closed-loop rollouts, on the CPU: tests/policy_reference.py - the numpy
restatement the GPU tests (test_policy_rollout.py) hold `WideGame.rollout_policy()` to - against
Philox4x32-10's known answers and the properties include/campx_hip.h promises."""

import numpy as np

import policy_reference as ref

N = 1 << 20


def _hex(words):
  return ' '.join('{:08x}'.format(int(w)) for w in words)


def test_philox_known_answers():
  cases = [
      ([0, 0, 0, 0], [0, 0], '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
      ([0xffffffff] * 4, [0xffffffff] * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
      ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
       'd16cfe09 94fdcceb 5001e420 24126ea1')]
  for counter, key, want in cases:
    assert _hex(ref.philox4x32_10(np.array(counter, np.uint32), np.array(key, np.uint32))) == want
  # the three at once, broadcast; and `words()` picks word f & 3 of block (e, f >> 2)
  got = ref.philox4x32_10(np.array([c for c, _, _ in cases], np.uint32),
                          np.array([k for _, k, _ in cases], np.uint32))
  assert [_hex(row) for row in got] == [w for _, _, w in cases]
  seed = 0x299f31d0a4093822
  block = ref.philox4x32_10(np.array([5, 7, 1, 0], np.uint32), np.array([0xa4093822, 0x299f31d0], np.uint32))
  frames = ((1 << 32) + 7) * 4 + np.arange(4)
  assert np.array_equal(ref.words(seed, 5, frames), block)


def _draws(rows, seed=3):
  x = ref.words(seed, np.arange(N), 0)
  return ref.sample(x, np.broadcast_to(np.asarray(rows, np.float32), (N, 5)))


def test_zero_weight_actions_are_never_drawn():
  for row in ([0, 0, .3, .3, .4], [.3, 0, 0, .3, .4], [.3, .3, 0, .4, 0], [.2, .3, .5, 0, 0],
              [0, 0, 0, 0, 2.5], [0, 1e-3, 0, 3e-3, 0]):
    a, bad = _draws(row)
    assert not bad.any()
    counts = np.bincount(a, minlength=5)
    for k in range(5):
      assert (counts[k] == 0) == (row[k] == 0), (row, counts)
  # the words' extremes: u = 0 and u = 1 - 2^-24
  x = np.array([0, 0xff, 0xffffff00, 0xffffffff], np.uint32)
  for row, want in (([.2, .3, .5, 0, 0], [0, 0, 2, 2]), ([0, 0, .5, .5, 0], [2, 2, 3, 3]),
                    ([0, 0, 0, 0, 7], [4, 4, 4, 4])):
    a, _ = ref.sample(x, np.broadcast_to(np.array(row, np.float32), (4, 5)))
    assert a.tolist() == want, row


def test_one_hot_rows_are_deterministic():
  for k in range(5):
    for scale in (1.0, 1e-3, 3e4):
      a, bad = _draws(np.eye(5, dtype=np.float32)[k] * scale)
      assert not bad.any() and (a == k).all()


def test_unnormalised_rows_sample_what_their_normalised_form_does():
  base = np.array([0.1, 0.2, 0.3, 0.15, 0.25], np.float64)
  for total in (1e-3, 7.5, 3e4):
    rows = (base * total).astype(np.float32)
    norm = (rows / rows.sum(dtype=np.float32)).astype(np.float32)
    a, _ = _draws(rows)
    b, _ = _draws(norm)
    same = float((a == b).mean())
    assert same >= 0.999, (total, same)


def test_frequencies_follow_the_weights():
  w = np.array([0.1, 0.2, 0.3, 0.15, 0.25], np.float32)
  x = ref.words(7, np.arange(N), 0)
  a, _ = ref.sample(x, np.broadcast_to(w, (N, 5)))
  freq = np.bincount(a, minlength=5) / float(N)
  assert np.abs(freq - w).max() < 0.0025, freq       # 5 sigma at 2^20 draws


def test_bad_rows_take_action_four_and_are_counted():
  x = ref.words(1, np.arange(64), 0)
  for row in ([np.nan, 1, 1, 1, 1], [1, 1, -0.5, 1, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, np.inf],
              [3e38, 3e38, 0, 0, 0]):
    a, bad = ref.sample(x, np.broadcast_to(np.array(row, np.float32), (64, 5)))
    assert bad.all() and (a == 4).all(), row


def test_two_calls_with_a_continued_counter_equal_one():
  from campx_amd import tabulate
  from campx_amd.games import boat_race
  traced = tabulate.trace(boat_race.build())
  rng = np.random.RandomState(5)
  policy = rng.uniform(0.05, 1.0, size=(traced.n_states, 5)).astype(np.float32)
  B = 37
  one, two = ref.PolicyWalker(traced, B), ref.PolicyWalker(traced, B)
  whole = one.rollout(policy, 20, seed=11)
  first = two.rollout(policy, 9, seed=11)
  second = two.rollout(policy, 11, seed=11)
  assert two.frame == one.frame == 20
  for k in ('states', 'actions', 'reward', 'discount', 'done', 'perf'):
    assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
  assert np.array_equal(one.state, two.state) and np.array_equal(one.ret.view(np.uint32), two.ret.view(np.uint32))
  assert len(np.unique(whole['actions'])) == 5 and len(np.unique(whole['states'])) > 1
  # ... and another seed, or the same frames counted from elsewhere, is another rollout
  other = ref.PolicyWalker(traced, B).rollout(policy, 20, seed=12)
  moved = ref.PolicyWalker(traced, B).rollout(policy, 20, seed=11, first_frame=4)
  assert not np.array_equal(other['actions'], whole['actions'])
  assert not np.array_equal(moved['actions'], whole['actions'])
  assert np.array_equal(moved['actions'][0], ref.sample(ref.words(11, np.arange(B), 4), policy[[0] * B])[0])
