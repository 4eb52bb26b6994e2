"""tools/benchlib.py on CPU: the row driver and its failure rule against a stub row script
(tests/benchlib_rows.py), and the `report()` of every script that runs on it against records written
by hand in the shape its `row()` documents."""
import copy
import importlib
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, 'tools')
if TOOLS not in sys.path:
  sys.path.insert(0, TOOLS)
import benchlib  # noqa: E402

STUB = os.path.join(REPO, 'tests', 'benchlib_rows.py')
SCRIPTS = ('bench_online', 'bench_shared', 'bench_population', 'bench_traces', 'bench_planning',
           'bench_visitation', 'bench_learner', 'bench_population_planning', 'bench_population_rewards',
           'bench_visit_population', 'bench_vtrace', 'bench_windows')


def stub_report(records):
  lines = ['# the stub'] + ['%s %s' % (r['kind'], r['outcome']) for r in records]
  ok = all(r['outcome'] != 'gate_missed' for r in records)
  return lines + ['gate: %s' % ('met' if ok else 'MISSED')], ok


def run_stub(tmp_path, kinds, seconds=30):
  start = tmp_path / 'started.txt'
  records, broke = benchlib.run_rows(STUB, [(kind, start) for kind in kinds], seconds)
  started = [line.split() for line in start.read_text().splitlines()]
  lines, ok = stub_report(records)
  status = benchlib.finish(str(tmp_path / 'report.txt'), lines, ok, broke)
  return records, broke, started, status, (tmp_path / 'report.txt').read_text().splitlines()


def test_rows_answer_in_order_and_the_gate_is_met(tmp_path):
  records, broke, started, status, text = run_stub(tmp_path, ('ok', 'skipped', 'ok2'))
  assert broke is None and status == 0
  assert records == [{'kind': 'ok', 'ms': 1.5, 'outcome': 'ok'}, {'kind': 'skipped', 'outcome': 'skipped'},
                     {'kind': 'ok2', 'ms': 1.5, 'outcome': 'ok'}]
  assert [kind for kind, _ in started] == ['ok', 'skipped', 'ok2']
  assert len({pid for _, pid in started}) == 3                  # a fresh process each
  assert text == ['# the stub', 'ok ok', 'skipped skipped', 'ok2 ok', 'gate: met']


def test_a_missed_gate_goes_on_and_exits_1(tmp_path):
  records, broke, started, status, text = run_stub(tmp_path, ('ok', 'gate_missed', 'ok2'))
  assert broke is None and status == 1
  assert [r['outcome'] for r in records] == ['ok', 'gate_missed', 'ok']
  assert [kind for kind, _ in started] == ['ok', 'gate_missed', 'ok2']
  assert text[-1] == 'gate: MISSED' and benchlib.ENDED not in text


@pytest.mark.parametrize('kind,seconds,status,why', [('exit5', 30, 5, 'exit status 5'), ('silent', 30, 0, '0 ROW lines'),
                                                     ('late', 2, None, 'outlasted its 2 s')])
def test_the_first_bad_row_ends_the_run(tmp_path, kind, seconds, status, why):
  records, broke, started, exit_status, text = run_stub(tmp_path, ('ok', kind, 'ok2', 'ok3'), seconds)
  assert [r['kind'] for r in records] == ['ok']                  # what was collected is kept
  assert [name for name, _ in started] == ['ok', kind]           # nothing after the bad row was started
  assert broke['row'][0] == kind and broke['status'] == status and broke['why'] == why
  assert ('the stub row gives up' in broke['stderr']) == (kind == 'exit5')
  assert exit_status == 2
  assert text[:3] == ['# the stub', 'ok ok', 'gate: met'] and text[-1] == benchlib.ENDED
  assert any(line.startswith('row %s ' % kind) and 'FAILED (%s)' % why in line for line in text)
  if kind == 'late':                                             # killed and reaped, not left behind
    with pytest.raises(ProcessLookupError):
      os.kill(int(started[-1][1]), 0)


def test_a_bad_first_row_still_writes_a_report(tmp_path):
  records, broke, started, status, text = run_stub(tmp_path, ('exit5', 'ok'))
  assert records == [] and status == 2 and [kind for kind, _ in started] == ['exit5']
  assert text[0] == '# the stub' and text[-1] == benchlib.ENDED
  assert benchlib.device_of(records) == 'no row answered'


@pytest.fixture(scope='module')
def torch_importers():
  """The modules among benchlib and SCRIPTS whose import, in a fresh interpreter, brings torch in."""
  code = ('import importlib, sys\n'
          'sys.path.insert(0, %r)\n'
          'for name in %r:\n'
          '  importlib.import_module(name)\n'
          '  if "torch" in sys.modules:\n'
          '    print("IMPORTS_TORCH", name)\n'
          '    break\n'
          'print("IMPORTED_ALL")\n' % (TOOLS, ('benchlib',) + SCRIPTS))
  done = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0 and 'IMPORTED_ALL' in done.stdout, done.stderr[-2000:]
  return [line.split()[1] for line in done.stdout.splitlines() if line.startswith('IMPORTS_TORCH')]


def test_benchlib_and_the_row_scripts_import_without_torch(torch_importers):
  assert torch_importers == []


def test_no_copy_of_the_timer_or_the_driver_is_left():
  for name in os.listdir(TOOLS):
    if name.endswith('.py') and name != 'benchlib.py':
      with open(os.path.join(TOOLS, name)) as fh:
        text = fh.read()
      for word in ('timed_ms', 'median_ms', 'medians_ms', 'median_us', 'timed'):
        assert 'def %s(' % word not in text, (name, word)
      if name[:-3] in SCRIPTS:
        assert 'import subprocess' not in text and 'GATE_MISSED =' not in text and 'SKIPPED =' not in text, name


# ---- report() of each script: (records that meet the gate, lines of their report, how to miss it) ----

def _set(index, **changes):
  def change(records):
    for key, value in changes.items():
      target = records[index]
      *way, last = key.split('__')
      for step in way:
        target = target[step]
      target[last] = value
  return change


GPU = 'a device'
TRIPLE = lambda ms: [ms, ms * 0.9, ms * 1.5]
REPORTS = {
    'bench_online': ([
        {'name': 'boat_race', 'S': 8, 'plan': [1, 41328, 0, 1], 'ours': 0.4, 'loop': 160.0, 'device': GPU, 'outcome': 'ok'},
        {'name': 'maze16', 'S': 159, 'plan': [2, 6368, 0, 0], 'ours': 0.9, 'loop': 166.0, 'device': GPU, 'outcome': 'ok'}],
        4, _set(1, ours=200.0, outcome='gate_missed')),
    'bench_shared': ([
        {'name': 'boat_race', 'S': 8, 'n': 16, 'P': 4096, 'path': 1, 'device': GPU, 'plan': [1, 4, 256, 9000, 1, 0],
         'ours': 0.5, 'loop': 170.0, 'tabular': 0.4, 'outcome': 'ok'},
        {'name': 'maze16', 'S': 159, 'n': 1, 'P': 65536, 'path': 1, 'device': GPU, 'outcome': 'skipped'}],
        4, _set(0, ours=171.0, outcome='gate_missed')),
    'bench_population': ([
        {'name': 'boat_race', 'S': 8, 'P': 1, 'plan': [1, 368, 0, 1], 'device': GPU, 'pop': 0.11, 'same_b': 0.1,
         'one_member': 0.1, 'outcome': 'ok'},
        {'name': 'maze16', 'S': 159, 'P': 256, 'plan': [2, 0, 0, 4], 'device': GPU, 'pop': 0.2, 'same_b': 0.1,
         'one_member': 0.03, 'outcome': 'ok'}],
        4, _set(1, pop=9.0, outcome='gate_missed')),
    'bench_traces': ([
        {'name': 'boat_race', 'S': 8, 'what': 'torch', 'path': 0, 'team': 0, 'device': GPU, 'runs': 3, 'ms': 300.0},
        {'name': 'boat_race', 'S': 8, 'what': 'tabular', 'path': 0, 'team': 0, 'device': GPU, 'runs': 15, 'ms': 0.4},
        {'name': 'boat_race', 'S': 8, 'what': 'traces', 'path': 0, 'team': 0, 'device': GPU, 'runs': 15, 'ms': 2.0,
         'plan': [1, 8, 20000, 0, 0]},
        {'name': 'boat_race', 'S': 8, 'what': 'traces', 'path': 2, 'team': 64, 'device': GPU, 'runs': 3, 'ms': 1.0,
         'plan': [2, 64, 512, 0, 0]}],
        7, _set(3, ms=301.0)),
    'bench_planning': ([
        {'kind': kind, 'S': S, 'fill_gbs': 3000.0, 'device': GPU,
         'policy_torch': 0.05, 'policy_path0': 0.01, 'policy_path1': path1, 'policy_path2': 0.02, 'policy_plan': 1,
         'policy_max_diff': 1e-7, 'greedy_torch': 0.04, 'greedy_path0': 0.01, 'greedy_path1': path1,
         'greedy_path2': 0.02, 'greedy_plan': 2, 'greedy_max_diff': 0.0}
        for kind, S, path1 in (('boat_race', 8, 0.01), ('synthetic', 4400000, None))],
        11, _set(1, greedy_path0=0.05)),
    'bench_visitation': ([
        {'kind': 'boat_race', 'S': 8, 'alive': 36, 'same': True, 'plan': 1, 'device': GPU, 'torch': 0.2, 'path0': 0.01,
         'path1': 0.01, 'path2': 0.02},
        {'kind': 'synthetic', 'S': 4400000, 'alive': 19800000, 'same': True, 'plan': 2, 'device': GPU, 'torch': 2.0,
         'path0': 0.5, 'path1': None, 'path2': 0.5}],
        8, _set(0, same=False)),
    'bench_learner': ([
        {'kind': kind, 'S': S, 'B': 65536, 'plan': [path, 4, 0, 0, 0, 640, 0, 0], 'device': GPU, 'max_diff_2': 0.0,
         'max_diff_3': 1e-6, 'form1': 3.0, 'form2': 2.5, 'form3': 0.3, 'sums_path0': 0.2, 'sums_path1': path1,
         'sums_path2': 0.25, 'sums_k0': 0.1, 'lookup': 0.05}
        for kind, S, path, path1 in (('boat_race', 8, 1, 0.2), ('uniform', 4400000, 2, None))],
        8, _set(0, form3=3.5)),
    'bench_population_planning': ([
        {'game': 'boat_race', 'S': 8, 'P': 16, 'plan': [1, 0, 0, 16, 1], 'device': GPU, 'path0': 0.05, 'path1': 0.05,
         'path2': 0.9, 'loop': 0.6, 'same_bits': True},
        {'game': 'maze16', 'S': 159, 'P': 65536, 'plan': [2, 0, 0, 4096, 1], 'device': GPU, 'path0': 9.0, 'path1': None,
         'path2': 9.0, 'loop': None}],
        6, _set(0, path0=0.7)),
    'bench_population_rewards': ([
        {'game': 'boat_race', 'S': 8, 'P': P, 'device': GPU,
         'greedy': {'plan': [1, 0, 0, P, 1], 'same_bits': True, 'loop': 0.04 * P, 'path0': 0.05, 'path1': 0.05,
                    'path2': 0.9},
         'policy': {'plan': [2, 0, 0, P, 1], 'same_bits': True, 'loop': 0.04 * P, 'path0': 0.06, 'path2': 0.06}}
        for P in (1, 16)],
        9, _set(1, policy__path0=0.7)),
    'bench_visit_population': ([
        {'game': 'boat_race', 'S': 8, 'P': 16, 'plan': [1, 0, 0, 16, 1], 'device': GPU, 'same_bits': True,
         'path0': TRIPLE(0.05), 'loop': TRIPLE(0.6), 'path2': TRIPLE(0.14)},
        {'game': 'maze16', 'S': 159, 'P': 1, 'plan': [1, 0, 0, 1, 1], 'device': GPU, 'same_bits': True,
         'path0': TRIPLE(0.05), 'loop': TRIPLE(0.05), 'path2': TRIPLE(0.12)}],
        6, _set(0, path0=TRIPLE(0.6))),
    'bench_vtrace': ([
        {'kind': 'ratio', 'B': 4096, 'S': 8, 'P': 1, 'kernel': [0.02], 'loop': 1.1, 'on_policy': 0.018, 'outcome': 'ok'},
        {'kind': 'maze16', 'B': 65536, 'S': 159, 'P': 1, 'kernel': [0.06, 0.07], 'loop': 1.4, 'outcome': 'ok'}],
        5, _set(1, kernel=[0.06, 1.5], outcome='gate_missed')),
    'bench_windows': ([
        {'name': 'maze16', 'h': 7, 'w': 7, 'N': 1048576, 'states': False, 'mine': 1048576 * 3 * 49,
         'theirs': 1048576 * 3 * 256, 'ours': 90.0, 'baseline': 3000.0, 'outcome': 'ok'},
        {'name': 'maze16', 'h': 5, 'w': 5, 'N': 159, 'states': True, 'mine': 159 * 3 * 25, 'theirs': 159 * 3 * 256,
         'ours': 9.0, 'baseline': 40.0, 'outcome': 'ok'}],
        4, _set(0, ours=3100.0, outcome='gate_missed')),
}


@pytest.mark.parametrize('script', SCRIPTS)
def test_report_formats_and_gates_hand_written_records(script):
  module = importlib.import_module(script)
  records, n_lines, miss = REPORTS[script]
  lines, ok = module.report(copy.deepcopy(records))
  gate = [line for line in lines if line.startswith('gate (')]
  assert ok is True and len(gate) == 1 and gate[0].endswith(': met')
  assert lines[0].startswith('# tools/%s.py' % script) and lines[0].endswith(records[0].get('device', ''))
  assert len(lines) == n_lines and not any('MISSED' in line or 'DIFFER' in line for line in lines)
  assert all(isinstance(line, str) and line for line in lines)
  bad = copy.deepcopy(records)
  miss(bad)
  lines, ok = module.report(bad)
  gate = [line for line in lines if line.startswith('gate (')]
  assert ok is False and len(gate) == 1 and gate[0].endswith(': MISSED')
  assert sum('GATE MISSED' in line or 'NO' in line.split() for line in lines) == 1
  # no record at all (the first row ended the run): still a header and a gate line
  lines, ok = module.report([])
  assert lines[0].startswith('# tools/%s.py' % script) and any(line.startswith('gate (') for line in lines)
