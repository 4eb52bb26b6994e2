"""What the `tools/bench_*.py` scripts share: the event-pair timers, the two games most of them
build, and the driver of a run whose rows each get a process of their own.

THE ROW PROTOCOL.  A script's `main` hands `run_rows()` its rows; each runs as a fresh child
`python script --row <args>` under its own time limit, where `row_main()` calls the script's
`row()` and prints its dict as ONE line `ROW <json>` on stdout.  The record carries an `outcome`:
`ok` (measured), `gate_missed` (measured, and the row's own gate is missed) or `skipped` (nothing to
measure, by design).  A row whose gate `report()` judges from its numbers answers `ok`.

THE FAILURE RULE.  The first child that exits non-zero (a signal's negative status, 134 and 139
included), prints no `ROW` line, or outlasts its limit ends the run: it is never tried again,
NOTHING MORE IS STARTED ON THE DEVICE, and what was collected is still formatted and written, with
the failed row, its status and the tail of its stderr beneath it.  The gate line of such a report
speaks of the collected rows only.

EXIT STATUSES of a script, from `finish()`: 0 gate met, 1 gate missed, 2 the run broke off.

Importing this module does not import torch: a parent process never opens the device.
"""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENDED = 'the run ended at the row above; the rows after it were not started'
STDERR_TAIL = 2000


def event_ms(fn):
  """The milliseconds of one call of `fn`, between one pair of events."""
  import torch
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def median_ms(fn, runs, warm=0):
  """`warm` calls, a synchronise, then the median of `runs` event pairs."""
  import torch
  for _ in range(warm):
    fn()
  torch.cuda.synchronize()
  return statistics.median(event_ms(fn) for _ in range(runs))


def alternating_ms(calls, runs, warm):
  """{name: (median, min, max)} in ms of the callables of the ordered dict `calls`: every warm-up
  round and every timed round calls each once, in order, so that a drifting clock meets them alike."""
  import torch
  for _ in range(warm):
    for fn in calls.values():
      fn()
  torch.cuda.synchronize()
  times = {name: [] for name in calls}
  for _ in range(runs):
    for name, fn in calls.items():
      times[name].append(event_ms(fn))
  return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def state_table_game(name, batch):
  """'boat_race' on its state table or 'maze16', the 16x16 maze, at `batch` environments: shown,
  and with action validation off."""
  from campx_amd.games import boat_race, maze
  if name == 'boat_race':
    game = boat_race.build(batch, 'cuda')
    game.use_state_table()
  elif name == 'maze16':
    game = maze.build(16, 16, batch=batch, device='cuda')
  else:
    raise ValueError('no such game: %r' % (name,))
  game.its_showtime()
  game.fused.validate_actions = False
  return game


def run_rows(script, rows, seconds):
  """Runs `rows` (tuples of arguments) one at a time, each as a fresh `python script --row <args>`
  with `seconds` to finish in.  Returns (records, broke): the records of the rows that answered, in
  order, and None - or, for the row that ended the run, a dict of its `row`, `why`, `status` (None
  when it outlasted its limit and was killed) and `stderr` tail."""
  records = []
  for args in rows:
    cmd = [sys.executable, os.path.abspath(script), '--row'] + [str(a) for a in args]
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
      out, err = child.communicate(timeout=seconds)
      status = child.returncode
      answers = [line[4:] for line in out.splitlines() if line.startswith('ROW ')]
      why = ('exit status %d' % status if status != 0 else
             '%d ROW lines' % len(answers) if len(answers) != 1 else None)
    except subprocess.TimeoutExpired:
      child.kill()
      out, err = child.communicate()
      status, why = None, 'outlasted its %d s' % seconds
    if why is not None:
      return records, {'row': list(args), 'why': why, 'status': status, 'stderr': err[-STDERR_TAIL:]}
    records.append(json.loads(answers[0]))
    print('row %s: %s' % (' '.join(cmd[3:]), records[-1]['outcome']), file=sys.stderr, flush=True)
  return records, None


def row_main(row_fn, argv):
  """The child's side: calls `row_fn` on `argv` (the words after `--row`, decimal ones as ints) and
  prints its record; the outcome is `ok` unless the row says otherwise."""
  record = row_fn(*[int(a) if a.lstrip('-').isdigit() else a for a in argv])
  record.setdefault('outcome', 'ok')
  print('ROW ' + json.dumps(record), flush=True)
  return 0


def out_path(argv, default):
  """The report's path: the first word of `argv`, or `default` under profiles/."""
  return argv[0] if argv else os.path.join(REPO, 'profiles', default)


def device_of(records):
  """The device the rows ran on, for a report's header: every `row()` records it as `device`."""
  return records[0]['device'] if records else 'no row answered'


def finish(path, lines, ok, broke):
  """Closes a run: the report `lines`, beneath them the row that ended the run if one did (`broke`
  of `run_rows()`), printed and written to `path` whatever happened.  Returns the exit status."""
  lines = list(lines)
  if broke:
    lines.append('row %s FAILED (%s)\n%s' % (' '.join(str(a) for a in broke['row']), broke['why'],
                                             broke['stderr'].rstrip('\n')))
    lines.append(ENDED)
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  with open(path, 'w') as fh:
    fh.write(text)
  return 2 if broke else (0 if ok else 1)
