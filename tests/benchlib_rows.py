"""A stub row script for tests/test_benchlib_cpu.py: the child side of tools/benchlib.py's row
protocol without a device (and without torch).

    python tests/benchlib_rows.py --row <kind> <start file>

Every row first appends '<kind> <pid>' to the start file, then behaves as its kind says."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import benchlib  # noqa: E402


def row(kind, start):
  with open(start, 'a') as fh:
    fh.write('%s %d\n' % (kind, os.getpid()))
  if kind == 'exit5':
    sys.stderr.write('the stub row gives up\n')
    sys.exit(5)
  if kind == 'silent':
    sys.exit(0)
  if kind == 'late':
    time.sleep(60)
  return {'kind': kind, 'ms': 1.5} if kind.startswith('ok') else {'kind': kind, 'outcome': kind}


if __name__ == '__main__':
  assert sys.argv[1] == '--row'
  sys.exit(benchlib.row_main(row, sys.argv[2:]))
