"""Observation windows of the state-table tier: what the agent sees instead of the whole board.

A `Window` is `height x width` cells, either centred on a tracked thing (egocentric - PyColab's
`ScrollingCropper`) or at a fixed place of the board (`FixedCropper`).  `WideGame`'s
`render_frame_windows()`, `render_trace_windows()` and `render_state_windows()` take one and write
`[..., L, height, width]` straight from trace entries or state ids (csrc/k_window.hip); the full
`[L, H, W]` observation is never written.  include/campx_hip.h has the rule: a window is, bit for
bit, a crop of the full observation, with cells off the board 0 - or 1 in the `pad` character's
layer.
"""

import collections

Resolved = collections.namedtuple('Resolved', ['thing', 'r0', 'c0', 'pad_layer'])


class Window(object):
  """`Window(5, 5, 'P', pad='#')`: five by five cells round the thing drawn as 'P', the wall's
  layer set where the window hangs over the edge.  `Window(3, 4, (-1, 2))`: three rows by four
  columns whose top-left cell is row -1, column 2 of the board.

  Args:
    height, width: cells; at most `2 * rows - 1` by `2 * cols - 1` of the game's board, and
        `layers * height * width >= 16` (both checked against the game at the call).
    centre: the character of a TRACKED thing - one whose cell is in the trace; the window's
        top-left cell is then `(row - height // 2, col - width // 2)` of the thing's cell, whether
        or not the thing shows there - or a `(row, col)` pair, the top-left cell of a fixed
        window; either may be negative.
    pad: None - every layer is 0 off the board - or a character of the game, whose layer is 1
        there.
  """

  def __init__(self, height, width, centre, pad=None):
    for name, v in (('height', height), ('width', width)):
      if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError('Window: {} must be an int >= 1, got {!r}'.format(name, v))
    if isinstance(centre, str):
      if len(centre) != 1:
        raise ValueError('Window: centre must be ONE character of a tracked thing or a (row, col) '
                         'pair, got {!r}'.format(centre))
    else:
      try:
        r, c = centre
        ok = all(isinstance(v, int) and not isinstance(v, bool) for v in (r, c))
      except (TypeError, ValueError):
        ok = False
      if not ok:
        raise ValueError('Window: centre must be the character of a tracked thing or a (row, col) '
                         'pair of ints, got {!r}'.format(centre))
      if not (-255 <= r <= 255 and -255 <= c <= 255):
        raise ValueError('Window: a fixed window\'s top-left cell must be within -255 .. 255, got '
                         '{!r}'.format(centre))
      centre = (int(r), int(c))
    if pad is not None and (not isinstance(pad, str) or len(pad) != 1):
      raise ValueError('Window: pad must be None or one character of the game, got {!r}'.format(pad))
    self.height, self.width, self.centre, self.pad = int(height), int(width), centre, pad

  def __repr__(self):
    return 'Window({}, {}, {!r}, pad={!r})'.format(self.height, self.width, self.centre, self.pad)

  def resolve(self, chars, spec):
    """(thing plane or -1, r0, c0, pad layer or -1) against a game's characters `chars` (layer
    order) and its `CampxWideSpec` (`n_dyn`, `dyn_layer`, `rows`, `cols`, `n_layers`)."""
    chars = list(chars)
    L, H, W = int(spec.n_layers), int(spec.rows), int(spec.cols)
    tracked = [chars[int(spec.dyn_layer[d])] for d in range(int(spec.n_dyn))]
    h, w = self.height, self.width
    if h > 2 * H - 1 or w > 2 * W - 1:
      raise ValueError('{!r}: a window on a {} x {} board is at most {} x {}'.format(
          self, H, W, 2 * H - 1, 2 * W - 1))
    if L * h * w < 16:
      raise ValueError('{!r}: rows of {} layers x {} x {} = {} elements are below the 16 the '
                       'kernel needs'.format(self, L, h, w, L * h * w))
    thing, r0, c0 = -1, 0, 0
    if isinstance(self.centre, str):
      ch = self.centre
      if ch not in chars:
        raise ValueError('{!r}: the game has no character {!r} (its characters: {})'.format(
            self, ch, ' '.join(repr(c) for c in chars)))
      if ch not in tracked:
        raise ValueError('{!r}: {!r} is scenery (or a piece of it), not a tracked thing: its cell '
                         'is not in the trace; the tracked things are {}'.format(
                             self, ch, ' '.join(repr(c) for c in tracked)))
      thing = tracked.index(ch)
    else:
      r0, c0 = self.centre
    pad_layer = -1
    if self.pad is not None:
      if self.pad not in chars:
        raise ValueError('{!r}: the game has no character {!r} to pad with (its characters: {})'
                         .format(self, self.pad, ' '.join(repr(c) for c in chars)))
      pad_layer = chars.index(self.pad)
    return Resolved(thing, r0, c0, pad_layer)
