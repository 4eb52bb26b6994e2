"""The oracle of the observation windows (include/campx_hip.h has the rule): a window is a crop
of the full observation, taken here by pad-and-index in torch - the only way to get one without
the window kernel."""

import torch


def crop(full, r0, c0, h, w, pad_layer=None):
  """`full` [N, L, H, W] -> [N, L, h, w]: the cells (r0[i] + y, c0[i] + x) of row i; off the board
  0, or 1 in layer `pad_layer`.  `r0`, `c0`: ints, or integer tensors [N]."""
  N, L, H, W = full.shape
  big = torch.zeros((N, L, H + 2 * h, W + 2 * w), dtype=full.dtype, device=full.device)
  if pad_layer is not None and pad_layer >= 0:
    big[:, pad_layer] = 1
  big[:, :, h:h + H, w:w + W] = full
  r0 = torch.as_tensor(r0, device=full.device).expand(N).long()
  c0 = torch.as_tensor(c0, device=full.device).expand(N).long()
  # a corner further out than one window from the board shows padding only: clamp it to there
  rows = (r0.clamp(-h, H) + h)[:, None] + torch.arange(h, device=full.device)[None, :]      # [N, h]
  cols = (c0.clamp(-w, W) + w)[:, None] + torch.arange(w, device=full.device)[None, :]      # [N, w]
  n = torch.arange(N, device=full.device)[:, None, None, None]
  l = torch.arange(L, device=full.device)[None, :, None, None]
  return big[n, l, rows[:, None, :, None], cols[:, None, None, :]]


def centres(entries, W, HW, h, w):
  """Top-left cells (r0, c0) of the egocentric windows of trace entries (any integer tensor):
  cell = entry & 0x3ff clamped to HW - 1, (cy, cx) = divmod(cell, W), minus (h // 2, w // 2).
  The `shows` bit is not consulted."""
  cell = (entries.long() & 0x3ff).clamp(max=HW - 1)
  return cell // W - h // 2, cell % W - w // 2
