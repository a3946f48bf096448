"""Sampling tables for the tests of the windowed spherical kernels' plans.  TEST INFRASTRUCTURE.

A Cassini table is shift-invariant along its row axis (row coordinate = h + f_k(w) modulo H), so every geometric table shows the
planners of csrc/sphere_plan.hip the same pattern in every row block.  The synthetic tables here are not: they reach the branches a
geometric table leaves to a handful of tiles (halves_fit failing, no polar items, six-source adjoint tiles, lists longer than six, the
LDS limit of the wrap-around window, dead taps).

Every table built is kept alive in TABLES: the plan caches of mode_hip.functional are keyed by the table's address."""
import numpy as np
import torch

from oracle import mode_ref

TABLES = {}

# sphere_position(ih, iw, 'Cassini') -> a table of iw rows x ih columns
GEOMETRIC = [(36, 72), (72, 144), (81, 162), (96, 192), (100, 200), (128, 256), (160, 320), (192, 384), (256, 512)]
TAPS = [(dh, dw) for dh in (-1, 0, 1) for dw in (-1, 0, 1)]


def _keep(name, make):
  if name not in TABLES:
    t = make().to(torch.float32).contiguous()
    assert t.dim() == 4 and t.shape[0] == 1 and t.shape[1] == 18
    TABLES[name] = t
  return TABLES[name]


def geometric(ih, iw):
  return _keep('cassini %dx%d' % (iw, ih), lambda: mode_ref.sphere_position(ih, iw, 'Cassini'))


def perturbed(ih=96, iw=192):
  """The geometric table with 0.45 sin(2 pi h / H) added to every row coordinate and 0.3 cos(2 pi h / H) to every column coordinate:
  no longer shift-invariant in h."""
  def make():
    t = mode_ref.sphere_position(ih, iw, 'Cassini').clone()
    H = t.shape[2]
    ang = 2 * np.pi * torch.arange(H, dtype=torch.float64) / H
    t[0, 0::2] += (0.45 * torch.sin(ang)).to(torch.float32).view(1, H, 1)
    t[0, 1::2] += (0.3 * torch.cos(ang)).to(torch.float32).view(1, H, 1)
    return t
  return _keep('perturbed %dx%d' % (iw, ih), make)


def affine(a, H=192, W=16, fh=0.3, fw=0.3, b=1.0):
  """Row coordinate a * h + dh + fh, column coordinate b * w + dw + fw for the tap (dh, dw) in {-1, 0, 1}^2.  With 0 < fh, fw < 1 the
  first row and column of the tap -1 have coordinates in (-1, 0) (the shifted-corner branch of the record arithmetic), and for a = 1 the
  last row of the tap 0 lies in (H - 1, H); coordinates >= H or W are dead taps."""
  def make():
    t = torch.zeros((1, 18, H, W), dtype=torch.float64)
    h = torch.arange(H, dtype=torch.float64).view(H, 1)
    w = torch.arange(W, dtype=torch.float64).view(1, W)
    for k, (dh, dw) in enumerate(TAPS):
      t[0, 2 * k] = a * h + dh + fh
      t[0, 2 * k + 1] = b * w + dw + fw
    return t
  return _keep('affine a=%g b=%g %dx%d f=(%g, %g)' % (a, b, H, W, fh, fw), make)


def sixteen_source(H=128, W=16):
  """Row and column scale 0.25 inside every 64 x 4 tile (row coordinate 64 (h // 64) + (h % 64) / 4 + dh + fh, column coordinate
  4 (w // 4) + (w % 4) / 4 + dw + fw): sixteen output pixels share every source, so every tile has adjoint lists longer than six."""
  def make():
    t = torch.zeros((1, 18, H, W), dtype=torch.float64)
    h = torch.arange(H, dtype=torch.float64).view(H, 1)
    w = torch.arange(W, dtype=torch.float64).view(1, W)
    for k, (dh, dw) in enumerate(TAPS):
      t[0, 2 * k] = 64 * torch.floor(h / 64) + (h % 64) / 4 + dh + 0.3
      t[0, 2 * k + 1] = 4 * torch.floor(w / 4) + (w % 4) / 4 + dw + 0.3
    return t
  return _keep('sixteen sources %dx%d' % (H, W), make)


def dead_taps(ih=96, iw=192, seed=5):
  """The geometric table with NaN, +inf, -inf, exactly -1 and exactly H (row) / W (column) coordinates sprinkled in: all dead taps."""
  def make():
    t = mode_ref.sphere_position(ih, iw, 'Cassini').clone()
    H, W = t.shape[2:]
    r = np.random.RandomState(seed)
    for value in (float('nan'), float('inf'), -float('inf'), -1.0, None):
      for _ in range(40):
        k, h, w, which = r.randint(9), r.randint(H), r.randint(W), r.randint(2)
        t[0, 2 * k + which, h, w] = (float(H), float(W))[which] if value is None else value
    return t
  return _keep('dead taps %dx%d' % (iw, ih), make)


def clustered(H=192, W=16):
  """Integer coordinates that send three output rows and two output columns to ONE source pixel in the columns w < 8 (row coordinate
  h - h % 3 + dh, column coordinate w - w % 2 + dw) and the identity h + dh, w + dw in the columns beyond: every adjoint list of the left
  half has six entries of weight exactly 1 inside one 81 x 8 window -- short and compact enough for the windowed input gradient, and
  three times what its fp16 form can take (a weight sum <= 2 - 2^-10 per list); the right half has lists of one entry."""
  def make():
    t = torch.zeros((1, 18, H, W), dtype=torch.float64)
    h = torch.arange(H, dtype=torch.float64).view(H, 1).expand(H, W)
    w = torch.arange(W, dtype=torch.float64).view(1, W).expand(H, W)
    left = w < 8
    for k, (dh, dw) in enumerate(TAPS):
      t[0, 2 * k] = torch.where(left, h - h % 3, h) + dh
      t[0, 2 * k + 1] = torch.where(left, w - w % 2, w) + dw
    return t
  return _keep('clustered %dx%d' % (H, W), make)
