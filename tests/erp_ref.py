"""Host restatement of the 3D60 ingest kernels' arithmetic (csrc/erp_ingest.hip), in numpy.

bilinear() is the re-projection with the bits of torch's CPU F.grid_sample(bilinear, border, align_corners=True): float32 operations
in the order of include/mode_hip.h, the fused multiply-adds taken through float64 (the product of two float32 is exact in float64; the
sum is rounded to float64 and then to float32).    That second rounding could in principle differ from a true fused multiply-add (double
rounding); over the fixture's cases (tests/golden/erp3d60.npz: 6 x 2 images, 6 x 2 depth maps) and the hand-made grids of
tests/test_gpu_erp3d60.py no such difference shows -- tests/test_erp3d60_host.py compares every value with the reference's output bit
for bit.  depth2disp() restates the reference's __depth2disp (dataloader/dataset3D60Loader.py:258-270) on plain arrays."""
import numpy as np

F32 = np.float32


def _fma(a, b, c):
  return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def taps(grid, Hs, Ws):
  """grid (..., 2) float32 of normalised (x, y) -> (x0, y0 int, nw, ne, sw, se float32, x1ok, y1ok bool)."""
  g = np.asarray(grid, dtype=F32)
  out = []
  for v, size in ((g[..., 0], Ws), (g[..., 1], Hs)):
    c = (v + F32(1)) * (F32(size - 1) / F32(2))
    c = np.minimum(np.maximum(c, F32(0)), F32(size - 1))
    c0 = np.floor(c)
    e = c - c0
    out.append((c0.astype(np.int64), e, F32(1) - e, c0.astype(np.int64) + 1 < size))
  (x0, ex, wx, x1ok), (y0, ey, wy, y1ok) = out
  return x0, y0, wx * wy, ex * wy, wx * ey, ex * ey, x1ok, y1ok


def bilinear(img, grid):
  """img (Hs, Ws) or (Hs, Ws, C), any real dtype -> float32 (H, W) or (H, W, C) sampled at grid (H, W, 2)."""
  a = np.asarray(img).astype(F32)
  flat = a.ndim == 2
  if flat:
    a = a[:, :, None]
  Hs, Ws = a.shape[:2]
  x0, y0, nw, ne, sw, se, x1ok, y1ok = taps(grid, Hs, Ws)
  x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
  zero = F32(0)
  p_nw = a[y0, x0]
  p_ne = np.where(x1ok[..., None], a[y0, x1], zero)  # corners outside the image count as 0 (their weight is 0)
  p_sw = np.where(y1ok[..., None], a[y1, x0], zero)
  p_se = np.where((x1ok & y1ok)[..., None], a[y1, x1], zero)
  w = [t[..., None] for t in (nw, ne, sw, se)]
  v = _fma(p_se, w[3], _fma(p_sw, w[2], _fma(p_ne, w[1], p_nw * w[0])))
  return v[..., 0] if flat else v


def cassini_u8(img_u8, grid):
  """erp2rect_cassini(img, ...).astype(np.uint8) of an 8-bit image."""
  return bilinear(img_u8, grid).astype(np.uint8)


def cassini_phi(width):
  return np.arange(0.5 * np.pi - (0.5 * np.pi / width), -0.5 * np.pi, -(np.pi / width)).astype(F32)


def depth2disp(depth, baseline=0.26, max_depth=20.0):
  """(H, W) float32 Cassini depth (already thresholded) -> float32 disparity: NaN where depth <= 0 or > max_depth, negative -> 0.
  The types are numpy 2's for the reference's expression, written out so that they do not depend on the numpy that runs this: the
  products of two float32 arrays (d * sin(phi), d * d) are float32, everything after the first Python scalar is float64, and the
  result is rounded to float32 once (what the kernel stores)."""
  depth = np.asarray(depth, dtype=F32)
  W = depth.shape[-1]
  phi = np.broadcast_to(cassini_phi(W), depth.shape)
  bad = (depth <= 0) | (depth > max_depth)
  d = np.where(bad, F32(1), depth)
  b, f64 = float(baseline), np.float64
  with np.errstate(invalid='ignore', divide='ignore'):
    c = np.cos(phi + F32(np.pi / 2))  # float32, as numpy rounds it
    num = (d * np.sin(phi)).astype(f64) + b
    den = ((d * d).astype(f64) + b * b) - ((2.0 * d.astype(f64)) * b) * c.astype(f64)
    disp = W * (np.arcsin(np.clip(num / np.sqrt(den), -1, 1)) - phi.astype(f64)) / np.pi
  disp[disp < 0] = 0
  return np.where(bad, F32(np.nan), disp.astype(F32)).astype(F32)


def disparity(depth_erp, grid, baseline=0.26, max_depth=20.0, mirror=False):
  """mode_erp_depth_disp on one map: -> (disp (H, W), thresholded Cassini depth (H, W))."""
  d = bilinear(depth_erp, grid)
  if mirror:
    d = np.ascontiguousarray(d[:, ::-1])
  d[d > max_depth] = 0
  return depth2disp(d, baseline, max_depth), d


def norm_lookup(u8):
  """(H, W, 3) bytes -> (3, H, W) float32 by the table of dataloader.preprocess.norm_table (what the kernels look up)."""
  import torch
  from dataloader import preprocess
  lut = preprocess.norm_table().numpy()
  return torch.from_numpy(np.stack([lut[u8[..., c], c] for c in range(3)]))


def hand_made():
  """A small odd-sized case whose grid holds -1, +1, values beyond both (the border clamp), points exactly on the last row and
  column and one ulp inside the corners: -> (pairs_u8 (2, 2, 7, 9, 3), depth (2, 7, 9), grid (5, 8, 2))."""
  He, We, H, W, N = 7, 9, 5, 8, 2
  rng = np.random.RandomState(5)
  u8 = rng.randint(0, 256, (N, 2, He, We, 3)).astype(np.uint8)
  u8[0, 0, :4, :5] = 255
  depth = (25 * rng.rand(N, He, We)).astype(F32)
  depth[:, :3, :3] = 0  # with grid[4, 0] = (-1, -1): an invalid pixel, whatever the seed
  grid = (rng.rand(H, W, 2) * 2 - 1).astype(F32)
  grid[0, :, 0] = [-1, 1, -1.5, 1.5, -1, 1, 0, 0.25]
  grid[0, :, 1] = [-1, 1, 1, -1, -3, 7, 1, -1]
  grid[1, :, 0] = F32(2) * np.arange(8, dtype=F32) / F32(We - 1) - F32(1)  # the pixel centres of columns 0 .. 7
  grid[1, :, 1] = 1  # the last row
  grid[2, :, 0] = 1  # the last column
  grid[2, :, 1] = np.linspace(-1, 1, 8).astype(F32)
  grid[3, 0] = np.nextafter(F32(1), F32(0))  # one ulp inside the last pixel
  grid[3, 1] = np.nextafter(F32(-1), F32(0))
  grid[4, 0] = (-1, -1)
  return u8, depth, grid
