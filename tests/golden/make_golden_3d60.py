#!/usr/bin/env python3
"""Golden vectors for the 3D60 ingest, made by the REFERENCE's own Dataset3D60Disparity.__getitem__
(dataloader/dataset3D60Loader.py:123-248) on files this script writes to a temporary directory.

  python tests/golden/make_golden_3d60.py [path/to/reference]      # writes tests/golden/erp3d60.npz

The RGB panoramas are PNGs written by PIL; the depth maps are .npy files stored under the .exr names of the list file.

Harness stand-ins (no reference file is edited or copied; they live only in this script):
  numba                    `jit` returns the function unchanged (utils/geometry.py imports it; the decorated loop is not used here).
  cv2                      four functions: Rodrigues by formula (float64 arithmetic, result in the vector's dtype), imread = np.load,
                           resize = the identity (it is only ever asked for the size the image already has; anything else raises),
                           flip(a, 1) = a copy of a[:, ::-1]; and the constant IMREAD_ANYDEPTH.
  torchvision.transforms   the three classes dataloader/preprocess.py uses on this path: Compose, ToTensor (uint8 HWC array ->
                           float32 CHW / 255), Normalize ((t - mean) / std with float32 mean and std).  The module's other helpers are
                           only looked up when the augmenting transforms are built, which this path never does.
  dataloader               an empty package whose path is the reference's directory, so that dataset3D60Loader and preprocess are
                           imported without running the package's __init__ (which imports the Deep360 loaders).

What the reference pins here: the re-projection (utils.geometry.erp2rect_cassini on torch's CPU grid_sample), the truncation to
bytes, the order of thresholding and flipping, the normalisation, and the sine rule (__depth2disp).  What it does NOT pin:
cv2.Rodrigues itself for the two non-zero rotations ('ud', 'ur') -- the matrix here comes from the stand-in's formula, and the project's
utils.geometry.rodrigues evaluates the same formula; the identity of 'lr' is exact either way.

Two cases, each run as 'lr', 'ud' and 'ur': ERP 32 x 64 -> Cassini 64 x 32, and the odd ERP 30 x 61 -> Cassini 48 x 20.  Every RGB image
is random bytes with a flat block of 255 and a flat block of 0; every depth map lies in (0, 25] with 10 % zeros (so maxDepth = 20
bites), a block of zeros (isolated zeros rarely survive the interpolation as an exact 0; the block gives the invalid, NaN pixels) and a
patch of depths far below the baseline, where the sine rule saturates.  (In exact
arithmetic the rule never gives a negative disparity; `disp[disp < 0] = 0` only catches rounding, and at these sizes no pixel needs it:
the script prints the count of zero disparities, 0 in every case.)

The stored disparities are float64: under numpy 2 a masked array combined with a Python scalar (`depth_not_0 * sin + self.baseline`)
is promoted to float64, where numpy 1 -- which the reference was written against -- stayed in float32.  The reference therefore pins the
NaN set and the values to rounding, not a float32 bit pattern; the tests compare disparities within the project's 1e-3 px bound.

Stored per case: the ERP inputs; per pair the grid the reference sampled with (recorded from its own F.grid_sample call), the float
re-projection of the left image before truncation, the float re-projection of both depth maps, the byte images and the six tensors of
the returned item; and the versions of the libraries that made them."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
CASES = (('a', (32, 64), (64, 32)), ('b', (30, 61), (48, 20)))  # tag, ERP (He, We), Cassini (H, W)
PAIRS = ('lr', 'ud', 'ur')


def _rodrigues(v):
  v = np.asarray(v)
  r = v.astype(np.float64).reshape(3)
  theta = float(np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
  if theta < np.finfo(np.float64).eps:
    return np.eye(3, dtype=v.dtype), None
  c, s = np.cos(theta), np.sin(theta)
  r = r / theta
  r_x = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
  return (c * np.eye(3) + (1 - c) * np.outer(r, r) + s * r_x).astype(v.dtype), None


def _resize(a, size):
  assert tuple(size) == (a.shape[1], a.shape[0]), (size, a.shape)
  return a


def _flip(a, code):
  assert code == 1
  return np.ascontiguousarray(a[:, ::-1])


class _Compose(object):
  def __init__(self, ts):
    self.ts = ts

  def __call__(self, x):
    for t in self.ts:
      x = t(x)
    return x


class _ToTensor(object):
  def __call__(self, pic):
    a = np.asarray(pic)
    assert a.dtype == np.uint8 and a.ndim == 3
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)


class _Normalize(object):
  def __init__(self, mean, std):
    self.mean, self.std = mean, std

  def __call__(self, t):
    mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
    std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
    return t.clone().sub_(mean).div_(std)


def _install_stand_ins():
  numba = types.ModuleType('numba')
  numba.jit = lambda *a, **k: (lambda f: f)
  cv2 = types.ModuleType('cv2')
  cv2.Rodrigues, cv2.imread, cv2.resize, cv2.flip, cv2.IMREAD_ANYDEPTH = _rodrigues, (lambda path, flags=None: np.load(path)), _resize, _flip, 2
  tv = types.ModuleType('torchvision')
  tr = types.ModuleType('torchvision.transforms')
  tr.Compose, tr.ToTensor, tr.Normalize = _Compose, _ToTensor, _Normalize
  tv.transforms = tr
  pkg = types.ModuleType('dataloader')
  pkg.__path__ = [os.path.join(REF, 'dataloader')]
  sys.modules.update({'numba': numba, 'cv2': cv2, 'torchvision': tv, 'torchvision.transforms': tr, 'dataloader': pkg})
  sys.path.insert(0, REF)


def _rgb(rng, he, we):
  a = rng.randint(0, 256, (he, we, 3)).astype(np.uint8)
  a[he // 8:he // 8 + he // 3, we // 10:we // 10 + we // 3] = 255
  a[he // 2:he // 2 + he // 4, we // 2:we // 2 + we // 3] = 0
  return a


def _depth(rng, he, we):
  d = (25.0 * (1.0 - rng.rand(he, we))).astype(np.float32)  # (0, 25]
  d[rng.rand(he, we) < 0.1] = 0
  d[he // 3:he // 3 + 5, we // 4:we // 4 + 9] = (0.002 + 0.05 * rng.rand(5, 9)).astype(np.float32)  # far below the 0.26 baseline
  d[2 * he // 3:2 * he // 3 + 5, we // 2:we // 2 + 9] = 0  # a block of invalid pixels: isolated zeros do not survive the interpolation
  return d


def main():
  _install_stand_ins()
  geo = importlib.import_module('utils.geometry')
  mod = importlib.import_module('dataloader.dataset3D60Loader')
  seen = []
  real_sample = geo.F.grid_sample

  def recording_sample(src, grid, **kw):
    out = real_sample(src, grid, **kw)
    seen.append((grid[0].numpy().copy(), out))
    return out

  rng = np.random.RandomState(3060)
  out = {'versions': np.array(['numpy ' + np.__version__, 'torch ' + torch.__version__, 'Pillow ' + PIL.__version__])}
  with tempfile.TemporaryDirectory() as root:
    for tag, (he, we), (h, w) in CASES:
      names = []
      for view, sub in (('l', 'Center_Left_Down'), ('r', 'Right'), ('u', 'Up')):
        os.makedirs(os.path.join(root, sub, tag), exist_ok=True)
        rgb, depth = _rgb(rng, he, we), _depth(rng, he, we)
        out['%s/rgb_%s' % (tag, view)], out['%s/depth_%s' % (tag, view)] = rgb, depth
        Image.fromarray(rgb).save(os.path.join(root, sub, tag, 'color.png'))
        with open(os.path.join(root, sub, tag, 'depth.exr'), 'wb') as f:
          np.save(f, depth)
      listfile = os.path.join(root, tag + '.txt')
      with open(listfile, 'w') as f:
        f.write(' '.join(['./%s/color.png' % tag] * 3 + ['./%s/depth.exr' % tag] * 3) + '\n')
      for pair in PAIRS:
        ds = mod.Dataset3D60Disparity(listfile, rootDir=root, curStage='training', shape=(h, w), crop=False, pair=pair, flip=True, maxDepth=20.0)
        del seen[:]
        geo.F.grid_sample = recording_sample
        try:
          item = ds[0]
        finally:
          geo.F.grid_sample = real_sample
        assert len(seen) == 4  # left RGB, right RGB, left depth, right depth
        key = '%s/%s/' % (tag, pair)
        out[key + 'grid'] = seen[0][0]
        assert all(np.array_equal(g, seen[0][0]) for g, _ in seen)
        out[key + 'left_f32'] = seen[0][1][0].permute(1, 2, 0).numpy().copy()  # (H, W, 3): the re-projection before truncation
        out[key + 'depth_left_f32'], out[key + 'depth_right_f32'] = seen[2][1][0, 0].numpy().copy(), seen[3][1][0, 0].numpy().copy()
        out[key + 'left_u8'] = seen[0][1][0].permute(1, 2, 0).numpy().astype(np.uint8)
        out[key + 'right_u8'] = seen[1][1][0].permute(1, 2, 0).numpy().astype(np.uint8)
        for k in ('leftImg', 'rightImg', 'dispMap', 'leftImg_flip', 'rightImg_flip', 'dispMap_flip'):
          out[key + k] = item[k].numpy().copy()
        nz = int((item['dispMap'].numpy() == 0).sum())
        print('%s %s: %d NaN, %d zero disparities, %d bytes 254 in the left image' %
              (tag, pair, int(np.isnan(item['dispMap'].numpy()).sum()), nz, int((out[key + 'left_u8'] == 254).sum())))
  path = os.path.join(HERE, 'erp3d60.npz')
  np.savez_compressed(path, **out)
  print('wrote erp3d60.npz with %d arrays, %d bytes' % (len(out), os.path.getsize(path)))


if __name__ == '__main__':
  main()
