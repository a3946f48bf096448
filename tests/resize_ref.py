"""Shared by tests/test_resize_host.py and tests/test_gpu_resize.py: the size pairs of DESIGN 19, the test images, Pillow itself as the
reference, and a numpy evaluation of dataloader.preprocess.pil_resize_table in Pillow's pass order."""
import numpy as np
from PIL import Image

from dataloader import preprocess

# (source (H, W), target (H, W))
CASES = (
    ((64, 32), (32, 16)),    # the halving
    ((64, 32), (128, 64)),   # up by two
    ((64, 32), (24, 12)),    # 8 / 3: 11 taps
    ((40, 24), (64, 40)),    # up, another ratio per axis
    ((64, 32), (16, 8)),     # the limit of 4: 16 taps
    ((48, 20), (48, 12)),    # equal height: the vertical pass is skipped
    ((37, 23), (50, 9)),     # odd byte strides; up along one axis, down along the other
    ((64, 32), (13, 7)),     # beyond the kernels' limit (host table only): 20 taps
)
KINDS = ('random', 'binary')


def image(kind, H, W, seed=0):
  """(H, W, 3) uint8: uniform bytes, or only 0 and 255 -- there the negative lobes clip at both ends."""
  r = np.random.RandomState(1000 * H + W + seed)
  if kind == 'random':
    return r.randint(0, 256, (H, W, 3)).astype(np.uint8)
  blocks = r.randint(0, 2, (-(-H // 5), -(-W // 3), 3)) * 255  # flat 5 x 3 blocks: the filter over- and undershoots at their edges
  return np.repeat(np.repeat(blocks, 5, 0), 3, 1)[:H, :W].astype(np.uint8)


CLIPS = [0, 0]  # sums below 0 / above 255 that one_pass has clipped so far


def pil_resize(a, H, W):
  """Pillow's own answer for one (Hs, Ws, 3) uint8 image."""
  return np.asarray(Image.fromarray(a).resize((W, H)))


def one_pass(a, n_out, axis):
  """One pass of Resample.c along `axis` of a (H, W, 3) uint8 array with the coefficients of pil_resize_table, in int64 (no product
  or sum here leaves 32 bits: 17 taps x 255 x 2^23)."""
  n = a.shape[axis]
  xmin, count, kk = preprocess.pil_resize_table(n, n_out)
  src = np.moveaxis(a, axis, 0).astype(np.int64)
  out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
  for i in range(n_out):
    acc = np.full(src.shape[1:], 1 << (preprocess.PIL_PRECISION_BITS - 1), dtype=np.int64)
    for j in range(count[i]):
      acc += src[xmin[i] + j] * int(kk[i, j])
    v = acc >> preprocess.PIL_PRECISION_BITS
    CLIPS[0] += int((v < 0).sum())
    CLIPS[1] += int((v > 255).sum())
    out[i] = np.clip(v, 0, 255)
  return np.moveaxis(out, 0, axis)


def two_pass(a, H, W):
  """Image.resize((W, H)) restated: the horizontal pass first, stored in 8 bits; a pass whose size does not change is skipped."""
  if a.shape[1] != W:
    a = one_pass(a, W, 1)
  if a.shape[0] != H:
    a = one_pass(a, H, 0)
  return a
