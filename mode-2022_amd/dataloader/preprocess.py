"""Input normalisation (reference dataloader/preprocess.py:8, 49-76): ToTensor + Normalize, without torchvision.

Only the non-augmented transforms exist as host transforms (Deep360DatasetDisparity / Deep360DatasetFusion build them with
augment=False, deep360_loader.py:77, 157, 161).  The colour-jitter + PCA-lighting augmentation of preprocess.py:33-46 is a device
call on 8-bit images -- dataloader.gpu_ingest.draw_colour_params + augment_u8_gpu, or frames_u8_gpu / erp_pairs_gpu with augment=
 -- and the package has no CPU path, so asking for it here still raises."""
import numpy as np
import torch

imagenet_stats = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}
deep360_stats = {'mean': [0], 'std': [1]}


def to_tensor(pic):
  """torchvision's ToTensor: PIL image or (H, W, C) array -> float32 (C, H, W); uint8 input is scaled by 1/255, other dtypes
  are kept as they are (so float32 depth maps pass through unscaled, as in the reference)."""
  a = np.asarray(pic)
  if a.ndim == 2:
    a = a[:, :, None]
  t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
  return t.to(torch.float32).div(255) if a.dtype == np.uint8 else t


class _Normalize(object):
  def __init__(self, mean, std):
    self.mean, self.std = mean, std

  def __call__(self, pic):
    t = to_tensor(pic)
    mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
    std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
    return (t - mean) / std


def color_normalize(normalize=imagenet_stats):
  return _Normalize(**normalize)


def depth_normalize(normalize=deep360_stats):
  return _Normalize(**normalize)


def get_transform_stage1(name='imagenet', normalize=None, augment=True):
  """RGB transform (preprocess.py:64-69); `normalize` is ignored there too (always the ImageNet statistics)."""
  if augment:
    raise NotImplementedError('the colour augmentation of preprocess.py:33-46 has no host transform here: it runs on the GPU, on 8-bit '
                              'images (dataloader.gpu_ingest.draw_colour_params and augment_u8_gpu / frames_u8_gpu(augment=...))')
  return color_normalize(imagenet_stats)


def get_transform_stage2(name='deep360', normalize=None, augment=False):
  """Depth transform (preprocess.py:72-74): to tensor, mean 0 / std 1."""
  return depth_normalize(deep360_stats)


def norm_table(name='imagenet'):
  """(256, 3) float32: row v = get_transform_stage1(augment=False) of a pixel whose three channels hold v -- the transform itself run
  over the 256 byte values, so that a lookup has its bits (mode_frames_u8_ingest / mode_rgb_half_pil only look values up)."""
  ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # (256, 1, 3): an image holding every value in every channel
  return get_transform_stage1(name, augment=False)(ramp)[:, :, 0].t().contiguous()


def _pil_bicubic(x):
  """Pillow's bicubic_filter (Resample.c, a = -0.5) in double."""
  a = -0.5
  x = abs(x)
  if x < 1.0:
    return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
  if x < 2.0:
    return (((x - 5) * x + 8) * x - 4) * a
  return 0.0


PIL_PRECISION_BITS = 32 - 8 - 2  # Resample.c: 8-bit pixels, 2 bits of headroom for the bicubic overshoot


def pil_half_table(n):
  """The coefficients of one pass of PIL.Image.resize to n // 2 out of n (the fusion loader's --resize, reference
  dataloader/deep360_loader.py:151-153), as Pillow's Resample.c builds them for 8-bit images (precompute_coeffs with the default
  bicubic filter, scale 2, support 4, then normalize_coeffs_8bpc): -> (xmin (n/2,) int32, count (n/2,) int32, kk (n/2, 8) int32).
  Output i is clip((2^21 + sum_{j < count[i]} px[xmin[i] + j] * kk[i, j]) >> 22, 0, 255).  All arithmetic in double, in Pillow's
  order; rows past count are zero.  Only five distinct rows exist: two at each edge and the 8-tap interior one."""
  if n < 2 or n % 2:
    raise ValueError('pil_half_table: %r is not a positive even size (Pillow halves other sizes with another scale)' % (n,))
  out, scale, support = n // 2, 2.0, 4.0
  xmin = np.zeros(out, dtype=np.int32)
  count = np.zeros(out, dtype=np.int32)
  kk = np.zeros((out, 8), dtype=np.int32)
  for i in range(out):
    center = (i + 0.5) * scale
    lo = max(0, int(center - support + 0.5))
    hi = min(n, int(center + support + 0.5))
    k = [_pil_bicubic((j + lo - center + 0.5) / scale) for j in range(hi - lo)]
    ww = 0.0
    for v in k:
      ww += v
    k = [v / ww for v in k] if ww != 0.0 else k
    xmin[i], count[i] = lo, hi - lo
    kk[i, :hi - lo] = [int(-0.5 + v * (1 << PIL_PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PIL_PRECISION_BITS)) for v in k]
  return xmin, count, kk


def pil_resize_table(n, out):
  """The coefficients of one pass of PIL.Image.resize from n to out along an axis, for any pair of sizes (the disparity loader's resize
  to the working size, reference dataloader/deep360_loader.py:92-97), as Pillow's Resample.c builds them for 8-bit images
  (precompute_coeffs with the default bicubic filter, then normalize_coeffs_8bpc):
  -> (xmin (out,) int32, count (out,) int32, kk (out, ksize) int32), ksize = 2 ceil(2 max(n / out, 1)) + 1.
  Output i is clip((2^21 + sum_{j < count[i]} px[xmin[i] + j] * kk[i, j]) >> 22, 0, 255).  pil_half_table's arithmetic in its order,
  with Pillow's general scale: the filter argument is multiplied by 1 / max(n / out, 1), the sum and the normalisation are in double,
  the fixed point is rounded away from zero; entries past count are zero.  pil_resize_table(n, n // 2) is pil_half_table(n) with a ninth,
  zero column.  Pillow runs the horizontal pass first, stores it in 8 bits, and skips a pass whose size does not change."""
  if n < 1 or out < 1:
    raise ValueError('pil_resize_table: sizes must be positive, got %r -> %r' % (n, out))
  scale = n / out
  filterscale = max(scale, 1.0)
  support = 2.0 * filterscale
  ksize = 2 * int(np.ceil(support)) + 1
  ss = 1.0 / filterscale
  xmin = np.zeros(out, dtype=np.int32)
  count = np.zeros(out, dtype=np.int32)
  kk = np.zeros((out, ksize), dtype=np.int32)
  for i in range(out):
    center = (i + 0.5) * scale
    lo = max(0, int(center - support + 0.5))
    hi = min(n, int(center + support + 0.5))
    k = [_pil_bicubic((j + lo - center + 0.5) * ss) for j in range(hi - lo)]
    ww = 0.0
    for v in k:
      ww += v
    k = [v / ww for v in k] if ww != 0.0 else k
    xmin[i], count[i] = lo, hi - lo
    kk[i, :hi - lo] = [int(-0.5 + v * (1 << PIL_PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PIL_PRECISION_BITS)) for v in k]
  return xmin, count, kk


def nearest_index_table(src, dst):
  """(dst,) int32: the source index that cv2.resize(..., INTER_NEAREST) copies into destination index i along an axis,
  min(floor(i * (src / dst)), src - 1) in double -- deep360_loader.resize_nearest's indices."""
  if src < 1 or dst < 1:
    raise ValueError('nearest_index_table: sizes must be positive, got %r -> %r' % (src, dst))
  return np.minimum(np.floor(np.arange(dst) * (src / dst)).astype(np.int64), src - 1).astype(np.int32)
