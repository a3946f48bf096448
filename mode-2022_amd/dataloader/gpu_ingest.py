"""8-bit frames on the GPU: the host half of the reference's loaders between the decoded PNGs and the two networks, as HIP kernels.

  frames_u8_gpu   preprocess.get_transform_stage1(augment=False) of every panorama of (F, 12, H, W, 3) uint8 frames and
                  models.mode_multiview.split_frames of the result, in one launch (mode_frames_u8_ingest); with rig= the same for the
                  (F, 2P, H, W, 3) frames of any utils.rig.CameraRig, through the slot table of mode_images_u8_augment
  rgb_half_gpu    Deep360DatasetFusion(resize=True)'s RGB branch (reference dataloader/deep360_loader.py:151-153, 161-163):
                  PIL.Image.resize((w / 2, h / 2)) of the four fusion panoramas, then the same transform (mode_rgb_half_pil)
  erp_pairs_gpu   Dataset3D60Disparity.__getitem__ (reference dataloader/dataset3D60Loader.py:175-248) for a batch of decoded 3D60
                  samples: both ERP panoramas and both ERP depth maps re-projected to rectified Cassini, the images truncated to bytes
                  and normalised, the depth turned into the disparity ground truth, for the pair and its mirrored twin
                  (mode_erp_pairs_u8_cassini, mode_erp_depth_disp)

  augment_u8_gpu  preprocess.get_transform_stage1(augment=True) of the reference (dataloader/preprocess.py:33-46, 78-95): ColorJitter(0.4,
                  0.4, 0.4) and the PCA Lighting(0.1) between ToTensor and Normalize, on (N, H, W, 3) uint8 images, with the random
                  draws made on the host (draw_colour_params -> ColourParams) and everything per pixel on the device
                  (mode_images_u8_augment); frames_u8_gpu(augment=) and erp_pairs_gpu(augment=) run their images through it

  pairs_u8_gpu    Deep360DatasetDisparity(shape=...) for a batch of decoded pairs stored at another size (reference
                  dataloader/deep360_loader.py:92-109): PIL.Image.resize of both panoramas between any two sizes, the nearest-neighbour
                  resize of the disparity times the width ratio, the training crop (draw_crop_windows), the transform or the colour
                  augmentation (mode_images_u8_resize_pil, mode_disp_resize_nearest); resize_u8_gpu is its 8-bit resize alone

The first two are bit for bit what the host computes, and so are the images of the third (its disparities differ from numpy's by the
last bits of asin) and everything pairs_u8_gpu returns: the normalisation is a lookup in the table the host transform produces
for the 256 byte values (preprocess.norm_table), the resize Pillow's own fixed-point arithmetic on the coefficients of
preprocess.pil_half_table / pil_resize_table.
Tables are built and uploaded once per device / per (H, W, device) and cached, so the calls can be captured into a graph after a
first eager call.  Importing this module does not load the native library; there is no CPU path."""
import threading

import numpy as np
import torch

from mode_hip import functional as _HF

from . import preprocess
from .deep360_loader import CROP_H, CROP_W

_lut_cache = _HF._LRU(8)    # device -> (256, 3) float32 normalisation table (graph-pinned while captured)
_half_cache = _HF._LRU(8)   # (H, W, device) -> (tab_w (W/2, 10), tab_h (H/2, 10)) int32 tables of mode_rgb_half_pil
_erp_cache = _HF._LRU(16)   # (pair, H, W, device) -> grid (1, H, W, 2); ('cols', W, device) -> cols (3, W): the 3D60 ingest's tables
_dst_cache = _HF._LRU(8)    # (F, want_rgb, device) -> (12 F, 2) int32: the slots of every panorama of F frames in cat(left, right, rgb)
_resize_cache = _HF._LRU(16)  # ('pil' | 'nearest', n, out, device) -> one axis' table of mode_images_u8_resize_pil / mode_disp_resize_nearest
_lock = threading.Lock()


def _norm_lut(device):
  key = str(device)
  with _lock:
    hit = _lut_cache.get(key)
    if hit is None:
      hit = preprocess.norm_table().to(device)
      _lut_cache[key] = hit
    return hit


def half_table_rows(n):
  """pil_half_table(n) packed as the kernel reads it: (n / 2, 10) int32 rows [xmin, count, kk[0..7]]."""
  xmin, count, kk = preprocess.pil_half_table(n)
  return torch.from_numpy(np.ascontiguousarray(np.concatenate([xmin[:, None], count[:, None], kk], axis=1), dtype=np.int32))


def _half_tables(H, W, device):
  key = (H, W, str(device))
  with _lock:
    hit = _half_cache.get(key)
    if hit is None:
      hit = (half_table_rows(W).to(device), half_table_rows(H).to(device))
      _half_cache[key] = hit
    return hit


def frames_u8_gpu(frames_u8, want_rgb=True, augment=None, rig=None):
  """(F, 12, H, W, 3) uint8 device frames -- the 12 panoramas of a frame in sorted file order, each as np.asarray(PIL image) lays
  it out -> (left (6F, 3, H, W), right (6F, 3, H, W), rgb (F, 12, H, W) or None): split_frames of the ImageNet-normalised panoramas.
  augment: ColourParams for the 12 F panoramas (row 12 f + k: panorama k of frame f) -> the same three tensors of the colour-augmented
  panoramas (augment_u8_gpu): left, right and rgb are three parts of one buffer that mode_images_u8_augment writes through its slot
  table in one call (panoramas 0, 1, 10, 11 have two slots each: their pair and the fusion RGB).
  rig: a utils.rig.CameraRig of P pairs -> frames (F, 2P, H, W, 3), pair-major, and left, right (P F, 3, H, W) with pair p of frame f
  at row P f + p, rgb (F, 3 len(rig.rgb), H, W): split_frames(rig=) of the normalised panoramas, bit for bit.  Both the plain and the
  augmented ingest of a rig go through mode_images_u8_augment and the rig's slot table (plain: no operations, zero shifts, which is
  the normalisation alone)."""
  if rig is not None:
    return _rig_frames_u8(frames_u8, want_rgb, augment, rig)
  _HF.require_u8_frames(frames_u8, 'frames_u8_gpu')
  if augment is None:
    return _HF.frames_u8_ingest(frames_u8, _norm_lut(frames_u8.device), want_rgb)
  F, _, H, W, _ = frames_u8.shape
  _require_params(augment, 12 * F, frames_u8.device, 'frames_u8_gpu')
  all3 = torch.empty(((16 if want_rgb else 12) * F, 3, H, W), dtype=torch.float32, device=frames_u8.device)
  if F:
    _HF.images_u8_augment(frames_u8.view(12 * F, H, W, 3), augment.ops, augment.coef, dst=_frame_slots(F, want_rgb, frames_u8.device),
                          out=all3)
  return all3[:6 * F], all3[6 * F:12 * F], (all3[12 * F:].view(F, 12, H, W) if want_rgb else None)


def _frame_slots(F, want_rgb, device):
  """(12 F, 2) int32 on the device: where panorama k of frame f goes in cat(left, right, rgb viewed as (4 F, 3, H, W)) -- left[6 f + k / 2]
  for even k, right[...] for odd, and for k = 0, 1, 10, 11 with want_rgb also slot 4 f + (0, 1, 2, 3) of the fusion RGB; -1: no second slot."""
  key = (F, bool(want_rgb), str(device))
  with _lock:
    hit = _dst_cache.get(key)
    if hit is None:
      f, k = np.divmod(np.arange(12 * F), 12)
      second = np.where((k < 2) | (k >= 10), 12 * F + 4 * f + np.where(k < 2, k, k - 8), -1) if want_rgb else np.full(12 * F, -1)
      hit = torch.from_numpy(np.stack([(k & 1) * 6 * F + 6 * f + k // 2, second], 1).astype(np.int32)).to(device)
      _dst_cache[key] = hit
    return hit


def _rig_slots(F, rig, want_rgb, device):
  """_frame_slots for a utils.rig.CameraRig of P pairs with K RGB panoramas: (2P F, 2) int32, panorama k of frame f -> left[P f + k / 2]
  for even k, right[...] for odd, and for k = rig.rgb[r] with want_rgb also slot K f + r of the fusion RGB viewed as (K F, 3, H, W),
  behind the 2P F slots of left and right; -1: no second slot.  For CameraRig.deep360() it is _frame_slots row for row."""
  key = ('rig', rig, F, bool(want_rgb), str(device))
  with _lock:
    hit = _dst_cache.get(key)
    if hit is None:
      P, K = len(rig.pairs), len(rig.rgb)
      f, k = np.divmod(np.arange(2 * P * F), 2 * P)
      rank = np.full(2 * P, -1)
      rank[list(rig.rgb)] = np.arange(K)
      second = np.where(rank[k] >= 0, 2 * P * F + K * f + rank[k], -1) if want_rgb else np.full(2 * P * F, -1)
      hit = torch.from_numpy(np.stack([(k & 1) * P * F + P * f + k // 2, second], 1).astype(np.int32)).to(device)
      _dst_cache[key] = hit
    return hit


def _identity_params(n, device):
  """ColourParams of n images with no operation and zero shifts (the normalisation alone), cached per (n, device)."""
  key = ('identity', n, str(device))
  with _lock:
    hit = _dst_cache.get(key)
  if hit is None:
    hit = ColourParams([[]] * n, np.ones((n, 3)), None, device)
    with _lock:
      _dst_cache[key] = hit
  return hit


def _rig_frames_u8(frames_u8, want_rgb, augment, rig):
  who = 'frames_u8_gpu'
  P, K = len(rig.pairs), len(rig.rgb)
  if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8:
    raise TypeError('%s: frames must be a uint8 tensor (got %s)' % (who, getattr(frames_u8, 'dtype', type(frames_u8))))
  _HF.require_gpu(frames_u8)
  if not frames_u8.is_contiguous():
    raise TypeError('%s: frames must be contiguous' % who)
  if frames_u8.dim() != 5 or frames_u8.shape[1] != 2 * P or frames_u8.shape[4] != 3:
    raise ValueError('%s: frames of a rig with %d pairs must be (F, %d, H, W, 3), got %s' % (who, P, 2 * P, tuple(frames_u8.shape)))
  F, _, H, W, _ = frames_u8.shape
  dev = frames_u8.device
  if augment is None:
    augment = _identity_params(2 * P * F, dev)
  else:
    _require_params(augment, 2 * P * F, dev, who)
  all3 = torch.empty(((2 * P + (K if want_rgb else 0)) * F, 3, H, W), dtype=torch.float32, device=dev)
  if F:
    _HF.images_u8_augment(frames_u8.view(2 * P * F, H, W, 3), augment.ops, augment.coef, dst=_rig_slots(F, rig, want_rgb, dev), out=all3)
  return all3[:P * F], all3[P * F:2 * P * F], (all3[2 * P * F:].view(F, 3 * K, H, W) if want_rgb else None)


# ------------------------------------------------------------------------------------ colour augmentation
# The reference's __imagenet_pca (dataloader/preprocess.py:10-25), float32 as torch.Tensor([...]) rounds them.
PCA_EIGVAL = torch.tensor([0.2175, 0.0188, 0.0045], dtype=torch.float32)
PCA_EIGVEC = torch.tensor([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]], dtype=torch.float32)
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_NONE = 0, 1, 2, 3, -1


def lighting_shift(alpha, eigval=PCA_EIGVAL, eigvec=PCA_EIGVEC):
  """Lighting's per-channel shift (reference preprocess.py:90-93) with its float32 torch operations in its order:
  shift[c] = sum_j (eigvec[c][j] * alpha[j]) * eigval[j]."""
  alpha = torch.as_tensor(alpha, dtype=torch.float32)
  return ((eigvec * alpha.view(1, 3)) * eigval.view(1, 3)).sum(1)


class ColourParams(object):
  """The device tables of mode_images_u8_augment for n images, built from host values:
    order    n rows of up to three operation codes in the order they are applied (OP_BRIGHTNESS 0, OP_CONTRAST 1, OP_SATURATION 2;
             OP_NONE -1 or a shorter row: fewer operations).  An operation appears at most once in a row; OP_HUE is refused (the
             reference's ColorJitter call has no hue).
    factors  (n, 3): brightness, contrast and saturation factor of every image, >= 0 (1 = identity; read only where the row names
             the operation).
    shifts   (n, 3) float32: Lighting's per-channel shift (lighting_shift), or None = zero.
  ops (n, 3) int32 and coef (n, 9) float32 are the device tensors; ops_host / coef_host the same values on the host.  coef holds per
  operation rho = float32(factor) and sigma = float32(1.0 - factor), the difference formed in double as torch forms it for a Python
  scalar.  copy_from(other) refills the device tensors in place, so that a captured graph can be replayed with new draws."""

  def __init__(self, order, factors, shifts=None, device='cuda'):
    self.ops_host, self.coef_host = self._tables(order, factors, shifts)
    self.n = self.ops_host.shape[0]
    self.device = torch.device(device)
    self.ops = self.ops_host.to(self.device)
    self.coef = self.coef_host.to(self.device)

  @staticmethod
  def _tables(order, factors, shifts):
    order = [list(int(c) for c in row) for row in order]
    n = len(order)
    factors = np.asarray(factors, dtype=np.float64).reshape(-1, 3) if n else np.zeros((0, 3))
    shifts = torch.zeros(n, 3) if shifts is None else torch.as_tensor(shifts, dtype=torch.float32).reshape(-1, 3)
    if factors.shape[0] != n or shifts.shape[0] != n:
      raise ValueError('ColourParams: %d orders, %d factor rows, %d shift rows' % (n, factors.shape[0], shifts.shape[0]))
    if not np.isfinite(factors).all() or (factors < 0).any():
      raise ValueError('ColourParams: factors must be finite and >= 0')
    if not bool(torch.isfinite(shifts).all()):
      raise ValueError('ColourParams: shifts must be finite')
    ops = np.full((n, 3), OP_NONE, dtype=np.int32)
    for i, row in enumerate(order):
      row = [c for c in row if c != OP_NONE]
      if OP_HUE in row:
        raise ValueError('ColourParams: image %d asks for hue, which the reference\'s ColorJitter(0.4, 0.4, 0.4) does not apply' % i)
      if any(c not in (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION) for c in row):
        raise ValueError('ColourParams: image %d has an unknown operation code in %s' % (i, row))
      if len(set(row)) != len(row):
        raise ValueError('ColourParams: image %d repeats an operation: %s' % (i, row))
      ops[i, :len(row)] = row
    coef = np.empty((n, 9), dtype=np.float32)
    coef[:, 0:6:2] = factors.astype(np.float32)
    coef[:, 1:6:2] = (1.0 - factors).astype(np.float32)  # (factors is float64 here)
    coef[:, 6:] = shifts.numpy()
    return torch.from_numpy(ops), torch.from_numpy(coef)

  def copy_from(self, other):
    """Refill the device (and host) tables from another ColourParams of the same n, in place."""
    if not isinstance(other, ColourParams) or other.n != self.n:
      raise ValueError('ColourParams.copy_from: needs ColourParams for %d images' % self.n)
    self.ops_host.copy_(other.ops_host)
    self.coef_host.copy_(other.coef_host)
    self.ops.copy_(other.ops)
    self.coef.copy_(other.coef)
    return self


def _require_params(params, n, device, who):
  if not isinstance(params, ColourParams):
    raise TypeError('%s: augment must be ColourParams (draw_colour_params), got %s' % (who, type(params)))
  if params.n != n:
    raise ValueError('%s: ColourParams for %d images, %d images given' % (who, params.n, n))
  if params.ops.device != device:
    raise ValueError('%s: ColourParams on %s, images on %s' % (who, params.ops.device, device))


def draw_colour_params(n, device, generator=None, brightness=0.4, contrast=0.4, saturation=0.4, alphastd=0.1, share=1):
  """Draw the colour augmentation of n images on the host and upload it: -> ColourParams.

  Per draw, in this order (what torchvision >= 0.8's ColorJitter.get_params / forward and then the reference's Lighting.__call__ consume):
    torch.randperm(4)                                      the order of brightness 0, contrast 1, saturation 2, hue 3; hue is dropped
    torch.empty(1).uniform_(max(0, 1 - v), 1 + v)          once each for brightness, contrast, saturation, in that order; a factor
                                                           given as None draws nothing and disables the operation
    torch.empty(3).normal_(0, alphastd)                    Lighting's alphas; alphastd == 0 draws nothing and gives zero shifts
  and shift = lighting_shift(alpha).  With `generator` the draws come from it, otherwise from torch's global generator.
  share = k gives k consecutive images one draw (2: both images of a pair, 12: a whole Deep360 frame); 1, every image on its own, is
  what the reference's loaders do, which transform image by image.
  torchvision is not a dependency of this package: the draw order above restates its documented behaviour and is not pinned by a run
  of the library."""
  if n < 0 or share < 1:
    raise ValueError('draw_colour_params: n = %r, share = %r' % (n, share))
  ranges = []
  for v in (brightness, contrast, saturation):
    if v is not None and v < 0:
      raise ValueError('draw_colour_params: a jitter value must be None or >= 0')
    ranges.append(None if v is None else (max(0.0, 1.0 - v), 1.0 + v))
  order, factors, shifts = [], [], []
  for _ in range(-(-n // share)):
    perm = torch.randperm(4, generator=generator).tolist()
    f = [1.0 if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator)) for r in ranges]
    alpha = torch.empty(3).normal_(0, alphastd, generator=generator) if alphastd != 0 else torch.zeros(3)
    order.append([c for c in perm if c != OP_HUE and ranges[c] is not None])
    factors.append(f)
    shifts.append(lighting_shift(alpha) if alphastd != 0 else torch.zeros(3))
  rows = [i // share for i in range(n)]
  return ColourParams([order[i] for i in rows], [factors[i] for i in rows], torch.stack([shifts[i] for i in rows]) if n else None, device)


def augment_u8_gpu(images_u8, params, return_means=False):
  """(N, H, W, 3) uint8 device images and ColourParams for N images -> (N, 3, H, W) float32: the reference's
  get_transform_stage1(augment=True) of every image with the draws of `params`, on mode_images_u8_augment (two launches, no host
  synchronisation).  With return_means also the (N,) contrast means the kernel used (0 where an image has no contrast step)."""
  if not torch.is_tensor(images_u8) or images_u8.dim() != 4:
    raise ValueError('augment_u8_gpu: images must be a (N, H, W, 3) uint8 tensor')
  _HF.require_gpu(images_u8)
  _require_params(params, images_u8.shape[0], images_u8.device, 'augment_u8_gpu')
  return _HF.images_u8_augment(images_u8, params.ops, params.coef, return_means=return_means)


def rgb_half_gpu(frames_u8, return_u8=False):
  """(F, 12, H, W, 3) uint8 device frames -> (F, 12, H/2, W/2) float32: panoramas 0, 1, 10, 11 halved as PIL.Image.resize halves them
  and normalised; with return_u8 also the 8-bit halved panoramas (F, 4, H/2, W/2, 3)."""
  _HF.require_u8_frames(frames_u8, 'rgb_half_gpu')
  H, W = frames_u8.shape[2:4]
  tab_w, tab_h = _half_tables(H, W, frames_u8.device)
  return _HF.rgb_half_pil(frames_u8, tab_w, tab_h, _norm_lut(frames_u8.device), return_u8)


# ------------------------------------------------------------------------------------ any working size
def resize_table_rows(n, out):
  """pil_resize_table(n, out) packed as the kernel reads it: (out, 2 + ksize) int32 rows [xmin, count, kk[0 .. ksize - 1]]."""
  xmin, count, kk = preprocess.pil_resize_table(n, out)
  return torch.from_numpy(np.ascontiguousarray(np.concatenate([xmin[:, None], count[:, None], kk], axis=1), dtype=np.int32))


def _axis_table(kind, n, out, device):
  """The device table of one axis, cached per (n, out, device): kind 'pil' -> resize_table_rows, 'nearest' -> nearest_index_table."""
  key = (kind, n, out, str(device))
  with _lock:
    hit = _resize_cache.get(key)
    if hit is None:
      hit = (resize_table_rows(n, out) if kind == 'pil' else torch.from_numpy(preprocess.nearest_index_table(n, out))).to(device)
      _resize_cache[key] = hit
    return hit


def _pil_tables(Hs, Ws, H, W, device):
  """(tab_w, tab_h) of mode_images_u8_resize_pil; None for an axis whose size does not change (Pillow skips that pass)."""
  if max(Hs, H) > _HF.RESIZE_MAX_SCALE * min(Hs, H) or max(Ws, W) > _HF.RESIZE_MAX_SCALE * min(Ws, W):
    raise ValueError('resize: %d x %d -> %d x %d is beyond a factor of %d along an axis' % (Hs, Ws, H, W, _HF.RESIZE_MAX_SCALE))
  return (None if Ws == W else _axis_table('pil', Ws, W, device)), (None if Hs == H else _axis_table('pil', Hs, H, device))


def _device_windows(windows, n, shape, crop, device, who):
  """windows (n, 2) (top, left), on the host (checked against the image, then uploaded: not inside a capture) or already on the device
  (trusted: the kernels move a window inside the image) -> contiguous int32 on the device."""
  if crop is None:
    raise ValueError('%s: windows need crop=(h, w)' % who)
  w = torch.as_tensor(windows)
  if w.dim() != 2 or tuple(w.shape) != (n, 2) or w.dtype not in (torch.int32, torch.int64):
    raise ValueError('%s: windows must be an integer (%d, 2) tensor of (top, left), got %s %s' % (who, n, w.dtype, tuple(w.shape)))
  if not w.is_cuda:
    if n and (int(w.min()) < 0 or int(w[:, 0].max()) > shape[0] - crop[0] or int(w[:, 1].max()) > shape[1] - crop[1]):
      raise ValueError('%s: a %d x %d window lies outside the %d x %d image' % (who, crop[0], crop[1], shape[0], shape[1]))
    w = w.to(torch.int32).to(device)
  return w.to(torch.int32).contiguous()


def draw_crop_windows(n, shape, crop=(CROP_H, CROP_W), generator=None):
  """(n, 2) int32 (top, left) on the host: n training windows of crop = (h, w) -- default the disparity loader's 512 x 256 -- inside a
  shape = (H, W) image, each coordinate uniform over its valid range [0, H - h] / [0, W - w] as the host loader's random.randint is
  (Deep360DatasetDisparity._window).  Per window the top is drawn first, then the left; with `generator` the draws come from it,
  otherwise from torch's global generator."""
  h, w = crop
  H, W = shape
  if n < 0 or not (0 < h <= H and 0 < w <= W):
    raise ValueError('draw_crop_windows: n = %r, a %r x %r window in a %r x %r image' % (n, h, w, H, W))
  u = torch.rand((n, 2), generator=generator, dtype=torch.float64)
  span = torch.tensor([H - h + 1, W - w + 1], dtype=torch.float64)
  return torch.minimum((u * span).floor(), span - 1).to(torch.int32)


def resize_u8_gpu(images_u8, shape, windows=None, crop=None, out=None):
  """(..., Hs, Ws, 3) uint8 device images -> (..., h, w, 3) uint8: every image resized to shape = (H, W) as PIL.Image.resize((W, H))
  resizes it (bicubic, 8 bits per channel, bit for bit; up to a factor of 4 along an axis, either way), on mode_images_u8_resize_pil.
  windows: (n, 2) (top, left) for the n = prod(...) images with crop = (h, w): only that window of every resized image is computed.
  out: a uint8 tensor of the result's shape to write into.  Equal sizes and no window return the input itself.
  Frames stored at another size than the networks' reach ModeMultiView / frames_u8_gpu this way: resize the (F, 12, Hs, Ws, 3) frames first."""
  if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() < 3 or images_u8.shape[-1] != 3:
    raise ValueError('resize_u8_gpu: images must be a (..., H, W, 3) uint8 tensor')
  _HF.require_gpu(images_u8)
  lead, (Hs, Ws) = tuple(images_u8.shape[:-3]), images_u8.shape[-3:-1]
  H, W = shape
  if (Hs, Ws) == (H, W) and windows is None and crop is None:
    return images_u8 if out is None else out.copy_(images_u8)
  flat = images_u8.contiguous().view(-1, Hs, Ws, 3)
  tab_w, tab_h = _pil_tables(Hs, Ws, H, W, flat.device)
  if windows is not None:
    windows = _device_windows(windows, flat.shape[0], (H, W), crop, flat.device, 'resize_u8_gpu')
  hw = (H, W) if crop is None else tuple(crop)
  if out is not None:
    if tuple(out.shape) != lead + hw + (3,) or not out.is_contiguous():
      raise ValueError('resize_u8_gpu: out must be a contiguous %s tensor' % (lead + hw + (3,),))
    out = out.view((-1,) + hw + (3,))
  u8 = _HF.images_u8_resize_pil(flat, (H, W), tab_w, tab_h, windows=windows, crop=crop, out_u8=out)[0]
  return u8.view(lead + hw + (3,))


def _pair_slots(N, device):
  """(2 N,) int32 on the device: image 2 n + s of N pairs -> slot s N + n (the left images first, then the right ones)."""
  key = ('pairs', N, str(device))
  with _lock:
    hit = _dst_cache.get(key)
    if hit is None:
      i = np.arange(2 * N)
      hit = torch.from_numpy(((i & 1) * N + (i >> 1)).astype(np.int32)).to(device)
      _dst_cache[key] = hit
    return hit


def pairs_u8_gpu(pairs_u8, disp=None, shape=(1024, 512), crop=None, windows=None, augment=None):
  """(N, 2, Hs, Ws, 3) uint8 device tensor -- the left and right panorama of N Deep360 pairs at their stored size, each as
  np.asarray(PIL RGB image) lays it out -- and optionally their (N, Hs, Ws) float32 disparity maps -> the host loader's dict of device
  tensors {'leftImg', 'rightImg': (N, 3, h, w) float32, 'dispMap': (N, 1, h, w)} ('dispMap' only with disp): what
  Deep360DatasetDisparity(shape=shape) makes of the pair (reference dataloader/deep360_loader.py:92-109).  shape = (H, W).
  As the loader's _fit, a pair is resized only when its stored WIDTH differs from W: both images as PIL.Image.resize((W, H)), the
  disparity by nearest neighbour times float32(W / Ws).  With equal widths the heights must agree too (ValueError otherwise).
  crop = (h, w) with windows (N, 2) (top, left; draw_crop_windows): the training crop -- the same window of the left image, the right
  image and the disparity of a sample; only the window is computed.  Host windows are checked and uploaded; pass a device tensor
  (refilled in place between replays) to capture the call into a graph.
  augment: ColourParams for the 2 N images (row 2 n: left, row 2 n + 1: right): the resize writes 8-bit images and augment_u8_gpu's
  kernels follow -- the reference's order: resize, crop, then the transform.  Without it the normalisation is a lookup in the resize's
  store.  Bit for bit the host loader's images; two to five launches, no host synchronisation, and nothing is uploaded after the first
  call per size (the tables are cached per (n, out, device))."""
  who = 'pairs_u8_gpu'
  if not torch.is_tensor(pairs_u8) or pairs_u8.dtype != torch.uint8 or pairs_u8.dim() != 5 or pairs_u8.shape[1] != 2 or pairs_u8.shape[4] != 3:
    raise ValueError('%s: pairs must be a (N, 2, H, W, 3) uint8 tensor' % who)
  _HF.require_gpu(pairs_u8, disp)
  N, _, Hs, Ws, _ = pairs_u8.shape
  H, W = shape
  dev = pairs_u8.device
  if Ws == W:
    if Hs != H:
      raise ValueError('%s: pairs stored at %d x %d have the working width but not the working height of %d x %d (the loader resizes '
                       'only when the widths differ)' % (who, Hs, Ws, H, W))
  if disp is not None and (not torch.is_tensor(disp) or tuple(disp.shape) != (N, Hs, Ws) or disp.dtype != torch.float32):
    raise ValueError('%s: disp must be a (%d, %d, %d) float32 tensor' % (who, N, Hs, Ws))
  if (crop is None) != (windows is None):
    raise ValueError('%s: crop=(h, w) and windows (draw_crop_windows) are given together' % who)
  if windows is not None:
    windows = _device_windows(windows, N, (H, W), crop, dev, who)
  hw = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
  tab_w, tab_h = _pil_tables(Hs, Ws, H, W, dev)
  flat = pairs_u8.contiguous().view(2 * N, Hs, Ws, 3)
  if augment is None:
    both = _HF.images_u8_resize_pil(flat, (H, W), tab_w, tab_h, lut=_norm_lut(dev), windows=windows, per_window=2, crop=crop, split=True,
                                    want_u8=False, want_f32=True)[1]
  else:
    _require_params(augment, 2 * N, dev, who)
    u8 = flat if (Ws == W and crop is None) else _HF.images_u8_resize_pil(flat, (H, W), tab_w, tab_h, windows=windows, per_window=2, crop=crop)[0]
    both = torch.empty((2 * N,) + (3,) + hw, dtype=torch.float32, device=dev)
    if N:
      _HF.images_u8_augment(u8, augment.ops, augment.coef, dst=_pair_slots(N, dev), out=both)
  out = {'leftImg': both[:N], 'rightImg': both[N:]}
  if disp is not None:
    if Ws == W and crop is None:
      out['dispMap'] = disp.unsqueeze(1)
    else:
      rows, cols = _axis_table('nearest', Hs, H, dev), _axis_table('nearest', Ws, W, dev)
      ratio = 1.0 if Ws == W else W / Ws
      out['dispMap'] = _HF.disp_resize_nearest(disp.contiguous(), (H, W), rows, cols, ratio, windows=windows, crop=crop).unsqueeze(1)
  return out


def _erp_tables(pairs, H, W, device):
  """(grid (G, H, W, 2), cols (3, W)) on the device for a tuple of pair names: G = 1 when they are all the same.  What is cached is
  one (1, H, W, 2) grid per pair name and the column table; the grids of a mixed batch are concatenated on the device (one copy kernel,
  no upload, capturable), so a loader that draws a pair per item (pair='all') never misses after its three grids are up."""
  from utils import geometry
  from . import dataset3D60Loader as L
  dev = str(device)
  with _lock:
    grids = {}
    for p in sorted(set(pairs)):
      hit = _erp_cache.get((p, H, W, dev))
      if hit is None:
        hit = torch.from_numpy(geometry.erp2rect_grid(geometry.pair_rotation(p), H, W)[None]).to(device)
        _erp_cache[(p, H, W, dev)] = hit
      grids[p] = hit
    cols = _erp_cache.get(('cols', W, dev))
    if cols is None:
      cols = torch.from_numpy(L.disp_cols(W)).to(device)
      _erp_cache[('cols', W, dev)] = cols
  return (grids[pairs[0]] if len(grids) == 1 else torch.cat([grids[p] for p in pairs])), cols


def erp_pairs_gpu(pairs_u8, depth_left=None, depth_right=None, pair='lr', shape=(512, 256), max_depth=20.0, baseline=0.26, flip=True,
                  return_u8=False, augment=None):
  """(N, 2, He, We, 3) uint8 device tensor -- the left and right ERP panorama of N 3D60 samples, each as np.asarray(PIL RGB image) lays
  it out -- and optionally the (N, He, We) float32 ERP depth of the left and of the right view -> the reference loader's dict of device
  tensors: 'leftImg', 'rightImg' (N, 3, H, W), 'dispMap' (N, 1, H, W, NaN where the depth is invalid), and with `flip` the mirrored twin
  'leftImg_flip', 'rightImg_flip', 'dispMap_flip'.  'dispMap' needs depth_left, 'dispMap_flip' depth_right; without them the key is absent.
  pair: 'lr', 'ud', 'ur', or a sequence of N of them (what a batch of Dataset3D60Disparity(device_ingest=True) items carries).  shape:
  the Cassini (H, W).  With return_u8 also 'cassini_u8' (N, 2, H, W, 3), the 8-bit Cassini images.  Two or three launches, no host
  synchronisation; the grids and the column table are cached per (pair, shape, device).
  augment: ColourParams for the 2 N images (row 2 n: left, row 2 n + 1: right) -> 'leftImg' and 'rightImg' are augment_u8_gpu of the
  8-bit Cassini images, and the twin is the mirror of the augmented pair (leftImg_flip = rightImg mirrored, rightImg_flip = leftImg
  mirrored); the disparities are untouched."""
  N = pairs_u8.shape[0] if torch.is_tensor(pairs_u8) and pairs_u8.dim() == 5 else 0
  pairs = (pair,) * max(N, 1) if isinstance(pair, str) else (tuple(pair) or ('lr',))  # (an empty batch still gets a grid of the right shape)
  if N and len(pairs) != N:
    raise ValueError('erp_pairs_gpu: %d pair names for %d samples' % (len(pairs), N))
  H, W = shape
  if W % 4 or H <= 0 or W <= 0:
    raise ValueError('erp_pairs_gpu: Cassini shape %s needs a positive height and a width that is a positive multiple of 4' % (tuple(shape),))
  _HF.require_gpu(pairs_u8)
  grid, cols = _erp_tables(pairs, H, W, pairs_u8.device)
  if augment is None:
    left, right, left_f, right_f, u8 = _HF.erp_pairs_u8_cassini(pairs_u8, grid, _norm_lut(pairs_u8.device), flip, return_u8)
  else:
    _require_params(augment, 2 * N, pairs_u8.device, 'erp_pairs_gpu')
    u8 = _HF.erp_pairs_u8_cassini(pairs_u8, grid, _norm_lut(pairs_u8.device), False, True)[4]
    both = torch.empty((2 * N, 3, H, W), dtype=torch.float32, device=pairs_u8.device)
    if N:
      slots = torch.arange(2 * N, dtype=torch.int32, device=pairs_u8.device)
      slots = (slots & 1) * N + (slots >> 1)  # image 2 n + s -> slot s N + n: the left images first, then the right ones
      _HF.images_u8_augment(u8.view(2 * N, H, W, 3), augment.ops, augment.coef, dst=slots.to(torch.int32), out=both)
    left, right = both[:N], both[N:]
    left_f, right_f = (torch.flip(right, (3,)), torch.flip(left, (3,))) if flip else (None, None)
  out = {'leftImg': left, 'rightImg': right}
  if depth_left is not None:
    out['dispMap'] = _HF.erp_depth_disp(depth_left, grid, cols, baseline, max_depth)
  if flip:
    out['leftImg_flip'], out['rightImg_flip'] = left_f, right_f
    if depth_right is not None:
      out['dispMap_flip'] = _HF.erp_depth_disp(depth_right, grid, cols, baseline, max_depth, mirror=True)
  if return_u8:
    out['cassini_u8'] = u8
  return out
