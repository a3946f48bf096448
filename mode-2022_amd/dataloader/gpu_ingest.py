"""8-bit frames on the GPU: the host half of the reference's loaders between the decoded PNGs and the two networks, as HIP kernels.

  frames_u8_gpu   preprocess.get_transform_stage1(augment=False) of every panorama of (F, 12, H, W, 3) uint8 frames and
                  models.mode_multiview.split_frames of the result, in one launch (mode_frames_u8_ingest)
  rgb_half_gpu    Deep360DatasetFusion(resize=True)'s RGB branch (reference dataloader/deep360_loader.py:151-153, 161-163):
                  PIL.Image.resize((w / 2, h / 2)) of the four fusion panoramas, then the same transform (mode_rgb_half_pil)
  erp_pairs_gpu   Dataset3D60Disparity.__getitem__ (reference dataloader/dataset3D60Loader.py:175-248) for a batch of decoded 3D60
                  samples: both ERP panoramas and both ERP depth maps re-projected to rectified Cassini, the images truncated to bytes
                  and normalised, the depth turned into the disparity ground truth, for the pair and its mirrored twin
                  (mode_erp_pairs_u8_cassini, mode_erp_depth_disp)

The first two are bit for bit what the host computes, and so are the images of the third (its disparities differ from numpy's by the
last bits of asin): the normalisation is a lookup in the table the host transform produces for the 256 byte
values (preprocess.norm_table), the resize Pillow's own fixed-point arithmetic on the coefficients of preprocess.pil_half_table.
Tables are built and uploaded once per device / per (H, W, device) and cached, so the calls can be captured into a graph after a
first eager call.  Importing this module does not load the native library; there is no CPU path."""
import threading

import numpy as np
import torch

from mode_hip import functional as _HF

from . import preprocess

_lut_cache = _HF._LRU(8)    # device -> (256, 3) float32 normalisation table (graph-pinned while captured)
_half_cache = _HF._LRU(8)   # (H, W, device) -> (tab_w (W/2, 10), tab_h (H/2, 10)) int32 tables of mode_rgb_half_pil
_erp_cache = _HF._LRU(16)   # (pair, H, W, device) -> grid (1, H, W, 2); ('cols', W, device) -> cols (3, W): the 3D60 ingest's tables
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


def frames_u8_gpu(frames_u8, want_rgb=True):
  """(F, 12, H, W, 3) uint8 device frames -- the 12 panoramas of a frame in sorted file order, each as np.asarray(PIL image) lays
  it out -> (left (6F, 3, H, W), right (6F, 3, H, W), rgb (F, 12, H, W) or None): split_frames of the ImageNet-normalised panoramas."""
  _HF.require_u8_frames(frames_u8, 'frames_u8_gpu')
  return _HF.frames_u8_ingest(frames_u8, _norm_lut(frames_u8.device), want_rgb)


def rgb_half_gpu(frames_u8, return_u8=False):
  """(F, 12, H, W, 3) uint8 device frames -> (F, 12, H/2, W/2) float32: panoramas 0, 1, 10, 11 halved as PIL.Image.resize halves them
  and normalised; with return_u8 also the 8-bit halved panoramas (F, 4, H/2, W/2, 3)."""
  _HF.require_u8_frames(frames_u8, 'rgb_half_gpu')
  H, W = frames_u8.shape[2:4]
  tab_w, tab_h = _half_tables(H, W, frames_u8.device)
  return _HF.rgb_half_pil(frames_u8, tab_w, tab_h, _norm_lut(frames_u8.device), return_u8)


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
                  return_u8=False):
  """(N, 2, He, We, 3) uint8 device tensor -- the left and right ERP panorama of N 3D60 samples, each as np.asarray(PIL RGB image) lays
  it out -- and optionally the (N, He, We) float32 ERP depth of the left and of the right view -> the reference loader's dict of device
  tensors: 'leftImg', 'rightImg' (N, 3, H, W), 'dispMap' (N, 1, H, W, NaN where the depth is invalid), and with `flip` the mirrored twin
  'leftImg_flip', 'rightImg_flip', 'dispMap_flip'.  'dispMap' needs depth_left, 'dispMap_flip' depth_right; without them the key is absent.
  pair: 'lr', 'ud', 'ur', or a sequence of N of them (what a batch of Dataset3D60Disparity(device_ingest=True) items carries).  shape:
  the Cassini (H, W).  With return_u8 also 'cassini_u8' (N, 2, H, W, 3), the 8-bit Cassini images.  Two or three launches, no host
  synchronisation; the grids and the column table are cached per (pair, shape, device)."""
  N = pairs_u8.shape[0] if torch.is_tensor(pairs_u8) and pairs_u8.dim() == 5 else 0
  pairs = (pair,) * max(N, 1) if isinstance(pair, str) else (tuple(pair) or ('lr',))  # (an empty batch still gets a grid of the right shape)
  if N and len(pairs) != N:
    raise ValueError('erp_pairs_gpu: %d pair names for %d samples' % (len(pairs), N))
  H, W = shape
  if W % 4 or H <= 0 or W <= 0:
    raise ValueError('erp_pairs_gpu: Cassini shape %s needs a positive height and a width that is a positive multiple of 4' % (tuple(shape),))
  _HF.require_gpu(pairs_u8)
  grid, cols = _erp_tables(pairs, H, W, pairs_u8.device)
  left, right, left_f, right_f, u8 = _HF.erp_pairs_u8_cassini(pairs_u8, grid, _norm_lut(pairs_u8.device), flip, return_u8)
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
