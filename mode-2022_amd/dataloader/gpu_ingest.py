"""8-bit frames on the GPU: the host half of the reference's loaders between the decoded PNGs and the two networks, as HIP kernels.

  frames_u8_gpu   preprocess.get_transform_stage1(augment=False) of every panorama of (F, 12, H, W, 3) uint8 frames and
                  models.mode_multiview.split_frames of the result, in one launch (mode_frames_u8_ingest)
  rgb_half_gpu    Deep360DatasetFusion(resize=True)'s RGB branch (reference dataloader/deep360_loader.py:151-153, 161-163):
                  PIL.Image.resize((w / 2, h / 2)) of the four fusion panoramas, then the same transform (mode_rgb_half_pil)

Both are bit for bit what the host computes: the normalisation is a lookup in the table the host transform produces for the 256 byte
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
