"""3D60 dataset of the disparity stage (public surface of the reference's dataloader/dataset3D60Loader.py:56-270: the class name,
constructor arguments, list-file format and returned keys of Dataset3D60Disparity).

3D60 frames are equirectangular (ERP).  Per sample the reference re-projects both RGB panoramas and both depth maps to rectified
Cassini (utils.geometry.erp2rect_cassini on the CPU), truncates the RGB result to bytes and normalises it, and turns the depth into
the disparity ground truth by the sine rule, for the pair and for its mirrored twin.  Here that arithmetic exists twice:

  device_ingest=False   on the host, with torch's CPU grid_sample as the reference itself runs it (the functions below);
  device_ingest=True    the item is the decoded ERP bytes, the ERP depths and the pair name, and the training loop makes one
                        dataloader.gpu_ingest.erp_pairs_gpu call per batch (csrc/erp_ingest.hip), bit-equal for the images.

Written against PIL + numpy.  Depth maps are read by an injectable `depthloader`; the default reads .npy, and .exr through cv2 if cv2
imports.  The two fusion classes of the reference file need stage-1 exports on disk and are not provided.

A list-file line is
  ./path/Left/rgb.png ./path/Right/rgb.png ./path/Up/rgb.png ./path/Left/depth.exr ./path/Right/depth.exr ./path/Up/depth.exr
and every name loses its first two characters and is joined to rootDir/{Center_Left_Down,Right,Up}/ (dataset3D60Loader.py:127-134)."""
import os
import random

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image
from torch.utils.data import Dataset

from utils.geometry import erp2rect_grid, pair_rotation

from . import preprocess

splits = ['training', 'testing', 'validation']
stereo_pairs = ['lr', 'ud', 'ur', 'all']  # left-right, up-down, up-right; 'all' draws one of them per item
# which of (left/down, right, up) plays the left and the right view of a pair (dataset3D60Loader.py:136-153)
_VIEWS = {'lr': (0, 1), 'ud': (2, 0), 'ur': (2, 1)}


# ---- file readers ---------------------------------------------------------------------------------------------------------
def default_loader(path):
  """RGB panorama as an (He, We, 3) uint8 array: np.array(Image.open(path).convert('RGB'))."""
  with Image.open(path) as im:
    return np.array(im.convert('RGB'))


def depth_loader(path):
  """(He, We) float32 depth map: .npy through numpy; anything else (3D60 ships OpenEXR) through cv2.imread(path, IMREAD_ANYDEPTH) as
  the reference reads it -- if cv2 can be imported.  Without cv2 that is an error at first use, not a silent substitute."""
  if path.endswith('.npy'):
    return np.load(path).astype(np.float32)
  try:
    os.environ.setdefault('OPENCV_IO_ENABLE_OPENEXR', '1')
    import cv2
  except ImportError as e:
    raise RuntimeError('depth_loader: reading %s needs cv2 (OpenEXR), which cannot be imported here (%s); convert the depth maps to '
                       '.npy or pass a depthloader to Dataset3D60Disparity' % (path, e))
  d = cv2.imread(path, cv2.IMREAD_ANYDEPTH)
  if d is None:
    raise RuntimeError('depth_loader: cv2 could not read %s' % path)
  return np.array(d).astype(np.float32)


# ---- the reference's host arithmetic ---------------------------------------------------------------------------------------
def erp2rect_host(erp, grid):
  """utils/geometry.py:159-200 on the CPU for a numpy (He, We) or (He, We, C) image and the (H, W, 2) float32 grid of
  utils.geometry.erp2rect_grid: F.grid_sample(bilinear, border, align_corners=True) on the same transposed view of the image, the
  result cast to the image's dtype (uint8: truncation) and squeezed."""
  a = np.asarray(erp)
  if a.ndim == 2:
    a = a[:, :, None]
  src = torch.FloatTensor(a).unsqueeze(0).transpose(1, 3).transpose(2, 3)
  g = torch.from_numpy(np.array(grid, dtype=np.float32)).unsqueeze(0)  # (a copy: the cached grid is read-only)
  out = F.grid_sample(src, g, mode='bilinear', align_corners=True, padding_mode='border')
  return out.transpose(1, 3).transpose(1, 2).numpy()[0].astype(a.dtype).squeeze()


def cassini_phi(width):
  """(width,) float32: the latitude of every Cassini column (__genCassiniPhiMap, :250-256)."""
  return np.arange(0.5 * np.pi - (0.5 * np.pi / width), -0.5 * np.pi, -(np.pi / width)).astype(np.float32)


def disp_cols(width):
  """(3, width) float32, the column table of mode_erp_depth_disp: phi, sin(phi), cos(phi + pi / 2) as numpy rounds them in __depth2disp."""
  phi = cassini_phi(width)
  return np.ascontiguousarray(np.stack((phi, np.sin(phi), np.cos(phi + np.pi / 2))), dtype=np.float32)


def depth2disp(depth, width, baseline=0.26, max_depth=20.0):
  """__depth2disp (:258-270): (H, width) float32 depth -> disparity by the sine rule; NaN where the depth is not in (0, max_depth],
  negative disparities set to 0.  The reference's expression on its masked array, so also its dtype: float32 under numpy 1, float64
  under numpy 2, where the masked array is promoted when it meets the Python scalar `baseline`."""
  depth = np.asarray(depth, dtype=np.float32)
  phi = np.broadcast_to(cassini_phi(width), depth.shape)
  d = np.ma.array(depth, mask=(depth <= 0) | (depth > max_depth))
  ratio = (d * np.sin(phi) + baseline) / np.sqrt(d * d + baseline * baseline - 2 * d * baseline * np.cos(phi + np.pi / 2))
  disp = width * (np.arcsin(np.clip(ratio, -1, 1)) - phi) / np.pi
  disp = disp.filled(np.nan)
  disp[disp < 0] = 0
  return disp


def host_sample(left_u8, right_u8, depth_left, depth_right, pair, shape=(512, 256), max_depth=20.0, baseline=0.26):
  """__getitem__:175-210 for one decoded sample: -> (leftImg, rightImg uint8 (H, W, 3), dispMap (H, W), the three of the mirrored
  twin).  (The reference's cv2.resize to (W, H) is the identity: erp2rect_cassini already returns that size.)"""
  H, W = shape
  grid = erp2rect_grid(pair_rotation(pair), H, W)
  left = erp2rect_host(left_u8, grid).astype(np.uint8)
  right = erp2rect_host(right_u8, grid).astype(np.uint8)
  dl = erp2rect_host(np.asarray(depth_left).astype(np.float32), grid)
  dr = erp2rect_host(np.asarray(depth_right).astype(np.float32), grid)
  left_f, right_f, dr_f = right[:, ::-1].copy(), left[:, ::-1].copy(), dr[:, ::-1].copy()  # cv2.flip(.., 1)
  dl[dl > max_depth] = 0.0
  dr_f[dr_f > max_depth] = 0.0
  return (left, right, depth2disp(dl, W, baseline, max_depth), left_f, right_f, depth2disp(dr_f, W, baseline, max_depth))


class Dataset3D60Disparity(Dataset):
  """One stereo pair per item, the reference's keys: {'leftImg', 'rightImg' (3, H, W), 'dispMap' (1, H, W), 'leftImg_flip',
  'rightImg_flip', 'dispMap_flip', 'leftNames', 'rightNames'}; with crop=True a random (H/2, W/2) window of the first three and
  'leftNames' (:212-230).  As in the reference the `flip` argument is stored and not read: the twin is always returned.

  device_ingest=True returns what the GPU path starts from instead: {'pairs_u8' (2, He, We, 3) uint8, 'depth_left', 'depth_right'
  (He, We) float32, 'pair', 'leftNames', 'rightNames'}; a batch of these goes to dataloader.gpu_ingest.erp_pairs_gpu (pairs_u8,
  depth_left, depth_right, pair=batch['pair'], shape=...).  crop=True stays on the host path."""

  def __init__(self, filenamesFile, rootDir='../../datasets/3D60/', curStage='training', shape=(512, 256), crop=False, pair='lr', flip=False,
               maxDepth=20.0, device_ingest=False, depthloader=depth_loader, rgbloader=default_loader):
    super(Dataset3D60Disparity, self).__init__()
    assert curStage in splits
    assert (rootDir is not None) and (rootDir != '')
    assert pair in stereo_pairs
    if device_ingest and crop:
      raise ValueError('Dataset3D60Disparity: crop=True (a random window per item) is a host-path option; use device_ingest=False')
    self.rootDir, self.curStage = rootDir, curStage
    self.height, self.width = shape
    self.pair, self.crop, self.flip = pair, crop, flip
    self.filenamesFile = filenamesFile
    self.baseline = 0.26  # left-right baseline
    self.maxDepth = maxDepth
    self.device_ingest = device_ingest
    self.depthloader, self.rgbloader = depthloader, rgbloader
    self.prefixes = [os.path.join(rootDir, d) for d in ('Center_Left_Down/', 'Right/', 'Up/')]
    self.processed = preprocess.get_transform_stage1(augment=False)
    with open(filenamesFile) as f:
      self.fileNameList = [line.strip().split(' ') for line in f.readlines()]

  def __len__(self):
    return len(self.fileNameList)

  def _draw_pair(self):
    if self.pair != 'all':
      return self.pair
    ra = random.random()  # the reference's thresholds as written (:156-174): [0, 1/3) lr, [1/2, 2/3) ud, the rest ur
    return 'lr' if ra < 1 / 3 else ('ud' if 1 / 2 <= ra < 2 / 3 else 'ur')

  def __getitem__(self, index):
    assert len(self.fileNameList) > 0
    name = self.fileNameList[index]
    rgb = [os.path.join(self.prefixes[v], name[v][2:]) for v in range(3)]
    depth = [os.path.join(self.prefixes[v], name[3 + v][2:]) for v in range(3)]
    pair = self._draw_pair()
    l, r = _VIEWS[pair]
    left_u8, right_u8 = self.rgbloader(rgb[l]), self.rgbloader(rgb[r])
    depth_l, depth_r = self.depthloader(depth[l]), self.depthloader(depth[r])
    if self.device_ingest:
      return {'pairs_u8': torch.from_numpy(np.stack((left_u8, right_u8))),
              'depth_left': torch.from_numpy(np.ascontiguousarray(depth_l, dtype=np.float32)),
              'depth_right': torch.from_numpy(np.ascontiguousarray(depth_r, dtype=np.float32)),
              'pair': pair, 'leftNames': rgb[l], 'rightNames': rgb[r]}
    left, right, disp, left_f, right_f, disp_f = host_sample(left_u8, right_u8, depth_l, depth_r, pair, (self.height, self.width),
                                                             self.maxDepth, self.baseline)
    if self.crop:
      th, tw = self.height // 2, self.width // 2
      x1, y1 = random.randint(0, self.width - tw), random.randint(0, self.height - th)
      win = (slice(y1, y1 + th), slice(x1, x1 + tw))
      # 'leftNames' is the Left/Down file whatever the pair, as the reference returns it here (:230 `leftName`, not `left` as :245)
      return {'leftImg': self.processed(np.ascontiguousarray(left[win])), 'rightImg': self.processed(np.ascontiguousarray(right[win])),
              'dispMap': torch.from_numpy(np.ascontiguousarray(disp[win])).unsqueeze_(0), 'leftNames': rgb[0]}
    return {'leftImg': self.processed(left), 'rightImg': self.processed(right), 'dispMap': torch.from_numpy(disp).unsqueeze_(0),
            'leftImg_flip': self.processed(left_f), 'rightImg_flip': self.processed(right_f),
            'dispMap_flip': torch.from_numpy(disp_f).unsqueeze_(0), 'leftNames': rgb[l], 'rightNames': rgb[r]}
