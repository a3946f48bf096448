"""Host references of the 8-bit ingest (tests/test_ingest_host.py, tests/test_gpu_ingest.py, tests/test_gpu_guard_bands_ingest.py):
numpy restatements driven by the product's own table builders, the Pillow / host-transform truths they are compared with, and the
seeded images.  Nothing here touches the GPU."""
import numpy as np
import torch
from PIL import Image

from dataloader import preprocess
from models.mode_multiview import FUSION_RGB, split_frames


def images(h, w, seed):
  """{'random', 'smooth', 'binary'}: (h, w, 3) uint8 -- seeded noise, a smooth pattern, and a random 0 / 255 image (4 x 4 blocks, shifted
  by one pixel: edges at every phase of the stride-2 taps) whose bicubic overshoot exercises the clip at both ends."""
  rng = np.random.RandomState(seed)
  y, x = np.mgrid[0:h, 0:w].astype(np.float64)
  smooth = np.stack([127.5 + 127.5 * np.sin(0.37 * x + 0.11 * y + c) * np.cos(0.05 * x - 0.23 * y) for c in range(3)], -1)
  return {'random': rng.randint(0, 256, (h, w, 3)).astype(np.uint8), 'smooth': np.rint(smooth).astype(np.uint8),
          'binary': (np.kron(rng.randint(0, 2, (h // 4 + 1, w // 4 + 1, 3)), np.ones((4, 4, 1), dtype=np.int64))[1:h + 1, 1:w + 1] * 255).astype(np.uint8)}


def frames_u8(F, H, W, seed, kind='random'):
  """(F, 12, H, W, 3) uint8 frames of images(...)[kind]; 'random' frames hold every byte value in every channel (asserted)."""
  a = np.stack([np.stack([images(H, W, seed + 100 * f + k)[kind] for k in range(12)]) for f in range(F)])
  if kind == 'random':
    flat = a.reshape(-1, 3)
    flat[:256] = np.arange(256, dtype=np.uint8)[:, None]  # the first 256 pixels of frame 0, panorama 0: a ramp in every channel
    assert all(len(np.unique(a[..., c])) == 256 for c in range(3))
  return a


def pil_half(a):
  """Pillow's own result: (h, w, 3) uint8 -> (h / 2, w / 2, 3)."""
  h, w = a.shape[:2]
  return np.asarray(Image.fromarray(a).resize((w // 2, h // 2)))


def _pass(a, n, axis, clipped):
  """One pass of Resample.c along `axis` of an int64 array of byte values, from pil_half_table(n).  clipped: [below 0, above 255] counts."""
  xmin, count, kk = preprocess.pil_half_table(n)
  a = np.moveaxis(a, axis, 0)
  out = np.empty((n // 2,) + a.shape[1:], dtype=np.int64)
  for i in range(n // 2):
    acc = np.full(a.shape[1:], 1 << (preprocess.PIL_PRECISION_BITS - 1), dtype=np.int64)
    for j in range(count[i]):
      acc += a[xmin[i] + j] * int(kk[i, j])
    assert np.abs(acc).max() < 2 ** 31  # 32-bit accumulation is enough
    v = acc >> preprocess.PIL_PRECISION_BITS
    clipped[0] += int((v < 0).sum())
    clipped[1] += int((v > 255).sum())
    out[i] = np.clip(v, 0, 255)
  return np.moveaxis(out, 0, axis)


def pil_half_numpy(a, clipped=None):
  """The two-pass integer restatement: horizontal pass, its 8-bit result, vertical pass.  clipped: a [0, 0] list that receives how many
  sums of either pass fell below 0 / above 255."""
  h, w = a.shape[:2]
  clipped = [0, 0] if clipped is None else clipped
  return _pass(_pass(a.astype(np.int64), w, 1, clipped), h, 0, clipped).astype(np.uint8)


def host_norm(a):
  """get_transform_stage1(augment=False) of one (h, w, 3) uint8 image -> (3, h, w) float32."""
  return preprocess.get_transform_stage1(augment=False)(a)


def host_frames(frames):
  """(F, 12, H, W, 3) uint8 -> (F, 12, 3, H, W) float32: the host transform of every panorama."""
  return torch.stack([torch.stack([host_norm(p) for p in f]) for f in frames])


def host_split(frames):
  """What the float path starts from: split_frames of the host-normalised panoramas."""
  return split_frames(host_frames(frames))


def ingest_numpy(frames, lut):
  """A stand-in of mode_frames_u8_ingest: lookups in the (256, 3) table and the kernel's index arithmetic."""
  F, _, H, W, _ = frames.shape
  lut = lut.numpy()
  planar = np.stack([lut[frames[..., c], c] for c in range(3)], 2)  # (F, 12, 3, H, W)
  left = np.empty((6 * F, 3, H, W), dtype=np.float32)
  right = np.empty((6 * F, 3, H, W), dtype=np.float32)
  rgb = np.empty((F, 12, H, W), dtype=np.float32)
  for f in range(F):
    for k in range(12):
      (right if k & 1 else left)[6 * f + k // 2] = planar[f, k]
      if k < 2 or k >= 10:
        slot = k if k < 2 else k - 8
        rgb[f, 3 * slot:3 * slot + 3] = planar[f, k]
  return torch.from_numpy(left), torch.from_numpy(right), torch.from_numpy(rgb)


def host_rgb_half(frames):
  """Deep360DatasetFusion(resize=True)'s RGB branch on the host: -> (u8 (F, 4, H/2, W/2, 3), rgb_half (F, 12, H/2, W/2) float32)."""
  u8 = np.stack([np.stack([pil_half(f[k]) for k in FUSION_RGB]) for f in frames])
  rgb = torch.stack([torch.cat([host_norm(p) for p in f]) for f in u8])
  return torch.from_numpy(u8.copy()), rgb
