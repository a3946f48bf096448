"""Camera rigs for the GPU tests and the hand-written single-call path they are compared with (a helper, not a test)."""
import math

import torch

from mode_hip import check, lib, ptr, stream_of
from utils import geometry as HG
from utils.rig import CameraRig, PairPose

# poses that no table of utils.geometry holds (and so no cached grid of another test)
FREE_ROTATE = PairPose('free_rotate', 0.26, 'rotate', (math.pi / 3, 0.2, -0.1))
FREE_VIEW = PairPose('free_view', 0.26, 'view', (0.3, -0.5, 0.4, 1.0, 0.2, -0.3))


def renamed(p, name):
  return PairPose(name, p.baseline, p.kind, p.pose)


def reversal(rig):
  """The same pairs in the opposite order; the RGB panoramas keep their images."""
  P = len(rig.pairs)
  return CameraRig(reversed(rig.pairs), tuple(2 * (P - 1 - k // 2) + k % 2 for k in rig.rgb), name='reversed')


def mixed16():
  """16 pairs: the six of Deep360 and the two free poses, all kinds interleaved, then the same eight again under other names."""
  d = CameraRig.deep360().pairs
  eight = (d[3], d[0], FREE_ROTATE, d[1], FREE_VIEW, d[4], d[2], d[5])  # view, identity, rotate, rotate, view, view, rotate, view
  return CameraRig(eight + tuple(renamed(p, p.name + 'b') for p in eight), (0, 3, 30), name='mixed16')


def rigs():
  d = CameraRig.deep360()
  out = {'deep360': d, 'reversed': reversal(d), 'subset': d.subset(('12', '13', '23'))}
  for p in (d.pairs[0], d.pairs[2], d.pairs[4]):
    out['one_' + p.kind] = CameraRig([p], (0,))
  out['rotate_only'] = CameraRig([d.pairs[2], FREE_ROTATE, d.pairs[1]], (0, 5))                   # V = 0: no workspace
  out['view_only'] = CameraRig([d.pairs[5], FREE_VIEW, d.pairs[3], d.pairs[4]], (1,))              # R = 0: no grids
  out['mixed16'] = mixed16()
  out['free'] = CameraRig([FREE_ROTATE, FREE_VIEW], (0, 1, 2))
  return out


def inputs(F, P, H, W, seed, device):
  """As tests/test_gpu_multiview._inputs draws them, for P pairs: zeros, near-zero values (depth far beyond the 1000 clip) and values up
  to a quarter of the width; a confidence beside them."""
  g = torch.Generator().manual_seed(seed)
  disp = torch.rand(F, P, H, W, generator=g) * (W / 4)
  u = torch.rand(F, P, H, W, generator=g)
  disp[u < 0.1] = 0
  tiny = (u >= 0.1) & (u < 0.2)
  disp[tiny] = torch.rand(int(tiny.sum()), generator=g) * 1e-2
  conf = torch.rand(F, P, H, W, generator=g)
  return disp.to(device), conf.to(device)


def sine_rule_call(disp, pair):
  """mode_disp2depth of one (H, W) map with the pair's baseline: the depth in the pair's own view, before any resampling."""
  disp = disp.contiguous()
  H, W = disp.shape
  depth = torch.empty_like(disp)
  with torch.cuda.device_of(disp):
    check(lib().mode_disp2depth(ptr(disp), ptr(depth), H, W, float(pair.baseline), stream_of(disp)), 'mode_disp2depth')
  return depth


def pair_call(disp, conf, pair):
  """One (H, W) map through the single-map entries: mode_disp2depth, then rotateCassini_gpu / depthViewTransWithConf_gpu by kind."""
  conf = conf.contiguous()
  depth = sine_rule_call(disp, pair)
  if pair.kind == 'identity':
    return depth, conf
  if pair.kind == 'rotate':
    both = HG.rotateCassini_gpu(torch.stack((depth, conf)).unsqueeze(0), *pair.pose)[0]
    return both[0], both[1]
  return HG.depthViewTransWithConf_gpu(depth, conf, *pair.pose)


def single_calls(disp, conf, rig, conf_png=False):
  """The loop of tests/test_gpu_multiview._six_calls for a rig: P single calls per frame and ModeFusion's interleave -> (F, 2P, H, W)."""
  frames = []
  for f in range(disp.shape[0]):
    chans = []
    for p, pair in enumerate(rig.pairs):
      d, c = pair_call(disp[f, p], conf[f, p], pair)
      if conf_png:
        c = torch.from_numpy(HG.conf_png_np(c.cpu().numpy())).to(disp.device)
      chans += [d, c]
    frames.append(torch.stack(chans))
  return torch.stack(frames)
