"""Scoring of fused depth in the equirectangular (ERP) domain, as the reference's test_fusion.py reports it (:76-100): per batch an
optional x2 bicubic upsampling of the fusion output (--resize, :82), cassini2Equirec of prediction and ground truth (:86-87), the
gt <= maxdepth selection (:89) and the eight metrics of utils.evaluation.depth_metrics (:93-100).

Here that is one call for any number of frames: mode_bicubic_up2 where asked, then mode_erp_depth_metrics -- resampling, selection
and the per-frame reductions in one pass, with no ERP tensors written unless asked for, no torch arithmetic and one copy back for the
whole batch.  Row f is what the reference's loop accumulates for frame f at its default batch size of 1, and has the bits of
evaluation.depth_metrics on that frame's cassini2Equirec maps.  GPU tensors only; importing this module loads no native library."""
import numpy as np

import mode_hip
from mode_hip import functional as _F
from mode_hip.functional import bicubic_up2  # noqa: F401  (re-exported: F.interpolate(scale_factor=[2, 2], mode='bicubic', align_corners=True))
from utils import evaluation as _E
from utils import geometry as _G

__all__ = ['erp_depth_metrics', 'bicubic_up2']

_RATIOS = (1.25**1, 1.25**2, 1.25**3)  # delta_acc(1), (2), (3)


def _frames(t, what):
  """(F, H, W) or (F, 1, H, W) -> the (F, H, W) view."""
  if t.dim() == 4 and t.shape[1] == 1:
    return t[:, 0]
  if t.dim() == 3:
    return t
  raise ValueError('erp_depth_metrics: %s of shape %s is not (F, H, W) or (F, 1, H, W)' % (what, tuple(t.shape)))


def _row(s, f):
  """depth_metrics' list from one frame's statistic vector, as the float64 row np.array() makes of it."""
  n = s[mode_hip.M_N]
  if n == 0:
    raise ZeroDivisionError('erp_depth_metrics: frame %d has no pixel with gt <= maxdepth (the reference divides by zero in delta_acc)' % f)
  return [float(v) for v in (_E._mae(s), _E._rmse(s), _E._absrel(s), _E._sqrel(s), _E._silog(s))] + \
         [_E._pct(s[mode_hip.M_RATIO + k], n) for k in range(3)]


def erp_depth_metrics(pred, gt, maxdepth=1000., upsample=False, return_erp=False):
  """pred, gt: (F, H, W) or (F, 1, H, W) float32 device tensors in the Cassini frame (H == 2 W); with upsample=True pred is
  (F, 1, H/2, W/2) and goes through bicubic_up2 first.  Returns an (F, 8) float64 numpy array, row f =
  np.array(evaluation.depth_metrics(pred_erp[f], gt_erp[f], gt_erp[f] <= maxdepth)) = [mae, rmse, absrel, sqrel, silog, delta_acc(1),
  delta_acc(2), delta_acc(3)] of frame f's panorama.  A frame with nothing selected raises ZeroDivisionError, as the reference's
  delta_acc does on that batch.  return_erp: also the (F, W, H) device panoramas, (rows, pred_erp, gt_erp)."""
  p, g = _frames(pred, 'pred'), _frames(gt, 'gt')
  F, H, W = g.shape
  if H != 2 * W or H == 0:
    raise ValueError('erp_depth_metrics: a Cassini frame is H = 2 W, got gt %d x %d' % (H, W))
  want = (F, H // 2, W // 2) if upsample else (F, H, W)
  if upsample and (H % 2 or W % 2):
    raise ValueError('erp_depth_metrics: upsample=True needs even H, W (gt is %d x %d)' % (H, W))
  if tuple(p.shape) != want:
    raise ValueError('erp_depth_metrics: pred %s does not fit gt %s%s: expected %s' %
                     (tuple(pred.shape), tuple(gt.shape), ' with upsample=True' if upsample else '', want))
  mode_hip.require_gpu(p, g)
  if upsample:
    p = bicubic_up2(p.contiguous().unsqueeze(1))[:, 0]
  grid = _G._c2e_grid(W, H, str(g.device))
  out = _F.erp_depth_metrics(p.contiguous(), g.contiguous(), grid, maxdepth, ratio=_RATIOS, return_erp=return_erp)
  stats = (out[0] if return_erp else out).cpu().numpy()  # the one copy back
  rows = np.array([_row(stats[f], f) for f in range(F)], dtype=np.float64).reshape(F, 8)
  return (rows, out[1], out[2]) if return_erp else rows
