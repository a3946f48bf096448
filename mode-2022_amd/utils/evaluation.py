"""Evaluation metrics of the reference (utils/evaluation.py): the same ten functions with the same names, parameters and result types,
each one pass of the HIP reduction mode_masked_metrics (csrc/metrics.hip) plus one small copy back -- no boolean-mask compaction,
no elementwise torch launches.  Two fused entries, disparity_metrics and depth_metrics, give the per-batch lists of the reference's
scripts (test_disparity.py:137-143, train_fusion.py:139-147, test_fusion.py:93-100) with the mask applied in the kernel.

Semantics are the reference's on CPU torch: per-element terms in fp32 as torch forms them, thresholds rounded to fp32, NaN fails every
threshold but counts in numel; sums in fp64 rounded to fp32 once.  Mean-type results are 0-d float32 numpy arrays (`.cpu().numpy()`),
percentages Python floats; empty input gives NaN means, a RuntimeError from max_ae and a ZeroDivisionError from the percentages.
GPU tensors only (NotImplementedError otherwise, as everywhere in mode_hip).  Importing this module loads no native library."""
import numpy as np

import mode_hip
from mode_hip import functional as _F

__all__ = ['mae', 'max_ae', 'rmse', 'absrel', 'sqrel', 'silog', 'pixel_error_pct', 'D1', 'delta_acc', 'threshold_acc',
           'disparity_metrics', 'depth_metrics']


def _stats(pred, gt, mask=None, px=(), d1=(), ratio=()):
  if pred.shape != gt.shape and mask is None:
    raise ValueError('pred %s and gt %s must have the same shape' % (tuple(pred.shape), tuple(gt.shape)))
  return _F.masked_metrics(pred, gt, mask, px=px, d1=d1, ratio=ratio)


def _f32(x):
  return np.array(x, dtype=np.float32)


def _mean(s, i, n_index):
  n = s[n_index]
  return np.float64(np.nan) if n == 0 else np.float64(s[i]) / n


def _pct(count, n):
  # the reference's 100 * numel(selected) / numel(error) on Python ints: a ZeroDivisionError for no element
  return 100 * int(count) / int(n)


def _mae(s):
  return _f32(_mean(s, mode_hip.M_SUM_ABS, mode_hip.M_N))


def _rmse(s):
  return _f32(np.sqrt(_mean(s, mode_hip.M_SUM_SQ, mode_hip.M_N)))


def _absrel(s):
  return _f32(_mean(s, mode_hip.M_SUM_ABSREL, mode_hip.M_N_GT))


def _sqrel(s):
  return _f32(_mean(s, mode_hip.M_SUM_SQREL, mode_hip.M_N_GT))


def _silog(s):
  m1, m2 = _mean(s, mode_hip.M_SUM_LOG, mode_hip.M_N_BOTH), _mean(s, mode_hip.M_SUM_LOG2, mode_hip.M_N_BOTH)
  with np.errstate(invalid='ignore'):
    return _f32(np.sqrt(m2 - m1 * m1))


def mae(pred, gt):
  return _mae(_stats(pred, gt))


def max_ae(pred, gt):
  s = _stats(pred, gt)
  if s[mode_hip.M_N] == 0:
    raise RuntimeError('max(): Expected reduction dim to be specified for input.numel() == 0. Specify the reduction dim with the '
                       "'dim' argument.")
  return _f32(s[mode_hip.M_MAX_ABS])


def rmse(pred, gt):
  return _rmse(_stats(pred, gt))


def absrel(pred, gt):
  return _absrel(_stats(pred, gt))


def sqrel(pred, gt):
  return _sqrel(_stats(pred, gt))


def silog(pred, gt):
  # sqrt of the silog (following KITTI)
  return _silog(_stats(pred, gt))


def pixel_error_pct(th_pixel, pred, gt):
  s = _stats(pred, gt, px=(th_pixel,))
  return _pct(s[mode_hip.M_PX], s[mode_hip.M_N])


def D1(th_pixel, th_pct, pred, gt):
  s = _stats(pred, gt, d1=((th_pixel, th_pct),))
  return _pct(s[mode_hip.M_D1], s[mode_hip.M_N])


def delta_acc(exp, pred, gt):
  s = _stats(pred, gt, ratio=(1.25**exp,))
  return _pct(s[mode_hip.M_RATIO], s[mode_hip.M_N])


def threshold_acc(err_pct, pred, gt):
  s = _stats(pred, gt, ratio=(1 + err_pct,))
  return _pct(s[mode_hip.M_RATIO], s[mode_hip.M_N])


def disparity_metrics(pred, gt, mask):
  """[MAE, RMSE, Px1, Px3, Px5, D1(3, 0.05)] of pred[mask], gt[mask] (test_disparity.py:137-143) in one pass and one copy; pred, gt
  and mask of equal element count ((B, 1, H, W) with (B, H, W) is fine)."""
  s = _stats(pred, gt, mask, px=(1, 3, 5), d1=((3, 0.05),))
  n = s[mode_hip.M_N]
  return [_mae(s), _rmse(s)] + [_pct(s[mode_hip.M_PX + k], n) for k in range(3)] + [_pct(s[mode_hip.M_D1], n)]


def depth_metrics(pred, gt, mask):
  """[mae, rmse, absrel, sqrel, silog, delta_acc(1), delta_acc(2), delta_acc(3)] of pred[mask], gt[mask] (train_fusion.py:139-147,
  test_fusion.py:93-100) in one pass and one copy; shapes as disparity_metrics."""
  s = _stats(pred, gt, mask, ratio=(1.25**1, 1.25**2, 1.25**3))
  n = s[mode_hip.M_N]
  return [_mae(s), _rmse(s), _absrel(s), _sqrel(s), _silog(s)] + [_pct(s[mode_hip.M_RATIO + k], n) for k in range(3)]
