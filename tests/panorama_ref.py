"""CPU restatement of the ERP-domain scoring for tests/test_gpu_panorama.py and tests/test_panorama_host.py: the input recipe, the
Cassini -> ERP resampling as torch's own F.grid_sample over the project's cached sample points (utils.geometry._c2e_grid), and the eight
depth metrics as plain torch formulas, in whatever dtype the caller asks for (float64: the truth; float32: the yardstick of how far
an fp32 evaluation of the same chain lies from it)."""
import math

import torch
import torch.nn.functional as F

from utils import geometry

MAXDEPTH = 1000.0
NAMES = ('mae', 'rmse', 'absrel', 'sqrel', 'silog', 'delta1', 'delta2', 'delta3')
RATIOS = (1.25, 1.25**2, 1.25**3)


def make_inputs(frames, H, W, seed=2022):
  """(pred, gt) float32 CPU tensors (frames, H, W): a smooth ground truth 2 + 40 (0.5 + 0.5 sin(3 pi i) cos(2 pi j)), i = r / (H - 1),
  j = c / (W - 1), with the top eighth of rows at 5000 ("sky", beyond maxdepth), pred = gt (1 + 0.3 N(0, 1)), and in the last frame a
  small block of pred = -1 (selected, but outside the log terms: N_BOTH < N)."""
  i = torch.arange(H, dtype=torch.float64)[:, None] / (H - 1)
  j = torch.arange(W, dtype=torch.float64)[None, :] / (W - 1)
  field = 2 + 40 * (0.5 + 0.5 * torch.sin(3 * math.pi * i) * torch.cos(2 * math.pi * j))
  field[:H // 8] = 5000
  gt = field.float().expand(frames, H, W).contiguous()
  g = torch.Generator().manual_seed(seed + 7 * H + frames)
  pred = (gt * (1 + 0.3 * torch.randn(frames, H, W, generator=g))).contiguous()
  pred[-1, H // 2:H // 2 + 4, W // 2:W // 2 + 3] = -1
  return pred, gt


def c2e(x, dtype):
  """(F, H, W) Cassini maps -> (F, W, H) ERP panoramas in `dtype` on the CPU (bilinear, border padding, align_corners=True)."""
  Fr, H, W = x.shape
  grid = geometry._c2e_grid(W, H, 'cpu').to(dtype).expand(Fr, W, H, 2)
  return F.grid_sample(x.cpu().to(dtype).unsqueeze(1), grid, mode='bilinear', padding_mode='border', align_corners=True)[:, 0]


def depth_metrics(p, g):
  """The eight metrics of one frame over already selected 1-D p, g, each formed in the tensors' dtype; the three accuracies as
  percentages of the selected count.  Python floats."""
  d = p - g
  pos = g > 0
  both = pos & (p > 0)
  l = torch.log(p[both]) - torch.log(g[both])
  r = torch.maximum(p / g, g / p)
  out = [float(d.abs().mean()), float((d * d).mean().sqrt()), float((d.abs()[pos] / g[pos]).mean()),
         float(((d * d)[pos] / (g * g)[pos]).mean()), float(((l * l).mean() - l.mean()**2).sqrt())]
  return out + [100 * int((r < k).sum()) / p.numel() for k in RATIOS]


def reference_rows(pred, gt, dtype, maxdepth=MAXDEPTH):
  """Per-frame rows of the chain in `dtype` on the CPU, and the ERP maps: (rows list of 8-lists, pred_erp, gt_erp)."""
  pe, ge = c2e(pred, dtype), c2e(gt, dtype)
  rows = []
  for f in range(pe.shape[0]):
    m = ge[f] <= maxdepth
    rows.append(depth_metrics(pe[f][m], ge[f][m]))
  return rows, pe, ge


def ambiguous_counts(pe64, ge64, maxdepth=MAXDEPTH, rel=1e-4):
  """Per frame: (selected count, [per threshold: selected pixels whose float64 ratio lies within `rel` (relative) of it])."""
  out = []
  for f in range(pe64.shape[0]):
    m = ge64[f] <= maxdepth
    p, g = pe64[f][m], ge64[f][m]
    r = torch.maximum(p / g, g / p)
    out.append((int(m.sum()), [int(((r - k).abs() <= rel * k).sum()) for k in RATIOS]))
  return out


def stat_means(s):
  """[mae, rmse, absrel, sqrel, silog] in float64 from one statistic vector of mode_erp_depth_metrics (no rounding to fp32)."""
  import mode_hip as M
  n, ng, nb = s[M.M_N], s[M.M_N_GT], s[M.M_N_BOTH]
  m1, m2 = s[M.M_SUM_LOG] / nb, s[M.M_SUM_LOG2] / nb
  return [s[M.M_SUM_ABS] / n, math.sqrt(s[M.M_SUM_SQ] / n), s[M.M_SUM_ABSREL] / ng, s[M.M_SUM_SQREL] / ng, math.sqrt(m2 - m1 * m1)]
