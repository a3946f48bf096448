#!/usr/bin/env python3
"""Micro-benchmark of the evaluation metrics and the SILog loss at train_fusion.py's validation batch (8 x 1024 x 512).

  python tools/metrics_bench.py [--iters 50] [--warmup 10] [--out FILE]

  * metrics: train_fusion.py:139-147 (`val`) as the reference writes it -- eight utils/evaluation.py expressions on pred[mask], gt[mask],
    each with its compaction and its `.cpu()` -- against utils.evaluation.depth_metrics (one mode_masked_metrics pass, one copy);
  * loss: train_fusion.py:82-87 on output[mask], gt[mask] as torch ops, forward + backward, against mode_hip.functional.silog_loss.
Every timed call ends in a device synchronise (the metric lists end in one by construction); the two sides alternate round by round
and the median per call is reported.  Prints one JSON line (also written to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def torch_val_metrics(pred, gt, mask):
  """train_fusion.py:139-147 as torch runs it: each of the eight metrics compacts pred[mask], gt[mask] itself, reduces, and copies its
  result to the host."""
  out = []
  p, g = pred[mask], gt[mask]
  out.append((p - g).abs().mean().cpu().numpy())
  p, g = pred[mask], gt[mask]
  out.append((p - g).square().mean().sqrt().cpu().numpy())
  p, g = pred[mask], gt[mask]
  pos = g > 0
  out.append(((p[pos] - g[pos]).abs() / g[pos]).mean().cpu().numpy())
  p, g = pred[mask], gt[mask]
  pos = g > 0
  out.append(((p[pos] - g[pos]).square() / g[pos].square()).mean().cpu().numpy())
  p, g = pred[mask], gt[mask]
  both = (g > 0) * (p > 0)
  d = p[both].log() - g[both].log()
  out.append((d.square().mean() - d.mean().square()).sqrt().cpu().numpy())
  for k in (1, 2, 3):
    p, g = pred[mask], gt[mask]
    ratio = torch.max(p / g, g / p)
    out.append(100 * ratio[ratio < 1.25**k].numel() / ratio.numel())
  return out


def torch_silog_step(pred, gt, mask):
  p, g = torch.squeeze(pred, 1)[mask], gt[mask]
  sel = (g > 0) * (p > 0)
  d = torch.log(p[sel]) - torch.log(g[sel])
  loss = torch.mean(torch.square(d)) - 0.5 * torch.square(torch.mean(d))
  gp, = torch.autograd.grad(loss, pred)
  return loss, gp


def ours_silog_step(pred, gt, mask):
  from mode_hip import functional as HF
  loss = HF.silog_loss(pred, gt, mask)
  gp, = torch.autograd.grad(loss, pred)
  return loss, gp


def timed(fn, *args):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  r = fn(*args)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3, r


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'metrics_bench needs a GPU'
  from utils import evaluation as E
  dev = torch.device('cuda:0')
  B, H, W, maxdepth = 8, 1024, 512, 1000.0
  g = torch.Generator(device='cpu').manual_seed(0)
  gt = (torch.rand(B, H, W, generator=g) * maxdepth * 1.05).to(dev)  # ~5 % above maxdepth: masked out
  pred = (gt.cpu().unsqueeze(1) * (1 + 0.1 * torch.randn(B, 1, H, W, generator=g))).to(dev)
  mask = gt <= maxdepth
  predg = pred.clone().requires_grad_()

  sides = {'metrics_torch': lambda: torch_val_metrics(pred.squeeze(1), gt, mask), 'metrics_ours': lambda: E.depth_metrics(pred, gt, mask),
           'silog_torch': lambda: torch_silog_step(predg, gt, mask), 'silog_ours': lambda: ours_silog_step(predg, gt, mask)}
  for _ in range(args.warmup):
    for f in sides.values():
      timed(f)
  times = {k: [] for k in sides}
  for _ in range(args.iters):
    for k, f in sides.items():
      times[k].append(timed(f)[0])

  # the two sides compute the same numbers (counts exactly, means to fp32 rounding, the loss gradient to fp32 rounding)
  a, b = sides['metrics_torch'](), sides['metrics_ours']()
  counts_equal = all(float(x) == float(y) for x, y in zip(a[5:], b[5:]))
  mean_rel = max(abs(float(x) - float(y)) / max(abs(float(x)), 1e-30) for x, y in zip(a[:5], b[:5]))
  (lt, gt_), (lo, go) = sides['silog_torch'](), sides['silog_ours']()
  lt, lo = float(lt.detach()), float(lo.detach())
  loss_rel = abs(lt - lo) / abs(lt)
  grad_rel = float((gt_ - go).double().norm() / gt_.double().norm())

  med = {k: float(np.median(v)) for k, v in times.items()}
  res = {'tool': 'metrics_bench', 'shape': [B, 1, H, W], 'iters': args.iters, 'device': torch.cuda.get_device_name(0),
         'metrics_torch_ms': round(med['metrics_torch'], 4), 'metrics_ours_ms': round(med['metrics_ours'], 4),
         'metrics_speedup': round(med['metrics_torch'] / med['metrics_ours'], 2),
         'silog_fwd_bwd_torch_ms': round(med['silog_torch'], 4), 'silog_fwd_bwd_ours_ms': round(med['silog_ours'], 4),
         'silog_speedup': round(med['silog_torch'] / med['silog_ours'], 2),
         'counts_equal': counts_equal, 'means_max_rel_diff': mean_rel, 'loss_rel_diff': loss_rel, 'grad_rel_l2_diff': grad_rel}
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
