#!/usr/bin/env python3
"""A/B of the self-supervised stereo loss on one MI355X, in one process: the loss composed from torch operators in fp32 on
the GPU (A; the only way a user has without HF.photometric_loss: elementwise, roll, gather and reduction launches, autograd's scatter in
the backward) against HF.photometric_loss (B; csrc/photometric.hip), forward + backward, at 1024 x 512 with K = 3 maps, B = 2 and B = 12.

    python tools/photometric_bench.py [--windows 4] [--min-window 0.3] [--out FILE.json]

The composition below is written from the definition in include/mode_hip.h.  First the two sides' outputs are compared (loss, and the
gradient relative to its largest element); then windows alternate A B A B ..., each at least --min-window seconds of device time between
two events.  Acceptance: every B window faster than every A window.  For B also the algorithmic bytes -- per pixel and map 7 floats read
(3 left, 3 right, 1 disparity) in each pass and 1 written in the backward, 60 B -- over its device time: an effective rate (the images
are re-read per map and the halo from cache, so it is not a share of the HBM peak)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

WEIGHTS = (0.5, 0.7, 1.0)


def composed_loss(torch, left, right, disps, weights, alpha=0.85, lam=0.1, beta=1.0, C1=1e-4, C2=9e-4):
  from dataloader.preprocess import imagenet_stats
  mean = torch.tensor(imagenet_stats['mean'], device=left.device).view(1, 3, 1, 1)
  std = torch.tensor(imagenet_stats['std'], device=left.device).view(1, 3, 1, 1)
  L, R = left * std + mean, right * std + mean
  B, _, H, W = L.shape

  def box(t):  # mean over the 3x3 window, rows wrapped, columns 1 .. W - 2
    rows = t + torch.roll(t, 1, -2) + torch.roll(t, -1, -2)
    return (rows[..., :-2] + rows[..., 1:-1] + rows[..., 2:]) / 9

  def members(t):
    return [torch.roll(t, -dy, -2)[..., 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]

  ex = torch.exp(-beta * (L[..., 1:] - L[..., :-1]).abs().mean(1))
  ey = torch.exp(-beta * (torch.roll(L, -1, -2) - L).abs().mean(1))
  mx = box(L)
  xs = [m - mx for m in members(L)]
  vx = sum(a * a for a in xs) / 9
  wcol = torch.arange(W, dtype=torch.float32, device=left.device).view(1, 1, W)
  loss = 0
  for d, wgt in zip(disps, weights):
    d = d.reshape(B, H, W)
    x = wcol - d
    valid = torch.isfinite(d) & (x >= 0) & (x <= W - 1)
    xv = torch.where(valid, x, torch.zeros_like(x))
    x0 = xv.detach().floor().clamp(max=W - 2)
    t = (xv - x0).unsqueeze(1)
    i0 = x0.long().unsqueeze(1).expand(B, 3, H, W)
    Rh = (1 - t) * R.gather(3, i0) + t * R.gather(3, i0 + 1)
    Rh = torch.where(valid.unsqueeze(1), Rh, torch.zeros_like(Rh))
    wvalid = torch.stack(members(valid)).all(0)
    my = box(Rh)
    ys = [m - my for m in members(Rh)]
    vy = sum(b * b for b in ys) / 9
    cxy = sum(a * b for a, b in zip(xs, ys)) / 9
    ssim = (2 * mx * my + C1) * (2 * cxy + C2) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    pe = (alpha * (1 - ssim) / 2 + (1 - alpha) * (L - Rh).abs()[..., 1:-1]).mean(1)
    photo = torch.where(wvalid, pe, torch.zeros_like(pe)).sum() / wvalid.sum().clamp(min=1)
    dn = d / W
    smooth = ((dn[..., 1:] - dn[..., :-1]).abs() * ex).mean() + ((torch.roll(dn, -1, -2) - dn).abs() * ey).mean()
    loss = loss + wgt * (photo + lam * smooth)
  return loss


def inputs(torch, B, H, W, K, dev, seed):
  """Low-passed noise images, the right one half independent, and K disparity maps of smooth fields plus noise in [-2, 48)."""
  g = torch.Generator(device=dev).manual_seed(seed)
  from dataloader.preprocess import imagenet_stats
  mean = torch.tensor(imagenet_stats['mean'], device=dev).view(1, 3, 1, 1)
  std = torch.tensor(imagenet_stats['std'], device=dev).view(1, 3, 1, 1)

  def lowpass(u):
    return (u + torch.roll(u, 1, -1) + torch.roll(u, 1, -2)) / 3

  base = lowpass(torch.rand(B, 3, H, W, generator=g, device=dev))
  other = lowpass(torch.rand(B, 3, H, W, generator=g, device=dev))
  left, right = (base - mean) / std, (0.5 * base + 0.5 * other - mean) / std
  hh = torch.linspace(0, 2 * math.pi, H, device=dev).view(1, H, 1)
  ww = torch.linspace(0, math.pi, W, device=dev).view(1, 1, W)
  disps = []
  for k in range(K):
    field = 23 + 20 * torch.sin(hh + k) * torch.sin(ww)
    d = torch.floor(field + 5 * torch.rand(B, H, W, generator=g, device=dev)) + 0.05 + 0.9 * torch.rand(B, H, W, generator=g, device=dev)
    disps.append(d.contiguous())
  return left.contiguous(), right.contiguous(), disps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--windows', type=int, default=4, help='windows per side and batch size')
  ap.add_argument('--min-window', type=float, default=0.3, help='seconds of device time per window, at least')
  ap.add_argument('--batches', type=int, nargs='+', default=[2, 12])
  ap.add_argument('--out', help='also write the result line to this file')
  args = ap.parse_args()

  import torch
  from mode_hip import functional as HF
  assert torch.cuda.is_available(), 'photometric_bench needs a GPU'
  dev = torch.device('cuda:0')
  H, W, K = 1024, 512, 3
  out = {'tool': 'photometric_bench', 'H': H, 'W': W, 'K': K, 'min_window_s': args.min_window, 'windows': args.windows, 'batch': {}}
  ok = True
  for B in args.batches:
    left, right, disps = inputs(torch, B, H, W, K, dev, 100 + B)

    def step(side):
      ds = [d.detach().requires_grad_(True) for d in disps]
      if side == 'A':
        loss = composed_loss(torch, left, right, ds, WEIGHTS)
      else:
        loss = HF.photometric_loss(left, right, ds, WEIGHTS)
      loss.backward()
      return loss.detach(), [d.grad for d in ds]

    la, ga = step('A')
    lb, gb = step('B')
    torch.cuda.synchronize()
    row = {'loss_A': float(la), 'loss_B': float(lb),
           'max_gradient_difference_over_max_gradient': max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(ga, gb))}
    assert abs(row['loss_A'] - row['loss_B']) <= 1e-5 * abs(row['loss_A']) and row['max_gradient_difference_over_max_gradient'] <= 1e-4, row
    del la, lb, ga, gb

    def window(side, n):
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(n):
        step(side)
      e1.record()
      torch.cuda.synchronize()
      return 1e-3 * e0.elapsed_time(e1)

    iters = {}
    for side in ('A', 'B'):
      window(side, 3)  # warm-up: allocator, kernels loaded
      per = window(side, 5) / 5
      iters[side] = max(5, int(math.ceil(1.2 * args.min_window / per)))
    times = {'A': [], 'B': []}
    for w in range(args.windows):
      for side in ('A', 'B'):
        sec = window(side, iters[side])
        while sec < args.min_window:  # the calibration ran slow: a longer window, and this one is not counted
          iters[side] = int(math.ceil(1.3 * iters[side] * args.min_window / sec))
          sec = window(side, iters[side])
        times[side].append(1e6 * sec / iters[side])
        print('B=%d window %d %s: %.1f us per forward + backward (%d in %.3f s)' % (B, w, side, times[side][-1], iters[side], sec), flush=True)
    nbytes = 4 * (2 * 7 + 1) * K * B * H * W
    for side in ('A', 'B'):
      v = sorted(times[side])
      row['%s_us' % side] = [round(x, 1) for x in times[side]]
      row['%s_us_median_min_max' % side] = [round(0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2]), 1), round(v[0], 1), round(v[-1], 1)]
    row['B_algorithmic_bytes'] = nbytes
    row['B_effective_GBps'] = [round(nbytes / (us * 1e-6) / 1e9, 1) for us in times['B']]
    row['speedup_median'] = round(row['A_us_median_min_max'][0] / row['B_us_median_min_max'][0], 2)
    row['every_B_window_faster_than_every_A_window'] = max(times['B']) < min(times['A'])
    ok = ok and row['every_B_window_faster_than_every_A_window']
    out['batch'][str(B)] = row
  out['every_B_window_faster_than_every_A_window'] = ok
  line = json.dumps(out)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(main())
