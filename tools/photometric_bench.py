#!/usr/bin/env python3
"""A/B of the self-supervised stereo loss on one MI355X, in one process: the loss composed from torch operators in fp32 on
the GPU (A; the only way a user has without HF.photometric_loss: elementwise, roll, gather and reduction launches, autograd's scatter in
the backward) against HF.photometric_loss (B; csrc/photometric.hip), forward + backward, at 1024 x 512 with K = 3 maps, B = 2 and B = 12.

    python tools/photometric_bench.py [--windows 4] [--min-window 0.3] [--out FILE.json]
    python tools/photometric_bench.py --lr [--out profiles/selfsup_bench_mi355x.json]     (below)

The composition below is written from the definition in include/mode_hip.h.  First the two sides' outputs are compared (loss, and the
gradient relative to its largest element); then windows alternate A B A B ..., each at least --min-window seconds of device time between
two events.  Acceptance: every B window faster than every A window.  For B also the algorithmic bytes -- per pixel and map 7 floats read
(3 left, 3 right, 1 disparity) in each pass and 1 written in the backward, 60 B -- over its device time: an effective rate (the images
are re-read per map and the halo from cache, so it is not a share of the HBM peak).

--lr: the whole bidirectional loss -- left-right consistency of K left and K right maps with dmax = 192, and both views'
photometric loss gated by the consistency masks -- composed from torch operators (A, written from the definitions in
include/mode_hip_selfsup.h) against HF.lr_consistency + HF.photometric_loss(view=, masks=) (B).  The maps are integers + 0.5 and
tau = 0.75: every |own - other(x)| is then a multiple of 0.5 in any precision, no pixel sits near the threshold, and the two sides (and a
float64 run of the composition) agree on every mask.  Before timing, B's loss and gradients are held to the bound of
tests/test_gpu_selfsup.py: at most 4 x the yardstick, which is A's own fp32 error against the float64 composition, never below
2^-23 of the quantity's largest element.  --kernels-only N runs N steps of side B and nothing else (for a kernel trace)."""
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


def composed_loss(torch, left, right, disps, weights, alpha=0.85, lam=0.1, beta=1.0, C1=1e-4, C2=9e-4, s=-1, masks=None):
  """s, masks: x = w + s d (s = +1: `left` is the right camera's image, the view's own), masks[k] (B, H, W) bool and-ed
  into the validity of a pixel.  The arithmetic is that of the disparities' dtype."""
  from dataloader.preprocess import imagenet_stats
  dt = disps[0].dtype
  mean = torch.tensor(imagenet_stats['mean'], device=left.device, dtype=dt).view(1, 3, 1, 1)
  std = torch.tensor(imagenet_stats['std'], device=left.device, dtype=dt).view(1, 3, 1, 1)
  left, right = left.to(dt), right.to(dt)
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
  wcol = torch.arange(W, dtype=dt, device=left.device).view(1, 1, W)
  loss = 0
  for k, (d, wgt) in enumerate(zip(disps, weights)):
    d = d.reshape(B, H, W)
    x = wcol + s * d
    valid = torch.isfinite(d) & (x >= 0) & (x <= W - 1)
    if masks is not None:
      valid = valid & masks[k]
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


def composed_lr(torch, dls, drs, weights, tau, dmax):
  """The left-right term of include/mode_hip_selfsup.h -> (loss, masks[view][k] (B, H, W) bool)."""
  W = dls[0].shape[-1]
  wcol = torch.arange(W, dtype=dls[0].dtype, device=dls[0].device).view(1, 1, W)
  loss, masks = 0, ([], [])
  for dl, dr, wgt in zip(dls, drs, weights):
    for v, (s, own, other) in enumerate(((-1, dl, dr), (1, dr, dl))):
      zero = torch.zeros_like(own)
      x = wcol + s * own
      valid = torch.isfinite(own) & (own >= 0) & (own <= dmax) & (x >= 0) & (x <= W - 1)
      own_s, xv = torch.where(valid, own, zero), torch.where(valid, x, zero)
      x0 = xv.detach().floor().clamp(max=W - 2)
      t = xv - x0
      i0 = x0.long()
      o0, o1 = other.gather(2, i0), other.gather(2, i0 + 1)
      valid = valid & torch.isfinite(o0) & torch.isfinite(o1)
      e = torch.where(valid, (own_s - ((1 - t) * torch.where(valid, o0, zero) + t * torch.where(valid, o1, zero))).abs(), zero)
      loss = loss + wgt * e.sum() / valid.sum().clamp(min=1)
      masks[v].append(valid & (e.detach() <= tau))
  return loss, masks


def composed_selfsup(torch, left, right, dls, drs, weights, tau, dmax):
  """Both views' loss with the consistency masks + the consistency term -> (loss, masks)."""
  lr, masks = composed_lr(torch, dls, drs, weights, tau, dmax)
  loss = (composed_loss(torch, left, right, dls, weights, s=-1, masks=masks[0]) +
          composed_loss(torch, right, left, drs, weights, s=1, masks=masks[1]) + lr)
  return loss, masks


def lr_inputs(torch, B, H, W, K, dev, seed):
  """The images of inputs() and K left and K right maps: integers on a smooth field plus noise, + 0.5 (see the module's text)."""
  left, right, _ = inputs(torch, B, H, W, K, dev, seed)
  g = torch.Generator(device=dev).manual_seed(seed + 1)
  hh = torch.linspace(0, 2 * math.pi, H, device=dev).view(1, H, 1)
  ww = torch.linspace(0, math.pi, W, device=dev).view(1, 1, W)
  maps = ([], [])
  for k in range(K):
    field = 90 + 80 * torch.sin(hh + k) * torch.sin(ww)  # 10 .. 170: inside dmax = 192
    for side in maps:
      side.append((torch.floor(field + 1.5 * torch.rand(B, H, W, generator=g, device=dev)) + 0.5).contiguous())
  return left, right, maps[0], maps[1]


def main_lr(args):
  import torch
  from mode_hip import functional as HF
  assert torch.cuda.is_available(), 'photometric_bench needs a GPU'
  dev = torch.device('cuda:0')
  H, W, K, tau, dmax = 1024, 512, 3, 0.75, 192
  out = {'tool': 'photometric_bench --lr', 'H': H, 'W': W, 'K': K, 'tau': tau, 'dmax': dmax, 'min_window_s': args.min_window,
         'windows': args.windows, 'batch': {}}
  ok = True
  for B in args.batches:
    left, right, dls, drs = lr_inputs(torch, B, H, W, K, dev, 100 + B)

    def step(side, dtype=torch.float32):
      ls = [d.detach().to(dtype).requires_grad_(True) for d in dls]
      rs = [d.detach().to(dtype).requires_grad_(True) for d in drs]
      if side == 'A':
        loss, masks = composed_selfsup(torch, left, right, ls, rs, WEIGHTS, tau, dmax)
        masks = torch.stack([torch.stack(m) for m in masks])
      else:
        lr, masks = HF.lr_consistency(ls, rs, WEIGHTS, tau=tau, dmax=dmax, return_masks=True)
        loss = (HF.photometric_loss(left, right, ls, WEIGHTS, view='left', masks=masks[0]) +
                HF.photometric_loss(right, left, rs, WEIGHTS, view='right', masks=masks[1]) + lr)
      loss.backward()
      return loss.detach(), [d.grad for d in ls + rs], masks

    if args.kernels_only:
      for _ in range(args.kernels_only):
        step('B')
      torch.cuda.synchronize()
      continue

    l64, g64, m64 = step('A', torch.float64)
    la, ga, ma = step('A')
    lb, gb, mb = step('B')
    torch.cuda.synchronize()
    row = {'loss_64': float(l64), 'loss_A': float(la), 'loss_B': float(lb), 'visible_fraction': float(m64.float().mean()),
           'mask_bytes_differing_A_B_from_64': [int((ma != m64).sum()), int((mb.bool() != m64).sum())]}
    assert row['mask_bytes_differing_A_B_from_64'] == [0, 0], row
    floor = 2.0 ** -23
    yl = max(abs(float(la) - float(l64)) / abs(float(l64)), floor)
    el = abs(float(lb) - float(l64)) / abs(float(l64))
    row['loss_error_over_yardstick'] = round(el / yl, 3)
    ratios = []
    for a, b, r in zip(ga, gb, g64):
      scale = float(r.abs().max())
      yg = max(float((a.double() - r).abs().max()) / scale, floor)
      ratios.append(round(float((b.double() - r).abs().max()) / scale / yg, 3))
    row['gradient_error_over_yardstick_dl_then_dr'] = ratios
    print('B=%d: %s' % (B, json.dumps(row)), flush=True)
    assert el <= 4 * yl and max(ratios) <= 4, row
    del l64, g64, m64, la, ga, ma, lb, gb, mb
    torch.cuda.empty_cache()

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
    for side in ('A', 'B'):
      v = sorted(times[side])
      row['%s_us' % side] = [round(x, 1) for x in times[side]]
      row['%s_us_median_min_max' % side] = [round(0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2]), 1), round(v[0], 1), round(v[-1], 1)]
    row['speedup_median'] = round(row['A_us_median_min_max'][0] / row['B_us_median_min_max'][0], 2)
    row['every_B_window_faster_than_every_A_window'] = max(times['B']) < min(times['A'])
    # the backward's gather: per row and view, W targets each walk ceil(dmax) + 3 records
    row['lr_bwd_lds_record_reads'] = 2 * K * B * H * W * (dmax + 3)
    ok = ok and row['every_B_window_faster_than_every_A_window']
    out['batch'][str(B)] = row
  if args.kernels_only:
    return 0
  out['every_B_window_faster_than_every_A_window'] = ok
  line = json.dumps(out)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')
  return 0 if ok else 1


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
  ap.add_argument('--lr', action='store_true', help='the bidirectional loss of DESIGN 24 instead of the left-view loss of DESIGN 22')
  ap.add_argument('--kernels-only', type=int, default=0, help='with --lr: N steps of side B and nothing else (for a kernel trace)')
  args = ap.parse_args()
  if args.lr:
    return main_lr(args)

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
