#!/usr/bin/env python3
"""What the colour augmentation costs on one MI355X, in one process, against the plain 8-bit ingest and against doing it on
the host.  Two workloads: one Deep360 frame (12 panoramas of 1024 x 512) and a batch of 3D60 pairs (ERP 256 x 512 -> Cassini 512 x 256).

    python tools/augment_bench.py [--calls 50] [--warmup 5] [--windows 4] [--pairs 8] [--host-calls 3] [--out FILE.json]

Per workload three sides, in alternating windows A B C A B C ... of `--calls` calls each (the host side: `--host-calls`):
  host   the float32 transform in torch on the CPU with 16 threads (ToTensor, the three blends in the drawn order, Lighting, Normalize --
         the arithmetic of include/mode_hip.h, batched per image) and the upload of the float32 result; wall time
  aug    dataloader.gpu_ingest.frames_u8_gpu(augment=params) / erp_pairs_gpu(augment=params); device time from two events
  plain  the same call without augment=: the yardstick; device time
For the frame also `aug_planes`: augment_u8_gpu alone (the two launches, without the copy of the four fusion panoramas' planes).
Achieved GB/s counts 3 bytes in per pixel per pass over the bytes (two passes for an image with a contrast step, one otherwise) and 12
bytes out.  No pass / fail threshold: the numbers go into DESIGN 18."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)


def host_augment(images_u8, ops, coef):
  """(N, H, W, 3) uint8 CPU tensor, ops (N, 3), coef (N, 9) -> (N, 3, H, W) float32: the contract of include/mode_hip.h in torch."""
  import torch
  k = torch.tensor([0.2989, 0.587, 0.114]).view(3, 1, 1)
  mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
  std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
  out = torch.empty((images_u8.shape[0], 3) + tuple(images_u8.shape[1:3]))
  for n in range(images_u8.shape[0]):
    x = images_u8[n].permute(2, 0, 1).to(torch.float32).div(255)
    grey = lambda t: ((k[0] * t[0] + k[1] * t[1]) + k[2] * t[2])
    for op in ops[n].tolist():
      if op not in (0, 1, 2):
        continue
      rho, sigma = coef[n, 2 * op], coef[n, 2 * op + 1]
      other = 0.0 if op == 0 else (grey(x).mean() if op == 1 else grey(x).unsqueeze(0))
      x = (rho * x + sigma * other).clamp(0, 1)
    out[n] = ((x + coef[n, 6:9].view(3, 1, 1)) - mean) / std
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=50, help='device calls per timed window')
  ap.add_argument('--host-calls', type=int, default=3, help='host-path calls per timed window')
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--windows', type=int, default=4, help='windows per side')
  ap.add_argument('--pairs', type=int, default=8, help='3D60 pairs in the batch')
  ap.add_argument('--out', help='also write the result line to this file')
  args = ap.parse_args()

  import numpy as np
  import torch
  from dataloader import gpu_ingest as G
  assert torch.cuda.is_available(), 'augment_bench needs a GPU'
  torch.set_num_threads(16)
  dev = torch.device('cuda:0')
  rng = np.random.RandomState(0)
  gen = torch.Generator().manual_seed(0)

  H, W = 1024, 512
  frame_host = torch.from_numpy(rng.randint(0, 256, (1, 12, H, W, 3)).astype(np.uint8))
  frame = frame_host.to(dev)
  p_frame = G.draw_colour_params(12, dev, generator=gen)
  N, He, We, Hc, Wc = args.pairs, 256, 512, 512, 256
  pairs = torch.from_numpy(rng.randint(0, 256, (N, 2, He, We, 3)).astype(np.uint8)).to(dev)
  p_pairs = G.draw_colour_params(2 * N, dev, generator=gen, share=2)
  cassini_host = G.erp_pairs_gpu(pairs, shape=(Hc, Wc), return_u8=True)['cassini_u8'].cpu().view(2 * N, Hc, Wc, 3)

  def host_side(images, p):
    def call():
      host_augment(images, p.ops_host, p.coef_host).to(dev)
      torch.cuda.synchronize()
    return call

  work = {
      'frame_1024x512': {
          'pixels': 12 * H * W, 'params': p_frame,
          'host': host_side(frame_host.view(12, H, W, 3), p_frame),
          'aug': lambda: G.frames_u8_gpu(frame, augment=p_frame),
          'aug_planes': lambda: G.augment_u8_gpu(frame.view(12, H, W, 3), p_frame),
          'plain': lambda: G.frames_u8_gpu(frame)},
      'pairs_3d60_%dx512x256' % N: {
          'pixels': 2 * N * Hc * Wc, 'params': p_pairs,
          'host': host_side(cassini_host, p_pairs),
          'aug': lambda: G.erp_pairs_gpu(pairs, shape=(Hc, Wc), augment=p_pairs),
          'plain': lambda: G.erp_pairs_gpu(pairs, shape=(Hc, Wc))},
  }
  out = {'tool': 'augment_bench', 'calls_per_window': args.calls, 'host_calls_per_window': args.host_calls, 'windows': args.windows,
         'host_threads': torch.get_num_threads()}
  for name, w in work.items():
    sides = [s for s in ('host', 'aug', 'aug_planes', 'plain') if s in w]
    for s in sides:
      for _ in range(args.warmup if s != 'host' else 1):
        w[s]()
    torch.cuda.synchronize()
    ms = {s: [] for s in sides}
    for k in range(args.windows):
      for s in sides:
        torch.cuda.synchronize()
        if s == 'host':
          t0 = time.perf_counter()
          for _ in range(args.host_calls):
            w[s]()
          ms[s].append(1e3 * (time.perf_counter() - t0) / args.host_calls)
        else:
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for _ in range(args.calls):
            w[s]()
          e1.record()
          torch.cuda.synchronize()
          ms[s].append(e0.elapsed_time(e1) / args.calls)
        print('%s window %d %-10s %.4f ms / call' % (name, k, s, ms[s][-1]), flush=True)
    with_contrast = int((w['params'].ops_host == G.OP_CONTRAST).any(1).sum())
    n_img = w['params'].n
    per_px = {'aug_planes': 3.0 * (1 + with_contrast / n_img) + 12, 'plain': 3.0 + 12}
    res = {'pixels': w['pixels'], 'images_with_contrast': with_contrast, 'images': n_img}
    for s in sides:
      res['%s_ms' % s] = [round(v, 4) for v in ms[s]]
      res['%s_ms_min_max' % s] = [round(min(ms[s]), 4), round(max(ms[s]), 4)]
    for s, b in per_px.items():
      if s in ms and not (name.startswith('pairs') and s == 'plain'):  # (the pairs' plain call is the re-projection, not a streaming pass)
        res['%s_GBps' % s] = [round(w['pixels'] * b / (v * 1e-3) / 1e9, 1) for v in ms[s]]
    out[name] = res
  line = json.dumps(out)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
