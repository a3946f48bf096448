#!/usr/bin/env python3
"""A/B of the training step's optimizer on one MI355X, in one process: torch.optim.Adam(fused=True) as bench.py constructs it (A) against
mode_hip.optim.Adam (B), on the 243 parameter tensors (5 489 280 floats) of ModeDisparity(192, 'Sphere', 1024, 512, 'Cassini').  No forward
pass: gradients come from a seed.

    python tools/optim_bench.py [--steps 200] [--warmup 20] [--windows 4] [--out FILE.json]
    python tools/optim_bench.py --only B --steps 10 --warmup 0        # under `rocprofv3 --kernel-trace --stats`: the launches of one side
    python tools/optim_bench.py launches SHORT.csv STEPS LONG.csv STEPS   # launches per step() from the kernel-stats CSVs of two such runs
                                                                          # of different length (the set-up's own kernels cancel)

After the warm-up the windows alternate A B A B ...; each holds `--steps` step() calls.  Per window: device time from two events around the
window, host time from a host clock around the un-synchronised calls (the device is idle when a window starts).  Acceptance: every
B window at or below every A window, in device and in host time.  For B also the bytes the algorithm moves per step -- 7 x 4 x n for the
update (p, exp_avg, exp_avg_sq read and written, the gradient read) plus 4 x n for the norm pass -- over its device time: an EFFECTIVE rate on
a working set of 4 x 4 x n = 88 MB + tables that fits the 256 MB Infinity Cache, not a share of the HBM peak."""
import argparse
import copy
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)


def launches(short, steps_short, long, steps_long):
  calls = []
  for path in (short, long):
    with open(path) as f:
      calls.append({r['Name']: int(r['Calls']) for r in csv.DictReader(f)})
  per_step = {}
  for name in calls[1]:
    d = calls[1][name] - calls[0].get(name, 0)
    if d:
      per_step[name] = d / float(steps_long - steps_short)
  for name, v in sorted(per_step.items(), key=lambda kv: -kv[1]):
    print('  %8.2f per step  %s' % (v, name[:160]))
  print(json.dumps({'kernel_launches': [sum(c.values()) for c in calls], 'steps': [steps_short, steps_long],
                    'launches_per_step': sum(per_step.values())}))


def main():
  if len(sys.argv) > 1 and sys.argv[1] == 'launches':
    return launches(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=200, help='step() calls per timed window')
  ap.add_argument('--warmup', type=int, default=20)
  ap.add_argument('--windows', type=int, default=4, help='windows per side')
  ap.add_argument('--only', choices=['A', 'B'], help='run one side only, untimed windows (for a kernel trace)')
  ap.add_argument('--out', help='also write the result line to this file')
  args = ap.parse_args()

  import torch
  import models
  from mode_hip import data_parallel, optim
  assert torch.cuda.is_available(), 'optim_bench needs a GPU'
  dev = torch.device('cuda:0')
  torch.manual_seed(0)
  net_a = models.ModeDisparity(192, 'Sphere', 1024, 512, 'Cassini').to(dev)
  net_b = copy.deepcopy(net_a)
  sides = {}
  for name, net in (('A', net_a), ('B', net_b)):
    red = data_parallel.GradAllReducer(net, fuse_accumulation=False)  # both sides read their gradients from one flat buffer, as in bench.py
    g = torch.Generator(device=dev).manual_seed(1234)
    red.flat.copy_(1e-3 * torch.randn(red.flat.numel(), generator=g, device=dev))
    sides[name] = (net, red)
  n, tensors = sides['A'][1].flat.numel(), len(sides['A'][1].params)
  assert (tensors, n) == (243, 5489280), (tensors, n)
  try:  # bench.py's construction
    opt_a = torch.optim.Adam(net_a.parameters(), lr=1e-3, betas=(0.9, 0.999), fused=True)
  except (TypeError, RuntimeError):
    opt_a = torch.optim.Adam(net_a.parameters(), lr=1e-3, betas=(0.9, 0.999))
  opt_b = optim.Adam(net_b.parameters(), lr=1e-3, betas=(0.9, 0.999), flat_grads=sides['B'][1].flat)
  opts = {'A': opt_a, 'B': opt_b}
  order = [args.only] if args.only else ['A', 'B']

  for name in order:
    for _ in range(args.warmup):
      opts[name].step()
  torch.cuda.synchronize()
  result = {s: {'device_us': [], 'host_us': []} for s in order}
  for w in range(args.windows):
    for name in order:
      opt = opts[name]
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      t0 = time.perf_counter()
      for _ in range(args.steps):
        opt.step()
      t1 = time.perf_counter()
      e1.record()
      torch.cuda.synchronize()
      result[name]['device_us'].append(1e3 * e0.elapsed_time(e1) / args.steps)
      result[name]['host_us'].append(1e6 * (t1 - t0) / args.steps)
      print('window %d %s: device %.2f us / step, host %.2f us / step()' % (w, name, result[name]['device_us'][-1], result[name]['host_us'][-1]), flush=True)
  if args.only:
    print(json.dumps({'only': args.only, 'steps': args.steps * args.windows + args.warmup}))
    return
  # the two sides saw the same gradients for the same number of steps: how far apart are the parameters?
  pa = torch.cat([p.detach().reshape(-1) for p in net_a.parameters() if p.requires_grad])
  pb = torch.cat([p.detach().reshape(-1) for p in net_b.parameters() if p.requires_grad])
  out = {'tool': 'optim_bench', 'tensors': tensors, 'numel': n, 'steps_per_window': args.steps, 'windows': args.windows,
         'max_abs_param_difference_A_B': float((pa - pb).abs().max()), 'B_skipped_steps': float(opt_b.skipped_steps)}
  for s in order:
    for k in ('device_us', 'host_us'):
      v = result[s][k]
      out['%s_%s' % (s, k)] = [round(x, 3) for x in v]
      out['%s_%s_min_max' % (s, k)] = [round(min(v), 3), round(max(v), 3)]
  out['B_bytes_per_step'] = opt_b.bytes_per_step
  out['B_effective_GBps_in_infinity_cache'] = [round(opt_b.bytes_per_step / (us * 1e-6) / 1e9, 1) for us in result['B']['device_us']]
  out['every_B_window_at_or_below_every_A_window'] = {k: max(result['B'][k]) <= min(result['A'][k]) for k in ('device_us', 'host_us')}
  line = json.dumps(out)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
