"""Time the 3D60 ingest: decoded equirectangular pairs in host memory to the normalised Cassini pairs and their disparity ground truth
on the device, at the paper's 3D60 size (ERP 256 x 512 -> Cassini 512 x 256), for batches of 1 and 8.

    python tools/ingest3d60_bench.py [--batches 1 8] [--reps 20] [--out profiles/ingest3d60_bench.json]

One row per batch size with pair 'lr' (one grid serves the batch), and one more at the largest batch with the three pairs mixed (a
grid per sample, concatenated on the device from the cached per-pair grids: what a loader with pair='all' produces).

Three ways, alternating A B A B per repetition:
  A  the reference's host path as dataloader.dataset3D60Loader restates it (host_sample per sample: four CPU grid_sample calls, the
     byte truncation, the sine rule for the pair and its twin; then the stage-1 transform of the four images), with 16 host threads,
     and the upload of the six resulting tensors
  B  the upload of the decoded bytes and the two ERP depth maps, and dataloader.gpu_ingest.erp_pairs_gpu on them
  C  erp_pairs_gpu alone on device-resident inputs, between device events over a window of calls, with the bytes it has to move
     (inputs and grid read once, every output written once) over that time
A and B: host clock around work that ends in a device synchronise; medians in ms.  A and B produce the same images (asserted, bit for
bit) and disparities within 1e-3 px.  Seeded random inputs; the timings do not depend on the values.  Writes one JSON file."""
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

from dataloader import dataset3D60Loader as L  # noqa: E402
from dataloader import gpu_ingest, preprocess  # noqa: E402

DEV = 'cuda:0'
HE, WE, H, W = 256, 512, 512, 256
HOST_THREADS = 16
KEYS = ('leftImg', 'rightImg', 'dispMap', 'leftImg_flip', 'rightImg_flip', 'dispMap_flip')


def make_batch(N, seed):
  rng = np.random.RandomState(seed)
  u8 = rng.randint(0, 256, (N, 2, HE, WE, 3)).astype(np.uint8)
  u8[:, :, 40:120, 60:200] = 255
  depth = (25.0 * (1.0 - rng.rand(2, N, HE, WE))).astype(np.float32)
  depth[:, :, 150:170, 100:180] = 0
  return u8, depth[0], depth[1]


def host_path(u8, dl, dr, pair, norm):
  """A: per sample as the loader's __getitem__, stacked as the default collate stacks them, uploaded."""
  items = []
  for n in range(u8.shape[0]):
    left, right, disp, left_f, right_f, disp_f = L.host_sample(u8[n, 0], u8[n, 1], dl[n], dr[n], pair[n], (H, W))
    items.append((norm(left), norm(right), torch.from_numpy(disp).unsqueeze_(0), norm(left_f), norm(right_f),
                  torch.from_numpy(disp_f).unsqueeze_(0)))
  return {k: torch.stack([it[i] for it in items]).to(DEV) for i, k in enumerate(KEYS)}


def device_path(u8_t, dl_t, dr_t, pair):
  """B: upload of the decoded inputs, one erp_pairs_gpu call."""
  return gpu_ingest.erp_pairs_gpu(u8_t.to(DEV), dl_t.to(DEV), dr_t.to(DEV), pair=pair, shape=(H, W))


def moved_bytes(N, G):
  ins = N * 2 * HE * WE * 3 + 2 * N * HE * WE * 4 + 3 * G * H * W * 2 * 4  # the grid is read by each of the three launches
  outs = 4 * N * 3 * H * W * 4 + 2 * N * H * W * 4
  return ins + outs


def events_ms(fn, window=0.5, warmup=3):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  n = 8
  while True:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
      fn()
    e.record()
    e.synchronize()
    ms = s.elapsed_time(e)
    if ms >= 1000 * window:
      return ms / n, n
    n *= 4


def line(N, reps, warmup, pair):
  """pair: a list of N pair names."""
  norm = preprocess.get_transform_stage1(augment=False)
  u8, dl, dr = make_batch(N, 600 + N)
  u8_t, dl_t, dr_t = torch.from_numpy(u8), torch.from_numpy(dl), torch.from_numpy(dr)  # pageable host memory, as a loader hands it over
  parts = {'A': [], 'B': []}

  def clock(key, fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    parts[key].append(1e3 * (time.perf_counter() - t0))
    return out

  a = lambda: clock('A', lambda: host_path(u8, dl, dr, pair, norm))
  b = lambda: clock('B', lambda: device_path(u8_t, dl_t, dr_t, pair))
  ra, rb = a(), b()
  worst = 0.0
  for k in KEYS:
    if 'Img' in k:
      assert torch.equal(ra[k], rb[k]), k
    else:
      assert torch.equal(ra[k].isnan(), rb[k].isnan()), k
      worst = max(worst, float((ra[k].double() - rb[k].double()).abs().nan_to_num().max()))
  assert worst <= 1e-3, worst
  for _ in range(warmup):
    a(), b()
  for v in parts.values():
    del v[:]
  for _ in range(reps):
    a(), b()
  d_u8, d_dl, d_dr = u8_t.to(DEV), dl_t.to(DEV), dr_t.to(DEV)
  ms_c, calls = events_ms(lambda: gpu_ingest.erp_pairs_gpu(d_u8, d_dl, d_dr, pair=pair, shape=(H, W)))
  nbytes = moved_bytes(N, 1 if len(set(pair)) == 1 else N)
  row = {'batch': N, 'pair': pair[0] if len(set(pair)) == 1 else 'mixed', 'reps': reps, 'host_threads': torch.get_num_threads(),
         'A_host_path_upload_ms': float(np.median(parts['A'])), 'A_min_ms': float(np.min(parts['A'])),
         'B_upload_bytes_erp_pairs_gpu_ms': float(np.median(parts['B'])), 'B_min_ms': float(np.min(parts['B'])),
         'A_over_B': float(np.median(parts['A']) / np.median(parts['B'])),
         'C_erp_pairs_gpu_ms': ms_c, 'C_calls_timed': calls, 'C_bytes': nbytes, 'C_GB_per_s': nbytes / (ms_c * 1e-3) / 1e9,
         'largest_disp_difference_px': worst}
  print(json.dumps(row), flush=True)
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ingest3d60_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'this benchmark needs the GPU'
  torch.set_num_threads(HOST_THREADS)
  rows = [line(N, args.reps, args.warmup, ['lr'] * N) for N in args.batches]
  if max(args.batches) >= 3:
    rows.append(line(max(args.batches), args.reps, args.warmup, [('lr', 'ud', 'ur')[n % 3] for n in range(max(args.batches))]))
  out = {'tool': 'tools/ingest3d60_bench.py', 'erp': [HE, WE], 'cassini': [H, W], 'device': torch.cuda.get_device_name(0),
         'torch': torch.__version__, 'numpy': np.__version__, 'rows': rows}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
