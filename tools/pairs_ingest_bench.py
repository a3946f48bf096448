"""Time the Deep360 pair ingest at a working size other than the stored one: decoded 1024 x 512 pairs and their disparity maps in host
memory to the normalised pairs and the disparity ground truth on the device, at 512 x 256 (BASELINE configs[0]) and 2048 x 1024
(configs[4]), for batches of 1 and 8.

    python tools/pairs_ingest_bench.py [--batches 1 8] [--reps 20] [--out profiles/pairs_ingest_bench.json]

Three ways, alternating A B A B per repetition:
  A  the host path as dataloader.deep360_loader.Deep360DatasetDisparity runs it per sample (PIL.Image.resize of both images, the
     nearest-neighbour resize of the disparity times the width ratio, the stage-1 transform), one sample after the other with 16 host
     threads, the default collate's stack, and the upload of the three float tensors
  B  the upload of the decoded bytes and the stored disparity maps, and dataloader.gpu_ingest.pairs_u8_gpu on them
  C  pairs_u8_gpu alone on device-resident inputs, between device events over a window of calls, with the bytes it has to move
     (inputs read once, the 8-bit intermediate written and read once, every output written once) over that time
A and B: host clock around work that ends in a device synchronise; medians in ms.  A and B produce the same tensors (asserted, bit for
bit, NaN where the host has NaN).  Seeded random inputs; the timings do not depend on the values.  Writes one JSON file."""
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
from PIL import Image  # noqa: E402

from dataloader import deep360_loader as L  # noqa: E402
from dataloader import gpu_ingest, preprocess  # noqa: E402

DEV = 'cuda:0'
HS, WS = 1024, 512
SIZES = ((512, 256), (2048, 1024))
HOST_THREADS = 16
KEYS = ('leftImg', 'rightImg', 'dispMap')


def make_batch(N, seed):
  rng = np.random.RandomState(seed)
  u8 = rng.randint(0, 256, (N, 2, HS, WS, 3)).astype(np.uint8)
  u8[:, :, 100:300, 60:200] = 255
  disp = (60.0 * rng.rand(N, HS, WS)).astype(np.float32)
  disp[:, 500:560, 100:180] = np.nan
  return u8, disp


def host_path(u8, disp, shape, norm):
  """A: per sample as the loader's __getitem__ from the decoded images on, stacked as the default collate stacks them, uploaded."""
  H, W = shape
  items = []
  for n in range(u8.shape[0]):
    views = [Image.fromarray(u8[n, s]).resize((W, H)) for s in (0, 1)]
    d = L.resize_nearest(disp[n], W, H) * (W / WS)
    items.append((norm(views[0]), norm(views[1]), torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))[None]))
  return {k: torch.stack([it[i] for it in items]).to(DEV) for i, k in enumerate(KEYS)}


def device_path(u8_t, disp_t, shape):
  """B: upload of the decoded inputs, one pairs_u8_gpu call."""
  return gpu_ingest.pairs_u8_gpu(u8_t.to(DEV), disp_t.to(DEV), shape=shape)


def moved_bytes(N, shape):
  H, W = shape
  ins = N * 2 * HS * WS * 3 + N * H * W * 4            # every byte of the pair; one source element per disparity output
  mid = 2 * (N * 2 * HS * W * 3)                       # the horizontal pass' 8-bit result, written and read
  outs = 2 * N * 3 * H * W * 4 + N * H * W * 4
  return ins + mid + outs


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


def line(N, shape, reps, warmup):
  norm = preprocess.get_transform_stage1(augment=False)
  u8, disp = make_batch(N, 700 + N)
  u8_t, disp_t = torch.from_numpy(u8), torch.from_numpy(disp)  # pageable host memory, as a loader hands it over
  parts = {'A': [], 'B': []}

  def clock(key, fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    parts[key].append(1e3 * (time.perf_counter() - t0))
    return out

  a = lambda: clock('A', lambda: host_path(u8, disp, shape, norm))
  b = lambda: clock('B', lambda: device_path(u8_t, disp_t, shape))
  ra, rb = a(), b()
  for k in KEYS:
    assert torch.equal(ra[k].isnan(), rb[k].isnan()) and torch.equal(ra[k].nan_to_num(-1.0), rb[k].nan_to_num(-1.0)), k
  del ra, rb
  for _ in range(warmup):
    a(), b()
  for v in parts.values():
    del v[:]
  for _ in range(reps):
    a(), b()
  d_u8, d_disp = u8_t.to(DEV), disp_t.to(DEV)
  ms_c, calls = events_ms(lambda: gpu_ingest.pairs_u8_gpu(d_u8, d_disp, shape=shape))
  nbytes = moved_bytes(N, shape)
  row = {'batch': N, 'stored': [HS, WS], 'shape': list(shape), 'reps': reps, 'host_threads': torch.get_num_threads(),
         'A_host_path_upload_ms': float(np.median(parts['A'])), 'A_min_ms': float(np.min(parts['A'])),
         'B_upload_bytes_pairs_u8_gpu_ms': float(np.median(parts['B'])), 'B_min_ms': float(np.min(parts['B'])),
         'A_over_B': float(np.median(parts['A']) / np.median(parts['B'])),
         'C_pairs_u8_gpu_ms': ms_c, 'C_calls_timed': calls, 'C_bytes': nbytes, 'C_GB_per_s': nbytes / (ms_c * 1e-3) / 1e9}
  print(json.dumps(row), flush=True)
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pairs_ingest_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'this benchmark needs the GPU'
  torch.set_num_threads(HOST_THREADS)
  import PIL
  rows = [line(N, shape, args.reps, args.warmup) for shape in SIZES for N in args.batches]
  out = {'tool': 'tools/pairs_ingest_bench.py', 'stored': [HS, WS], 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
         'numpy': np.__version__, 'pillow': PIL.__version__, 'rows': rows}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
