#!/usr/bin/env python3
"""Output hashes of the two spherical gradient operators, taken on the GPU at the commit BEFORE their polar kernels were rescheduled.

  python tests/golden/make_golden_polar_bits.py     # writes polar_parent_bits.json (needs the MI355X)

polar_parent_bits.json: SHA-256 of the raw bytes (fp32, C order) of what (a) HF.sphere_conv_bwd_data_t and (b)
HF.sphere_conv_bwd_weight_t write for the cases below, under the `bf16x6` arithmetic with every switch at its default.  The
rescheduled kernels (sphere_bwd_data_adj9_kernel on 8 waves, sphere_bww_polar_split_kernel with its loads issued ahead) keep every
output element's sequence of operations, so tests/test_gpu_polar_bits.py recomputes the outputs and compares the hashes: one
differing bit anywhere fails it.  Do not regenerate this file together with a kernel change -- it pins what the parent computed.

Inputs: the seeded CPU generator of tests/test_gpu_split.py (`_rand`, restated here so that the fixture does not depend on a test
module), the seeds of its spherical tests."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

OUT = os.path.join(HERE, 'polar_parent_bits.json')
DEV = 'cuda:0'

# (ih, iw, B, ci, co, groups)
BWD_DATA = [(32, 64, 3, 40, 16, 1),     # the list kernel does most tiles here; channel count off the 32-block
            (128, 256, 1, 48, 32, 2)]
BWD_WEIGHT = [(128, 256, 1, 40, 24, 1),
              (128, 256, 2, 64, 128, 1)]  # polar items exist only at this table size


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def key(kind, case):
  return '%s/%dx%d_B%d_%d->%d_g%d' % ((kind,) + tuple(case[:3]) + (case[3], case[4], case[5]))


def digest(t):
  return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def bwd_data(case):
  """One call of HF.sphere_conv_bwd_data_t on NaN-filled storage (the operator writes every element); returns gxt on the device."""
  from mode_hip import functional as HF
  from oracle import mode_ref
  ih, iw, B, ci, co, groups = case
  pos = mode_ref.sphere_position(ih, iw, 'Cassini').contiguous()
  H, W = pos.shape[2:]
  w = _rand((co, ci // groups, 3, 3), 401, (2.0 / (9 * ci // groups))**0.5)
  gy = _rand((B, co, H, W), 402)
  pd, wd = pos.to(DEV), w.to(DEV)
  gyt = gy.to(DEV).transpose(2, 3).contiguous()

  def run():
    gxt = torch.full((B, ci, W, H), float('nan'), device=DEV)
    HF.sphere_conv_bwd_data_t(gyt, pd, wd, gxt, groups)
    return gxt
  return run


def bwd_weight(case):
  """One call of HF.sphere_conv_bwd_weight_t adding to zeros; returns gw on the device."""
  from mode_hip import functional as HF
  from oracle import mode_ref
  ih, iw, B, ci, co, groups = case
  pos = mode_ref.sphere_position(ih, iw, 'Cassini').contiguous()
  H, W = pos.shape[2:]
  x = _rand((B, ci, H, W), 411)
  gy = _rand((B, co, H, W), 412)
  pd = pos.to(DEV)
  xt, gyt = x.to(DEV).transpose(2, 3).contiguous(), gy.to(DEV).transpose(2, 3).contiguous()

  def run():
    gw = torch.zeros((co, ci // groups, 3, 3), device=DEV)
    HF.sphere_conv_bwd_weight_t(gyt, pd, xt, gw, groups)
    return gw
  return run


def main():
  from mode_hip import functional as HF
  HF.set_conv_arith('bf16x6')
  out = {}
  for kind, make, cases in (('bwd_data', bwd_data, BWD_DATA), ('bwd_weight', bwd_weight, BWD_WEIGHT)):
    for case in cases:
      t = make(case)()
      torch.cuda.synchronize()
      assert torch.isfinite(t).all(), key(kind, case)
      out[key(kind, case)] = {'sha256': digest(t), 'shape': list(t.shape), 'dtype': 'float32'}
      print(key(kind, case), out[key(kind, case)]['sha256'])
  with open(sys.argv[1] if len(sys.argv) > 1 else OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main()
