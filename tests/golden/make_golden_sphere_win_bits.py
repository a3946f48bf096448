#!/usr/bin/env python3
"""Output hashes of the windowed spherical operators, taken on the GPU at the commit BEFORE csrc/sphere_conv_win.hip was split into one
file per pass.

  python tests/golden/make_golden_sphere_win_bits.py     # writes sphere_win_parent_bits.json (needs the MI355X)

sphere_win_parent_bits.json: SHA-256 of the raw bytes (fp32, C order) of what the plane-transposed operators write for the cases below:
the forward (HF.sphere_conv_fwd_t), the folded-BatchNorm eval forward (HF.sphere_conv_bn_eval, transposed=True), the input gradient
(HF.sphere_conv_bwd_data_t) and the weight gradient (HF.sphere_conv_bwd_weight_t).  The split moves code between files and must not
change one instruction, so tests/test_gpu_sphere_win_bits.py recomputes the outputs and compares the hashes: one differing bit
anywhere fails it.  Do not regenerate this file together with a kernel change -- it pins what the parent computed.

The table is sphere_position(128, 256, 'Cassini'), the smallest with compact, mid and wrap tiles, polar items and six-source adjoint
tiles all present (tests/test_sphere_win_bits_plan.py checks that on the host).  The (32, 64) table (stored 64 x 32) serves the input
gradient alone: on three bf16 pieces its adjoint plan has 8 good tiles, three of them six-source, and none left to the gather kernel, so
the whole result comes from sphere_bwd_data_split_kernel at W = 32 -- which the large table, with its 64 left-over tile ids, never
shows.  On two fp16 pieces tile (0, 0), whose adjoint lists weigh more than that form's headroom, is left to the gather kernel (7 good
tiles, two of them six-source): the hash of that one case was taken again with this recipe when the planner learned the headroom, and
the result outside tile (0, 0) kept its bits.  Its forward
plan is (0, 8, 0) with no polar items: without compact tiles the model keeps such a table off the windowed forward and weight gradient
(HF._plan_usable), so it has no case there.  HF.SPHERE_BWD_SPLIT_MIN_WG is 0 for the duration of an input-gradient case: the default
sends problems this small to the gather kernel.

Inputs: the seeded CPU generator of tests/test_gpu_split.py (`_rand`, restated here so that the fixture does not depend on a test
module)."""
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

OUT = os.path.join(HERE, 'sphere_win_parent_bits.json')
DEV = 'cuda:0'
TABLE = (128, 256)
SMALL_TABLE = (32, 64)  # input gradient only

# forward: (ih, iw, B, ci, co, groups, arith, f16)
FWD = [(128, 256, 2, 32, 40, 1, 'bf16x6', False),   # two 16-channel chunks: the window hand-over; Co = 40: the partial M-tile store
       (128, 256, 2, 32, 40, 1, 'bf16x6', True),    # the two-piece fp16 arithmetic of a training forward
       (128, 256, 1, 40, 24, 1, 'bf16x6', False),   # Cig % 16 != 0: the fp32 windowed kernels
       (128, 256, 1, 32, 32, 2, 'bf16x6', False)]
# eval epilogue: (ih, iw, B, ci, co, groups, arith, relu, add)
EVAL = [(128, 256, 1, 32, 40, 1, 'bf16x6', relu, add) for relu in (False, True) for add in (False, True)]
# input gradient: (ih, iw, B, ci, co, groups, arith, f16)
BWD_DATA = ([(128, 256, 2, ci, co, 1, 'bf16x6', f16) for (ci, co) in ((32, 32), (64, 48)) for f16 in (True, False)] +
            [(32, 64, 2, 32, 32, 1, 'bf16x6', f16) for f16 in (True, False)])
# weight gradient: (ih, iw, B, ci, co, groups, arith, f16)
BWD_WEIGHT = [(128, 256, 2, 32, 40, 1, 'bf16x6', True), (128, 256, 2, 32, 40, 1, 'bf16x6', False),
              (128, 256, 1, 40, 24, 1, 'bf16x6', True), (128, 256, 1, 40, 24, 1, 'bf16x6', False),
              (128, 256, 2, 32, 40, 1, 'f32', False), (128, 256, 1, 40, 24, 1, 'f32', False)]


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def key(kind, case):
  return '%s/%dx%d_B%d_%d->%d_g%d_%s_%s' % ((kind,) + tuple(case[:7]) + ('_'.join(str(int(v)) for v in case[7:]),))


def digest(t):
  return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class switches(object):
  """The arithmetic and the module switches of one case, restored on exit."""

  def __init__(self, arith, **flags):
    self.arith, self.flags = arith, flags

  def __enter__(self):
    from mode_hip import functional as HF
    self.prev = (HF.CONV_ARITH, {k: getattr(HF, k) for k in self.flags})
    HF.set_conv_arith(self.arith)
    for k, v in self.flags.items():
      setattr(HF, k, v)

  def __exit__(self, *exc):
    from mode_hip import functional as HF
    HF.set_conv_arith(self.prev[0])
    for k, v in self.prev[1].items():
      setattr(HF, k, v)
    return False


def _table(ih, iw):
  from oracle import mode_ref
  return mode_ref.sphere_position(ih, iw, 'Cassini').contiguous()


def _t(x):
  return x.to(DEV).transpose(2, 3).contiguous()


def fwd(case):
  """One call of HF.sphere_conv_fwd_t on NaN-filled storage (the operator writes every element); returns yt on the device."""
  from mode_hip import functional as HF
  ih, iw, B, ci, co, groups, arith, f16 = case
  pos = _table(ih, iw)
  H, W = pos.shape[2:]
  w = _rand((co, ci // groups, 3, 3), 501, (2.0 / (9 * ci // groups))**0.5).to(DEV)
  xt, pd = _t(_rand((B, ci, H, W), 502)), pos.to(DEV)

  def run():
    yt = torch.full((B, co, W, H), float('nan'), device=DEV)
    with switches(arith):
      ran = []
      HF.sphere_conv_fwd_t(xt, pd, w, yt, groups, f16=f16, amax_out=ran)
      assert bool(ran) == bool(f16 and ci // groups % 16 == 0), 'the fp16 arithmetic ran: %s' % bool(ran)
    return yt
  return run


def eval_bn(case):
  """One call of HF.sphere_conv_bn_eval(transposed=True) (the operator allocates its result); returns it."""
  from mode_hip import functional as HF
  ih, iw, B, ci, co, groups, arith, relu, add = case
  pos = _table(ih, iw)
  H, W = pos.shape[2:]
  w = _rand((co, ci // groups, 3, 3), 511, (2.0 / (9 * ci // groups))**0.5).to(DEV)
  xt, pd = _t(_rand((B, ci, H, W), 512)), pos.to(DEV)
  res = _t(_rand((B, co, H, W), 513)) if add else None
  bn = torch.nn.BatchNorm2d(co).to(DEV).eval()
  with torch.no_grad():
    bn.weight.copy_(_rand((co,), 514).abs() + 0.5)
    bn.bias.copy_(_rand((co,), 515))
    bn.running_mean.copy_(_rand((co,), 516, 0.1))
    bn.running_var.copy_(_rand((co,), 517).abs() + 0.5)

  def run():
    with switches(arith), torch.no_grad():
      return HF.sphere_conv_bn_eval(xt, pd, w, bn, (1, 1), groups, add=res, relu=relu, transposed=True)
  return run


def bwd_data(case):
  """One call of HF.sphere_conv_bwd_data_t on NaN-filled storage; returns gxt on the device."""
  from mode_hip import functional as HF
  ih, iw, B, ci, co, groups, arith, f16 = case
  pos = _table(ih, iw)
  H, W = pos.shape[2:]
  w = _rand((co, ci // groups, 3, 3), 521, (2.0 / (9 * ci // groups))**0.5).to(DEV)
  gyt, pd = _t(_rand((B, co, H, W), 522)), pos.to(DEV)

  def run():
    gxt = torch.full((B, ci, W, H), float('nan'), device=DEV)
    with switches(arith, SPHERE_BWD_SPLIT_MIN_WG=0, SPHERE_BWD_F16=f16):
      assert HF.sphere_adjplan(pd, 3, 3) is not None and HF.lib().mode_sphere_conv_bwd_data_win_supported(ci, co, groups) == 1
      HF.sphere_conv_bwd_data_t(gyt, pd, w, gxt, groups)
    return gxt
  return run


def bwd_weight(case):
  """One call of HF.sphere_conv_bwd_weight_t adding to zeros; returns gw on the device."""
  from mode_hip import functional as HF
  ih, iw, B, ci, co, groups, arith, f16 = case
  pos = _table(ih, iw)
  H, W = pos.shape[2:]
  xt, gyt, pd = _t(_rand((B, ci, H, W), 531)), _t(_rand((B, co, H, W), 532)), pos.to(DEV)

  def run():
    gw = torch.zeros((co, ci // groups, 3, 3), device=DEV)
    with switches(arith, SPHERE_BWD_F16=f16):
      HF.sphere_conv_bwd_weight_t(gyt, pd, xt, gw, groups)
    return gw
  return run


KINDS = (('fwd', fwd, FWD), ('eval', eval_bn, EVAL), ('bwd_data', bwd_data, BWD_DATA), ('bwd_weight', bwd_weight, BWD_WEIGHT))


def main():
  out = {}
  for kind, make, cases in KINDS:
    for case in cases:
      run = make(case)
      t = run()
      torch.cuda.synchronize()
      assert torch.isfinite(t).all(), key(kind, case)
      assert torch.equal(run(), t), key(kind, case)
      out[key(kind, case)] = {'sha256': digest(t), 'shape': list(t.shape), 'dtype': 'float32'}
      print(key(kind, case), out[key(kind, case)]['sha256'], flush=True)
  with open(sys.argv[1] if len(sys.argv) > 1 else OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main()
