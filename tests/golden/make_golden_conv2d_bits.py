#!/usr/bin/env python3
"""Output hashes of the regular 3x3 Conv2d operators, taken on the GPU at the commit BEFORE csrc/conv2d.hip was split into
conv2d_f32_fwd.hip (the fp32 forward kernels), conv2d_f32_wgrad.hip (the fp32 weight-gradient kernel and the reduction) and conv2d.hip
(the C entries of the family and their one argument check).

  python tests/golden/make_golden_conv2d_bits.py     # writes conv2d_parent_bits.json (needs the MI355X)

conv2d_parent_bits.json: SHA-256 of the raw bytes (fp32, C order) of what the operators of mode_hip.functional return for the cases
below.  The split moves kernels between files (tools/isa_same.py shows that no instruction changed) and writes the host code between
the entries and the launches once; that host code picks the tile, the split-K slices S and the rows per work unit run_groups, and S
and run_groups decide the order in which a weight gradient is summed.  So tests/test_gpu_conv2d_bits.py recomputes the outputs and
compares the hashes: one differing bit anywhere fails it.  Do not regenerate this file together with a change of a kernel or of a
launch -- it pins what the parent computed.

Cases (B, Ci, Co, H, W, dilation): x (B, Ci, H, W), w (Co, Ci, 3, 3).  kNumCU = 256.  Every case asserts its route
(HF._conv2d_route), so none can fall back to another family unnoticed.

Under set_conv_arith('f32') -- mode_conv2d_fwd / _bwd_data / _bwd_weight, the fp32 MFMA kernels.  conv2d_kernel<MT, TH, DIL[, EPI]>:
MT = cdiv(rows, 32) with rows = Co (forward) or Ci (input gradient), TH = 8 when big = B * cdiv(H, 8) * cdiv(W, 32) >= 2 * kNumCU = 512,
else 4.  conv2d_bwd_weight_kernel<DIL>: T = B * cdiv(H, 4) * cdiv(W, 32) tiles, S = min(cdiv(512, MTo * MTc), T) slices.
  A (2,  8,   8, 128, 512, 1)  big = 2 * 16 * 16 = 512 -> forward <1, 8, 1>, input gradient <1, 8, 1>; T = 2 * 32 * 16 = 1024, S = 512
  B (2, 20,  40,   7,  33, 1)  big = 4 -> forward (rows 40) <2, 4, 1>, input gradient (rows 20) <1, 4, 1>; T = 2 * 2 * 2 = 8 = S
                               (cdiv(512, 2) = 256 > T); a partial 8-channel chunk, a partial 32-channel tile, H and W no tile divides
  C (1, 72, 100,   9,  35, 2)  forward (rows 100) <4, 4, 2>, input gradient (rows 72) <3, 4, 2>; T = 3 * 2 = 6 = S (cdiv(512, 12) = 43),
                               masked 32 x 32 blocks on both channel axes
  D (2,  8,  40, 128, 512, 2)  forward <2, 8, 2>, input gradient <1, 8, 2>; T = 1024, S = cdiv(512, 2) = 256 < T
  eval (conv2d_bn_eval with add= and relu=True -> mode_conv2d_fwd_bn, the folded pack): B -> <2, 4, 1, true>, C -> <4, 4, 2, true>
  the stride-2 layer: Conv2d3x3S2Function on x (2, 8, 8, 16), w (16, 8, 3, 3): mode_zero_insert2 of gy (2, 16, 4, 8) feeds
  mode_conv2d_bwd_data (rows 8: <1, 4, 1>) and mode_conv2d_bwd_weight (T = 2 * 2 * 1 = 4 = S); gx and gw are hashed.

Under 'bf16x6', with CONV2D_F16 on (the *_split_f16 entries) and off (the *_split entries).  conv2d_split_kernel<MT, TH, DIL, EPI, F16>:
64 output channels per workgroup (MT = 2) in cdiv(rows, 32) / 2 y-slices of ONE launch, an odd 32-channel block at the end a launch
of its own (MT = 1, o0 = the channels before it); TH = 16 when big = B * cdiv(H, 16) * cdiv(W, 32) * (y-slices) >= 512, else 8.
conv2d_bww_split_kernel<DIL, F16>: nGroups = cdiv(H, 4) row groups; run_groups = nGroups, halved while above 4 and
B * cdiv(W, 32) * cdiv(nGroups, run_groups) < cdiv(256, MTo * MTc); units = B * cdiv(W, 32) * cdiv(nGroups, run_groups); S = the least
of cdiv(256, MTo * MTc), units and the fp32 grid's S.
  E (1,  32,  32,  10,  40, 1)  forward, input gradient, input gradient with acc=, weight gradient.  One 32-channel block: <1, 8, 1>
                                alone.  Weight gradient: nGroups = 3 = run_groups, units = 1 * 2 * 1 = 2, S = min(256, 2, 6) = 2
  F (1,  16,  96,  12,  40, 2)  forward: three 32-channel blocks -> <2, 8, 2> with one y-slice, then <1, 8, 2> with o0 = 64; input
                                gradient: K = 96 (six chunks), rows = 16 -> <1, 8, 2>; weight gradient: MTo = 3, nGroups = 3 =
                                run_groups, units = 2, S = min(cdiv(256, 3) = 86, 2, 6) = 2
  G (2,  16, 128, 128, 512, 1)  forward: two y-slices, big = 2 * 8 * 16 * 2 = 512 -> <2, 16, 1>; input gradient (rows 16): big = 256
                                -> <1, 8, 1>; weight gradient: nGroups = 32, cdiv(256, 4) = 64 wanted, 2 * 16 * 1 = 32 < 64 -> run_groups
                                = 16 (2 * 16 * 2 = 64: stop), units = 64 = S, below the 128 the workspace is sized for
  H (1, 256, 256,   8,  32, 1)  forward and input gradient: four 64-channel y-slices in one launch <2, 8, 1> (the fusion bottleneck)
  eval (conv2d_bn_eval, relu=True) on E and F, CONV2D_EVAL_F16 on (mode_conv2d_fwd_split_f16_bn, abs_max_folded_kernel + the folded
  fp16 pack) and off (mode_conv2d_fwd_split with an epilogue), each with add= (EPI 2) and without (EPI 1); with the switch on the
  maximum buffer the call leaves (HF.known_abs_max(y)) is hashed as well -- all MODE_BN_ABSMAX_FLOATS words of it: the first word
  alone is zero after this kernel (a workgroup leaves its maximum in slot 16 * (1 + block % 128), bn_internal.h), and which slots are
  filled is a property of the launch.

Reached: 9 of the 32 conv2d_kernel instantiations and 22 of the 48 conv2d_split_kernel ones.  Not reached, and left to the listing
comparison (tools/isa_same.py: their listings are the parent's):
  conv2d_kernel<MT, TH, DIL> plain: <3, 4, 1>, <4, 4, 1>, <1, 4, 2>, <2, 4, 2>, <2, 8, 1>, <3, 8, 1>, <4, 8, 1>, <3, 8, 2>, <4, 8, 2>; with the
  epilogue: every one but <2, 4, 1, true> and <4, 4, 2, true>;
  conv2d_split_kernel<MT, TH, DIL, EPI, F16>, for either F16: EPI 0 at <1, 16, 1>, <1, 16, 2>, <2, 16, 2>; EPI 1 and EPI 2 at <2, 8, 1> and at
  every 16-row tile -- a case of a fraction of a second reaches the tall tile only through many rows, and one of them is here.

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

OUT = os.path.join(HERE, 'conv2d_parent_bits.json')
DEV = 'cuda:0'

A, B_, C, D = (2, 8, 8, 128, 512, 1), (2, 20, 40, 7, 33, 1), (1, 72, 100, 9, 35, 2), (2, 8, 40, 128, 512, 2)
E, F, G_, H_ = (1, 32, 32, 10, 40, 1), (1, 16, 96, 12, 40, 2), (2, 16, 128, 128, 512, 1), (1, 256, 256, 8, 32, 1)
S2 = (2, 8, 16, 8, 16, 1)  # the stride-2 layer: x (2, 8, 8, 16), w (16, 8, 3, 3)

TRAIN = ('fwd', 'bwd_data', 'bwd_weight')
# (operator, arithmetic, CONV2D_F16 = CONV2D_EVAL_F16, shape)
CASES = ([(op, 'f32', True, s) for s in (A, B_, C, D) for op in TRAIN] +
         [('eval_add', 'f32', True, s) for s in (B_, C)] +
         [(op, 'f32', True, S2) for op in ('s2_gx', 's2_gw')] +
         [(op, 'bf16x6', f16, s) for f16 in (True, False) for s, ops in ((E, TRAIN + ('bwd_data_acc',)), (F, TRAIN), (G_, TRAIN),
                                                                         (H_, TRAIN[:2])) for op in ops] +
         [(op, 'bf16x6', f16, s) for f16 in (True, False) for s in (E, F) for op in ('eval', 'eval_add')] +
         [(op, 'bf16x6', True, s) for s in (E, F) for op in ('eval_amax', 'eval_add_amax')])


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def key(case):
  op, arith, f16, shape = case
  return '%s/%s_f16%d_B%d_%d->%d_%dx%d_d%d' % ((op, arith, int(f16)) + tuple(shape))


def digest(t):
  return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


SWITCHES = ('CONV_ARITH', 'CONV2D_F16', 'CONV2D_EVAL_F16')


def settings(case):
  """The module switches of functional.py a case runs under (the test sets the same three with monkeypatch)."""
  return dict(zip(SWITCHES, (case[1], case[2], case[2])))


class switches(object):
  """settings(case) for the length of a with block."""

  def __init__(self, case):
    self.want = settings(case)

  def __enter__(self):
    from mode_hip import functional as HF
    self.prev = {k: getattr(HF, k) for k in SWITCHES}
    for k, v in self.want.items():
      setattr(HF, k, v)

  def __exit__(self, *exc):
    from mode_hip import functional as HF
    for k, v in self.prev.items():
      setattr(HF, k, v)
    return False


def _bn(co):
  bn = torch.nn.BatchNorm2d(co).to(DEV).eval()
  with torch.no_grad():
    bn.weight.copy_(_rand((co,), 714).abs() + 0.5)
    bn.bias.copy_(_rand((co,), 715))
    bn.running_mean.copy_(_rand((co,), 716, 0.1))
    bn.running_var.copy_(_rand((co,), 717).abs() + 0.5)
  return bn


def make(case):
  """The inputs of `case` on the device and a function that calls its operator once (under the module switches as they stand) and
  returns the result."""
  from mode_hip import functional as HF
  op, arith, f16, (B, ci, co, H, W, dil) = case
  scale = (2.0 / (9 * ci))**0.5
  want = 'f32' if arith == 'f32' else 'split_f16' if f16 else 'split'

  def on_route(which, f16_arg, h=H, w=W):
    got = HF._conv2d_route(ci, co, h, w, dil, which, f16_arg)
    assert got == want, '%s: on the %s route, not %s' % (key(case), got, want)

  if op in ('s2_gx', 's2_gw'):
    x, w, gy = _rand((B, ci, H, W), 701).to(DEV), _rand((co, ci, 3, 3), 702, scale).to(DEV), _rand((B, co, H // 2, W // 2), 704).to(DEV)

    def run():
      on_route(1, HF._conv2d_f16(True))
      on_route(2, HF._conv2d_f16(True))
      xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
      HF.Conv2d3x3S2Function.apply(xr, wr).backward(gy)
      return xr.grad if op == 's2_gx' else wr.grad
    return run

  x, w = _rand((B, ci, H, W), 701).to(DEV), _rand((co, ci, 3, 3), 702, scale).to(DEV)
  gy = _rand((B, co, H, W), 704).to(DEV)
  if op == 'fwd':
    def run():
      on_route(0, HF._conv2d_f16(True))
      return HF.conv2d_fwd(x, w, dil, f16=True)
  elif op == 'bwd_data':
    def run():
      on_route(1, HF._conv2d_f16(True))
      return HF.conv2d_bwd_data(gy, w, dil)
  elif op == 'bwd_data_acc':
    acc = _rand((B, ci, H, W), 705).to(DEV)

    def run():
      on_route(1, HF._conv2d_f16(True))
      return HF.conv2d_bwd_data(gy, w, dil, acc=acc)
  elif op == 'bwd_weight':
    def run():
      on_route(2, HF._conv2d_f16(True))
      return HF.conv2d_bwd_weight(gy, x, dil)
  elif op in ('eval', 'eval_add', 'eval_amax', 'eval_add_amax'):
    bn, res = _bn(co), (_rand((B, co, H, W), 703).to(DEV) if 'add' in op else None)

    def run():
      on_route(0, HF.CONV2D_EVAL_F16)
      with torch.no_grad():
        y = HF.conv2d_bn_eval(x, w, bn, dil, add=res, relu=True)
      if not op.endswith('amax'):
        return y
      am = HF.known_abs_max(y)
      assert am is not None, '%s: the call left no maximum' % key(case)
      return am.clone()
  else:
    raise ValueError(op)
  return run


def main():
  out = {}
  for case in CASES:
    with switches(case):
      run = make(case)
      t = run()
      torch.cuda.synchronize()
      assert torch.isfinite(t).all(), key(case)
      assert torch.equal(run(), t), key(case)
    out[key(case)] = {'sha256': digest(t), 'shape': list(t.shape), 'dtype': 'float32'}
    print(key(case), out[key(case)]['sha256'], flush=True)
  assert len(out) == len(CASES)
  with open(sys.argv[1] if len(sys.argv) > 1 else OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')


if __name__ == '__main__':
  main()
