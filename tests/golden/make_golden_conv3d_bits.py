#!/usr/bin/env python3
"""Output hashes of the 3-D convolution operators, taken on the GPU at the commit BEFORE csrc/conv3d.hip was split into
conv3d_f32_fwd.hip (forward kernels), conv3d_f32_wgrad.hip (weight-gradient kernels) and conv3d.hip (the C entries of the family).

  python tests/golden/make_golden_conv3d_bits.py     # writes conv3d_parent_bits.json (needs the MI355X)

conv3d_parent_bits.json: SHA-256 of the raw bytes (fp32, C order) of what the operators of mode_hip.functional return for the cases
below.  The split moves the kernels between files (tools/isa_same.py shows that no instruction changed) and rewrites the host code
between the entries and the launches once instead of three times; that host code picks the tile, the split-K slices S and the depths
per work unit ring_dc, and S and ring_dc decide the order in which a weight gradient is summed.  So tests/test_gpu_conv3d_bits.py
recomputes the outputs and compares the hashes: one differing bit anywhere fails it.  Do not regenerate this file together with a
change of a kernel or of a launch -- it pins what the parent computed.

Cases (B, Ci, Co, D, H, W) = the convolution's input x (B, Ci, D, H, W) and Co output channels; for the transposed convolution x is
(B, Ci, D, H, W) and the output (B, Co, 2D, 2H, 2W).  kNumCU = 256, and a `tile` below is TD x TH rows of 32 output voxels.

Under set_conv_arith('f32') -- every entry runs the fp32 MFMA kernels:
  forward, stride 1 (conv3d_s1 picks the tile from big = B * cdiv(D, 2) * cdiv(H, 8) * cdiv(W, 32) and mid = the same with cdiv(H, 4),
  each against 2 * kNumCU = 512):
    (2,  8,  8, 16, 64, 128)   MT = 1, big = 2 * 8 * 8 * 4 = 512              -> conv3d_kernel<1, 2, 8, 1>
    (2,  8,  8, 16, 32, 128)   MT = 1, big = 256, mid = 2 * 8 * 8 * 4 = 512   -> conv3d_kernel<1, 2, 4, 1>
    (2, 20, 40,  5,  7,  33)   the input gradient (rows = 20): MT = 1, mid = 24 -> conv3d_kernel<1, 1, 4, 1>; the forward
                               (rows = 40): MT = 2 -> <2, 1, 4, 1>; three 8-channel chunks with the last one partial, a partial
                               32-channel tile, and D, H, W that no tile size divides
    (2,  8, 40, 16, 32, 128)   forward: MT = 2, mid = 512 -> conv3d_kernel<2, 2, 4, 1>; input gradient: rows = 8 -> <1, 2, 4, 1>
    input gradient of each: the same kernels with the weights packed transposed and flipped (flip = 1)
    weight gradient of each: a sample has far fewer than 2^29 elements -> conv3d_bwd_weight_ring_kernel; S (512 / (MTo * MTc), at
    most the work units) and ring_dc (D, halved while it is above 6 and there are fewer than 2 S units) differ between the four
  forward, stride 2:          (2, 8, 16, 8, 8, 8) -> conv3d_kernel<1, 1, 4, 2>;   (1, 32, 64, 4, 8, 64) -> <2, 1, 4, 2>
  weight gradient, stride 2:  (2, 8, 16, 8, 8, 8): MTo = 1 -> conv3d_bwd_weight_s2_kernel<1>;   (1, 32, 64, 4, 8, 64): MTo = 2 -> <2>
  transposed convolution:     (2, 24, 40, 2, 5, 35) -> deconv3d_kernel<2, 2, false>, two output-channel tiles (grid y), the second partial
  one output channel:         (1, 20, 1, 3, 5, 33) -> the Co = 1 dispatch of mode_conv3d_fwd / _bwd_data / _bwd_weight (the kernels are
                              in csrc/conv3d_c1.hip and did not move; the dispatch did)
  eval (conv3d_bn_eval / deconv3d_bn_eval with a residual and ReLU: the EPI = true instantiations and the folded pack):
    stride 1 (2, 20, 40, 5, 7, 33) -> conv3d_kernel<2, 1, 4, 1, true>;  stride 2 (2, 8, 16, 8, 8, 8) -> <1, 1, 4, 2, true>;
    transposed (2, 24, 40, 2, 5, 35) -> deconv3d_kernel<2, 2, true>

Under the default 'bf16x6' -- the entries whose kernels live in the conv3d_split*.hip files, whose argument check, split-K partition
and reduction are host code of conv3d.hip:
  (1, 32, 32, 6, 10, 40), CONV3D_S1_F16 on:  mode_conv3d_fwd_split_f16, _bwd_data_split_f16, _bwd_weight_split_f16
  the same, CONV3D_S1_F16 off:               mode_conv3d_fwd_split, _bwd_data_split, _bwd_weight_split
  the same with acc= (both settings):        mode_conv3d_bwd_data_split_f16 with acc / mode_conv3d_bwd_data_split_acc
  (1, 32, 64, 4, 8, 64) stride 2:            mode_conv3d_fwd_s2_split, mode_conv3d_bwd_weight_s2_split
  (1, 64, 32, 6, 16, 32) transposed:         mode_deconv3d_fwd_split
Each of these asserts that the shape is on the split path (HF._split3d), so a case cannot fall back to the fp32 entry unnoticed.

Not reached: conv3d_bwd_weight_kernel<S, WTH>, the fallback for samples of 2^29 elements and more.  Nothing that runs in seconds
gets there; the listing comparison alone covers it.

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

OUT = os.path.join(HERE, 'conv3d_parent_bits.json')
DEV = 'cuda:0'

S1_F32 = [(2, 8, 8, 16, 64, 128), (2, 8, 8, 16, 32, 128), (2, 20, 40, 5, 7, 33), (2, 8, 40, 16, 32, 128)]
S2_F32 = [(2, 8, 16, 8, 8, 8), (1, 32, 64, 4, 8, 64)]
DECONV_F32 = (2, 24, 40, 2, 5, 35)
CO1 = (1, 20, 1, 3, 5, 33)
S1_SPLIT = (1, 32, 32, 6, 10, 40)
S2_SPLIT = (1, 32, 64, 4, 8, 64)
DECONV_SPLIT = (1, 64, 32, 6, 16, 32)

# (operator, arithmetic, CONV3D_S1_F16, stride, shape)
CASES = ([(op, 'f32', True, 1, s) for s in S1_F32 + [CO1] for op in ('fwd', 'bwd_data', 'bwd_weight')] +
         [(op, 'f32', True, 2, s) for s in S2_F32 for op in ('fwd', 'bwd_weight')] +
         [('deconv', 'f32', True, 2, DECONV_F32)] +
         [('eval', 'f32', True, 1, S1_F32[2]), ('eval', 'f32', True, 2, S2_F32[0]), ('deconv_eval', 'f32', True, 2, DECONV_F32)] +
         [(op, 'bf16x6', f16, 1, S1_SPLIT) for f16 in (True, False) for op in ('fwd', 'bwd_data', 'bwd_weight', 'bwd_data_acc')] +
         [(op, 'bf16x6', True, 2, S2_SPLIT) for op in ('fwd', 'bwd_weight')] +
         [('deconv', 'bf16x6', True, 2, DECONV_SPLIT)])


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def key(case):
  op, arith, f16, stride, shape = case
  return '%s/%s_f16%d_s%d_B%d_%d->%d_%dx%dx%d' % ((op, arith, int(f16), stride) + tuple(shape))


def digest(t):
  return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class switches(object):
  """The arithmetic and CONV3D_S1_F16 of one case, restored on exit (the test sets the same two with monkeypatch)."""

  def __init__(self, arith, f16):
    self.arith, self.f16 = arith, f16

  def __enter__(self):
    from mode_hip import functional as HF
    self.prev = (HF.CONV_ARITH, HF.CONV3D_S1_F16)
    HF.set_conv_arith(self.arith)
    HF.CONV3D_S1_F16 = self.f16

  def __exit__(self, *exc):
    from mode_hip import functional as HF
    HF.set_conv_arith(self.prev[0])
    HF.CONV3D_S1_F16 = self.prev[1]
    return False


def _bn(co):
  bn = torch.nn.BatchNorm3d(co).to(DEV).eval()
  with torch.no_grad():
    bn.weight.copy_(_rand((co,), 614).abs() + 0.5)
    bn.bias.copy_(_rand((co,), 615))
    bn.running_mean.copy_(_rand((co,), 616, 0.1))
    bn.running_var.copy_(_rand((co,), 617).abs() + 0.5)
  return bn


def make(case):
  """The inputs of `case` on the device and a function that calls its operator once (under the module switches as they stand) and
  returns the result."""
  from mode_hip import functional as HF
  op, arith, f16, stride, (B, ci, co, D, H, W) = case
  o = lambda n: (n - 1) // stride + 1
  scale = (2.0 / (27 * ci))**0.5
  split = arith == 'bf16x6'

  def on_split(which, vol=(D, H, W), cc=(ci, co)):
    assert HF._split3d(cc[0], cc[1], stride, which, vol) == split, '%s: not on the %s path' % (key(case), arith)

  if op in ('deconv', 'deconv_eval'):
    x, w = _rand((B, ci, D, H, W), 601).to(DEV), _rand((ci, co, 3, 3, 3), 602, scale).to(DEV)
    if op == 'deconv':
      def run():
        on_split(1, (2 * D, 2 * H, 2 * W), (co, ci))
        return HF.deconv3d_fwd(x, w)
      return run
    bn, res = _bn(co), _rand((B, co, 2 * D, 2 * H, 2 * W), 603).to(DEV)

    def run():
      with torch.no_grad():
        return HF.deconv3d_bn_eval(x, w, bn, add=res, relu=True)
    return run

  x, w = _rand((B, ci, D, H, W), 601).to(DEV), _rand((co, ci, 3, 3, 3), 602, scale).to(DEV)
  gy = _rand((B, co, o(D), o(H), o(W)), 604).to(DEV)
  if op == 'fwd':
    def run():
      on_split(0)
      return HF.conv3d_fwd(x, w, stride)
  elif op == 'bwd_data':
    def run():
      on_split(1)
      return HF.conv3d_bwd_data(gy, w, x.shape, stride)
  elif op == 'bwd_data_acc':
    acc = _rand((B, ci, D, H, W), 605).to(DEV)

    def run():
      on_split(1)
      assert HF.lib().mode_conv3d_bwd_data_split_acc_supported(ci, co, stride) == 1
      return HF.conv3d_bwd_data(gy, w, x.shape, stride, acc=acc)
  elif op == 'bwd_weight':
    def run():
      on_split(2)
      return HF.conv3d_bwd_weight(gy, x, stride)
  elif op == 'eval':
    bn, res = _bn(co), _rand(tuple(gy.shape), 603).to(DEV)

    def run():
      with torch.no_grad():
        return HF.conv3d_bn_eval(x, w, bn, stride, add=res, relu=True)
  else:
    raise ValueError(op)
  return run


def main():
  out = {}
  for case in CASES:
    with switches(case[1], case[2]):
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
