"""GPU (-m gpu): both sides of the size limits of the split-operand kernels (csrc/size_contracts.h), through the public
`functional` operators: the last shape inside a limit runs on the split entry and is right, the first shape beyond it runs on another
entry -- the fp32 kernels -- and is right too.  Which entry ran is read from a recording stand-in for the ctypes handle.

Every case has B = 1 and device-generated inputs (a seeded device generator; a 2 GiB host array takes longer than a test may).  The
references are float64 on the CPU over SLABS only: a few planes (rows) of the operands, cut with their true neighbours and with zeros
beyond the volume's faces, and a plain tap-by-tap evaluation of the convolution on them.  For the weight gradients the output
gradient is non-zero on a few slabs only, so that the exact gradient IS the sum over those slabs -- the kernels still walk every
offset of the tensors, and the last slab reads the highest ones.  What a broken limit would do there: garbage in place of the zero
padding along the borders of those planes is several thousand wrong products of order one against a bound of ~0.01, and a wrapped
descriptor returns exactly zero.

Bounds are those of each operator's existing test (tests/test_gpu_split.py `_tol`, 2e-5 of the largest weight gradient;
tests/test_gpu_f16.py for the fp16 arithmetic), not tuned to this run; the errors are printed beside them.  No case launches a split
kernel beyond its limit, and nothing here runs the library of before the limits were enforced.

Three cheap boundaries of the same kind ride along: the BatchNorm grid limit, the statistics epilogue's, and the LDS limit of the
folded cost-volume convolution -- dispatcher limits with a fallback whose two sides nothing else tests."""
import collections
import time

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import mode_ref

import mode_hip
from mode_hip import functional as HF
from models import stage3d

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PEAK = {'bytes': 0}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  mode_hip.lib()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  yield
  torch.cuda.empty_cache()
  print('test_gpu_size_contracts: peak device memory %.2f GiB' % (PEAK['bytes'] / 2.0**30))


@pytest.fixture(autouse=True)
def _free_between_cases():
  keep = (HF.CONV_ARITH, HF.CONV3D_S1_F16, HF.CONV2D_F16, HF.CONV3D_EVAL_F16, HF.CONV3D_BN_STATS)
  t0 = time.time()
  yield
  HF.set_conv_arith(keep[0])
  HF.CONV3D_S1_F16, HF.CONV2D_F16, HF.CONV3D_EVAL_F16, HF.CONV3D_BN_STATS = keep[1:]
  torch.cuda.synchronize()
  PEAK['bytes'] = max(PEAK['bytes'], torch.cuda.max_memory_allocated())
  torch.cuda.empty_cache()
  print('case took %.2f s, peak so far %.2f GiB' % (time.time() - t0, PEAK['bytes'] / 2.0**30))


class RecordingLib(object):
  """Stands in for the ctypes handle (as test_gpu_repeat.PoisoningLib): the names of the launching entries, in call order, and of
  mode_weight_pack_reuse, which launches nothing but tells a packed-weight cache hit (test_gpu_eval_precision reads it here)."""
  RECORDED = (mode_hip.LAUNCHING | {'mode_weight_pack_reuse'}) - {'mode_debug_poison'}

  def __init__(self, real):
    self._real, self.names = real, []

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in self.RECORDED:
      return fn

    def call(*args):
      self.names.append(name)
      return fn(*args)

    return call


@pytest.fixture
def recorder(monkeypatch):
  real = mode_hip.lib()
  proxy = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', proxy)
  yield proxy
  monkeypatch.setattr(mode_hip, '_lib', real)


def _ran(recorder, prefix):
  """The entries of family `prefix` that ran since the last look (maximum passes and the like left out)."""
  names = [n for n in recorder.names if n.startswith(prefix)]
  del recorder.names[:]
  return names


def _randn(shape, seed, scale=1.0):
  g = torch.Generator(device=DEV).manual_seed(seed)
  t = torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)
  return t.mul_(scale) if scale != 1.0 else t


def _tol(terms, want):  # tests/test_gpu_split.py
  return 2.0**-22 * np.sqrt(terms) * 8 * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ float64 references over slabs
def _planes64(t, planes):
  """(C, len(planes), H, W) float64 on the CPU: the depth planes `planes` of the device tensor t (1, C, D, H, W), zeros for a plane
  outside the volume."""
  C, D, H, W = t.shape[1:]
  out = torch.zeros((C, len(planes), H, W), dtype=torch.float64)
  for i, z in enumerate(planes):
    if 0 <= z < D:
      out[:, i] = t[0, :, z].cpu().double()
  return out


def _conv3_planes64(x, w64, a, b):
  """Output planes a..b (inclusive) of conv3d(x, w, stride 1, padding 1), all channels and whole planes, from the input planes
  a - 1 .. b + 1 alone: (Co, b - a + 1, H, W) float64."""
  n = b - a + 1
  slab = F.pad(_planes64(x, list(range(a - 1, b + 2))), (1, 1, 1, 1))
  H, W = x.shape[3:]
  out = torch.zeros((w64.shape[0], n, H, W), dtype=torch.float64)
  for kd in range(3):
    for kh in range(3):
      for kw in range(3):
        out += torch.einsum('oc,cdhw->odhw', w64[:, :, kd, kh, kw], slab[:, kd:kd + n, kh:kh + H, kw:kw + W])
  return out


def _flipped(w64):
  """The input gradient of a stride-1 convolution is the convolution of gy with the weight transposed and reversed."""
  return w64.transpose(0, 1).flip(2, 3, 4).contiguous()


def _wgrad3_planes64(gy, x, planes):
  """The weight gradient (Co, Ci, 3, 3, 3) for a gy that is non-zero on depth planes `planes` only: the sum over those planes."""
  Co, Ci = gy.shape[1], x.shape[1]
  H, W = x.shape[3:]
  gw = torch.zeros((Co, Ci, 3, 3, 3), dtype=torch.float64)
  for p in planes:
    g = _planes64(gy, [p])[:, 0].reshape(Co, H * W)
    slab = F.pad(_planes64(x, [p - 1, p, p + 1]), (1, 1, 1, 1))
    for kd in range(3):
      for kh in range(3):
        for kw in range(3):
          gw[:, :, kd, kh, kw] += g @ slab[:, kd, kh:kh + H, kw:kw + W].reshape(Ci, H * W).t()
  return gw


def _wgrad2_rows64(gy, x, groups, dil):
  """The 3 x 3 weight gradient (padding = dilation) for a gy (1, Co, H, W) that is non-zero on the row ranges `groups` only."""
  Co, Ci = gy.shape[1], x.shape[1]
  H, W = x.shape[2:]
  gw = torch.zeros((Co, Ci, 3, 3), dtype=torch.float64)
  for r0, r1 in groups:  # rows r0 .. r1 - 1
    n = r1 - r0
    g = gy[0, :, r0:r1].cpu().double().reshape(Co, n * W)
    rows = torch.zeros((Ci, n + 2 * dil, W), dtype=torch.float64)
    lo, hi = max(r0 - dil, 0), min(r1 + dil, H)
    rows[:, lo - (r0 - dil):hi - (r0 - dil)] = x[0, :, lo:hi].cpu().double()
    rows = F.pad(rows, (dil, dil))
    for kh in range(3):
      for kw in range(3):
        gw[:, :, kh, kw] += g @ rows[:, kh * dil:kh * dil + n, kw * dil:kw * dil + W].reshape(Ci, n * W).t()
  return gw


def _err(got, want):
  return float((got.detach().cpu().double() - want).abs().max())


# ------------------------------------------------------------------------------------------------ stride-1 3-D: forward, input gradient
S1_SHAPES = {'inside': (1023, 128, 512), 'beyond': (1024, 128, 512)}  # 32 * DHW = 2^31 - 2^23 | 2^31


def _plane_pairs(D):
  return [(0, 1), (511, 512), (D - 2, D - 1)]


@pytest.mark.parametrize('side', ['inside', 'beyond'])
def test_conv3d_forward_and_input_gradient_on_both_sides_of_the_descriptor_limit(side, recorder):
  """conv3d_fwd, conv3d_bwd_data (plain and acc=) at 8 -> 8: 1023 x 128 x 512 is the last volume of this plane size whose 8 channel
  planes are a descriptor below 2^31 bytes, 1024 x 128 x 512 puts the descriptor's end ON the sentinel offset.  Output depth planes
  {0, 1}, {511, 512}, {D - 2, D - 1}, whole planes and all channels, in both settings of CONV3D_S1_F16."""
  D, H, W = S1_SHAPES[side]
  Ci = Co = 8
  assert mode_hip.lib().mode_conv3d_split_shape_supported(Ci, Co, D, H, W, 1, 0) == (1 if side == 'inside' else 0)
  assert mode_hip.lib().mode_conv3d_split_shape_supported(Ci, Co, D, H, W, 1, 1) == (1 if side == 'inside' else 0)
  w = _randn((Co, Ci, 3, 3, 3), 1102, (2.0 / (27 * Co))**0.5)
  w64 = w.cpu().double()
  x = _randn((1, Ci, D, H, W), 1101)  # (also the output gradient of the input-gradient half: Ci == Co)
  pairs = _plane_pairs(D)
  want_y = [_conv3_planes64(x, w64, a, b) for a, b in pairs]
  want_gx = [_conv3_planes64(x, _flipped(w64), a, b) for a, b in pairs]
  for f16 in (True, False):
    HF.CONV3D_S1_F16 = f16
    sfx = '_f16' if f16 else ''
    # forward
    del recorder.names[:]
    y = HF.conv3d_fwd(x, w, 1)
    assert _ran(recorder, 'mode_conv3d_fwd') == (['mode_conv3d_fwd_split' + sfx] if side == 'inside' else ['mode_conv3d_fwd']), side
    for (a, b), want in zip(pairs, want_y):
      e = _err(y[0, :, a:b + 1], want)
      bound = 2.0**-22 * (Ci * 27)**0.5 * float(want.abs().max()) if (f16 and side == 'inside') else _tol(Ci * 27, want)
      print('conv3d_fwd %s f16 %d planes %d..%d: error %.3e, bound %.3e' % (side, f16, a, b, e, bound))
      assert e <= bound, (side, f16, a, b, e, bound)
    del y
    # input gradient, plain and with a gradient that is already there
    gx = HF.conv3d_bwd_data(x, w, (1, Ci, D, H, W), 1)
    assert _ran(recorder, 'mode_conv3d_bwd_data') == (['mode_conv3d_bwd_data_split' + sfx] if side == 'inside' else ['mode_conv3d_bwd_data']), side
    acc = _randn((1, Ci, D, H, W), 1103)
    gxa = HF.conv3d_bwd_data(x, w, (1, Ci, D, H, W), 1, acc=acc)
    ran = _ran(recorder, 'mode_conv3d_bwd_data')
    assert ran == (['mode_conv3d_bwd_data_split' + (sfx if f16 else '_acc')] if side == 'inside' else ['mode_conv3d_bwd_data']), (side, ran)
    for (a, b), want in zip(pairs, want_gx):
      e = _err(gx[0, :, a:b + 1], want)
      want_acc = want + acc[0, :, a:b + 1].cpu().double()
      ea = _err(gxa[0, :, a:b + 1], want_acc)
      if f16 and side == 'inside':
        bound, bound_a = 2.0**-22 * (Co * 27)**0.5 * float(want.abs().max()), 2.0**-22 * (Co * 27)**0.5 * float(want_acc.abs().max())
      else:
        bound, bound_a = _tol(Co * 27, want), _tol(Co * 27, want_acc)
      print('conv3d_bwd_data %s f16 %d planes %d..%d: error %.3e, bound %.3e; with acc %.3e, bound %.3e' % (side, f16, a, b, e, bound, ea, bound_a))
      assert e <= bound and ea <= bound_a, (side, f16, a, b, e, bound, ea, bound_a)
    del gx, gxa, acc


@pytest.mark.parametrize('side', ['inside', 'beyond'])
def test_conv3d_bn_eval_on_both_sides_of_the_descriptor_limit(side, recorder):
  """conv3d_bn_eval with ReLU and a residual at the same shapes: the eval epilogues ride on the same staging."""
  D, H, W = S1_SHAPES[side]
  Ci = Co = 8
  w = _randn((Co, Ci, 3, 3, 3), 1112, (2.0 / (27 * Co))**0.5)
  x = _randn((1, Ci, D, H, W), 1111)
  add = _randn((1, Co, D, H, W), 1113)
  bn = nn.BatchNorm3d(Co).to(DEV).eval()
  r = np.random.RandomState(1114)
  with torch.no_grad():
    bn.weight.copy_(torch.from_numpy(r.uniform(0.5, 1.5, Co).astype(np.float32)))
    bn.bias.copy_(torch.from_numpy(r.standard_normal(Co).astype(np.float32) * 0.3))
    bn.running_mean.copy_(torch.from_numpy(r.standard_normal(Co).astype(np.float32) * 0.5))
    bn.running_var.copy_(torch.from_numpy(r.uniform(0.3, 2.0, Co).astype(np.float32)))
  w64 = w.cpu().double()
  scale64 = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu().view(Co, 1, 1, 1)
  shift64 = bn.bias.double().cpu().view(Co, 1, 1, 1) - bn.running_mean.double().cpu().view(Co, 1, 1, 1) * scale64
  del recorder.names[:]
  with torch.no_grad():
    y = HF.conv3d_bn_eval(x, w, bn, 1, add, True)
  f16 = HF.CONV3D_EVAL_F16
  ran = _ran(recorder, 'mode_conv3d_fwd')
  assert ran == (['mode_conv3d_fwd_split' + ('_f16_bn' if f16 else '')] if side == 'inside' else ['mode_conv3d_fwd_bn']), (side, ran)
  for a, b in _plane_pairs(D):
    pre = _conv3_planes64(x, w64, a, b) * scale64 + shift64 + add[0, :, a:b + 1].cpu().double()
    want = torch.relu(pre)
    e = _err(y[0, :, a:b + 1], want)
    # tests/test_gpu_f16.py::test_eval_epilogues_on_two_fp16_pieces for the fp16 epilogue; `_tol` for the others
    bound = 2.0**-22 * (27 * max(Ci, Co))**0.5 * 0.5 * float(pre.abs().max()) if (f16 and side == 'inside') else _tol(Ci * 27, pre)
    print('conv3d_bn_eval %s planes %d..%d: error %.3e, bound %.3e' % (side, a, b, e, bound))
    assert e <= bound, (side, a, b, e, bound)


# ------------------------------------------------------------------------------------------------ stride-1 3-D: weight gradient
WG3_SHAPES = {'inside': (255, 128, 512), 'beyond': (256, 128, 512)}  # 128 * DHW = 2^31 - 2^23 | 2^31


@pytest.mark.parametrize('side', ['inside', 'beyond'])
def test_conv3d_weight_gradient_on_both_sides_of_the_block_limit(side, recorder):
  """conv3d_bwd_weight at 16 -> 16: the kernel's descriptor is 32 channel planes whatever the channel count, so a 16-channel layer
  reaches its limit at a sample of 2^28 elements, where the old sample test (< 2^29) still said yes.  gy is non-zero on depth planes
  {0, 1, 127, D - 2, D - 1}, x random everywhere; the whole gradient is compared, with and without `into=`, in both settings of
  CONV3D_S1_F16.  (~5 x 128 x 512 unit-variance terms: magnitude ~600, bound ~0.01.)"""
  D, H, W = WG3_SHAPES[side]
  C = 16
  assert mode_hip.lib().mode_conv3d_split_shape_supported(C, C, D, H, W, 1, 2) == (1 if side == 'inside' else 0)
  planes = [0, 1, 127, D - 2, D - 1]
  x = _randn((1, C, D, H, W), 1121)
  gy = torch.zeros((1, C, D, H, W), dtype=torch.float32, device=DEV)
  for i, p in enumerate(planes):
    gy[0, :, p] = _randn((C, H, W), 1122 + i)
  want = _wgrad3_planes64(gy, x, planes)
  scale = max(1.0, float(want.abs().max()))
  for f16 in (True, False):
    HF.CONV3D_S1_F16 = f16
    entry = 'mode_conv3d_bwd_weight' + (('_split_f16' if f16 else '_split') if side == 'inside' else '')
    del recorder.names[:]
    got = HF.conv3d_bwd_weight(gy, x, 1)
    assert _ran(recorder, 'mode_conv3d_bwd_weight') == [entry], side
    into = torch.ones((C, C, 3, 3, 3), dtype=torch.float32, device=DEV)
    HF.conv3d_bwd_weight(gy, x, 1, into=into)
    assert _ran(recorder, 'mode_conv3d_bwd_weight') == [entry], side
    # fp16 arithmetic: tests/test_gpu_f16.py (terms = the positions summed per element, x.numel() // ci)
    bound = 2.0**-22 * float(D * H * W)**0.5 * 0.2 * float(want.abs().max()) if (f16 and side == 'inside') else 2e-5 * scale
    e, ei = _err(got, want), _err(into, want + 1.0)
    print('conv3d_bwd_weight %s f16 %d: error %.3e, into= %.3e, bound %.3e (max |want| %.4g)' % (side, f16, e, ei, bound, float(want.abs().max())))
    assert e <= bound and ei <= bound, (side, f16, e, ei, bound)
    del got, into


def _wgrad3_s2_planes64(gy, x, planes):
  """The weight gradient (Co, Ci, 3, 3, 3) of the stride-2 convolution for a gy (1, Co, D / 2, H / 2, W / 2) that is non-zero on its
  depth planes `planes` only: output voxel q reads x at 2 q + k - 1."""
  Co, Ci = gy.shape[1], x.shape[1]
  Ho, Wo = gy.shape[3:]
  gw = torch.zeros((Co, Ci, 3, 3, 3), dtype=torch.float64)
  for q in planes:
    g = _planes64(gy, [q])[:, 0].reshape(Co, Ho * Wo)
    slab = F.pad(_planes64(x, [2 * q - 1, 2 * q, 2 * q + 1]), (1, 1, 1, 1))
    for kd in range(3):
      for kh in range(3):
        for kw in range(3):
          gw[:, :, kd, kh, kw] += g @ slab[:, kd, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2].reshape(Ci, Ho * Wo).t()
  return gw


WG3S2_SHAPES = {'inside': (254, 128, 512), 'beyond': (256, 128, 512)}  # 32 * DHW = 2^29 - 2^22 | 2^29


@pytest.mark.parametrize('side', ['inside', 'beyond'])
def test_conv3d_stride2_weight_gradient_on_both_sides_of_its_offset_limit(side, recorder):
  """conv3d_bwd_weight, stride 2, 32 -> 64: the split kernel addresses a 32-channel block of x with 32-bit byte offsets
  (32 * DHW < 2^29 elements).  A limit this work did not move, but one of the few whose two sides fit on the device (x 2 GiB, gy
  0.5 GiB) and nothing tested either.  gy is non-zero on its depth planes {0, 1, Do - 2, Do - 1}; the whole gradient is compared."""
  D, H, W = WG3S2_SHAPES[side]
  Ci, Co = 32, 64
  assert mode_hip.lib().mode_conv3d_split_shape_supported(Ci, Co, D, H, W, 2, 2) == (1 if side == 'inside' else 0)
  Do = D // 2
  planes = [0, 1, Do - 2, Do - 1]
  x = _randn((1, Ci, D, H, W), 1171)
  gy = torch.zeros((1, Co, Do, H // 2, W // 2), dtype=torch.float32, device=DEV)
  for i, q in enumerate(planes):
    gy[0, :, q] = _randn((Co, H // 2, W // 2), 1172 + i)
  want = _wgrad3_s2_planes64(gy, x, planes)
  scale = max(1.0, float(want.abs().max()))
  entry = 'mode_conv3d_bwd_weight' + ('_s2_split' if side == 'inside' else '')
  del recorder.names[:]
  got = HF.conv3d_bwd_weight(gy, x, 2)
  assert _ran(recorder, 'mode_conv3d_bwd_weight') == [entry], side
  e = _err(got, want)
  print('stride-2 conv3d_bwd_weight %s [%s]: error %.3e, bound %.3e (max |want| %.4g)' % (side, entry, e, 2e-5 * scale, float(want.abs().max())))
  assert e <= 2e-5 * scale, (side, e)  # tests/test_gpu_split.py::test_split_stride2_weight_gradient_against_float64


# ------------------------------------------------------------------------------------------------ 3 x 3 2-D weight gradient
@pytest.mark.parametrize('H', [2040, 2048, 2056])
@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('C', [32, 16])
def test_conv2d_weight_gradient_around_the_panorama_size(C, dil, H, recorder):
  """conv2d_bwd_weight at C -> C on H x 4096: 2040 rows is inside the split kernel's limit (128 HW + 4 dil W < 2^30), the 2048 x 4096
  panorama sits exactly on it and 2056 rows is beyond -- both run on the fp32 kernel.  gy is non-zero on rows {0..3}, {1020..1023},
  {H - 4..H - 1}; the whole gradient is compared, whichever entry ran, in both settings of CONV2D_F16."""
  W = 4096
  inside = H == 2040
  assert mode_hip.lib().mode_conv2d_split_shape_supported(C, C, H, W, dil, 2) == (1 if inside else 0)
  groups = [(0, 4), (1020, 1024), (H - 4, H)]
  x = _randn((1, C, H, W), 1131)
  gy = torch.zeros((1, C, H, W), dtype=torch.float32, device=DEV)
  for i, (r0, r1) in enumerate(groups):
    gy[0, :, r0:r1] = _randn((C, r1 - r0, W), 1132 + i)
  want = _wgrad2_rows64(gy, x, groups, dil)
  scale = max(1.0, float(want.abs().max()))
  for f16 in (True, False):
    HF.CONV2D_F16 = f16
    entry = 'mode_conv2d_bwd_weight' + (('_split_f16' if f16 else '_split') if inside else '')
    del recorder.names[:]
    got = HF.conv2d_bwd_weight(gy, x, dil)
    assert _ran(recorder, 'mode_conv2d_bwd_weight') == [entry], (H, f16)
    bound = 4e-6 * float(want.abs().max()) if (f16 and inside) else 2e-5 * scale  # tests/test_gpu_f16.py | tests/test_gpu_split.py
    e = _err(got, want)
    print('conv2d_bwd_weight %d->%d d%d %dx%d f16 %d [%s]: error %.3e, bound %.3e (max |want| %.4g)' %
          (C, C, dil, H, W, f16, entry, e, bound, float(want.abs().max())))
    assert e <= bound, (C, dil, H, f16, e, bound)
    del got


# ------------------------------------------------------------------------------------------------ three dispatcher limits with a fallback
@pytest.mark.parametrize('shape', [(4369, 15, 8), (4096, 16, 8)], ids=['inside', 'beyond'])
def test_batchnorm_on_both_sides_of_its_grid_limit(shape, recorder):
  """bn_supported: B * C < 65536 (one workgroup row per (sample, channel) in a 16-bit grid dimension).  4369 x 15 = 65535 runs on the
  fused kernels, 4096 x 16 = 65536 on the torch module; training forward and backward with ReLU and a residual against float64 under
  the bounds of tests/test_gpu_kernels.py::test_bn_act_train_and_eval."""
  inside = shape[0] * shape[1] < 65536
  C = shape[1]
  ref_bn, dev_bn = nn.BatchNorm1d(C).double(), nn.BatchNorm1d(C).to(DEV)
  g = torch.Generator().manual_seed(7)
  gamma = 1 + 0.2 * torch.randn(C, generator=g)
  beta = 0.3 * torch.randn(C, generator=g)
  with torch.no_grad():
    for bn in (ref_bn, dev_bn):
      bn.weight.copy_(gamma)
      bn.bias.copy_(beta)
  y = _randn(shape, 1141, 2.0) + 1.5
  add = _randn(shape, 1142)
  gout = _randn(shape, 1143)
  ya = y.cpu().double().requires_grad_(True)
  aa = add.cpu().double().requires_grad_(True)
  o_ref = torch.relu(ref_bn(ya) + aa)
  o_ref.backward(gout.cpu().double())
  yd, ad = y.clone().requires_grad_(True), add.clone().requires_grad_(True)
  assert HF.bn_supported(yd) == inside
  del recorder.names[:]
  out = stage3d.bn_act(dev_bn, yd, ad, True)
  out.backward(gout)
  ran = _ran(recorder, 'mode_bn_')
  assert (len(ran) > 0) == inside, ran
  errs = (_err(out, o_ref.detach()), _err(yd.grad, ya.grad), _err(ad.grad, aa.grad), _err(dev_bn.weight.grad, ref_bn.weight.grad),
          _err(dev_bn.bias.grad, ref_bn.bias.grad), _err(dev_bn.running_mean, ref_bn.running_mean), _err(dev_bn.running_var, ref_bn.running_var))
  print('bn_act %s %s: out %.2e gy %.2e gadd %.2e gweight %.2e gbias %.2e mean %.2e var %.2e' % ((shape, ran[:2]) + errs))
  assert errs[0] < 2e-5
  assert errs[1] < 5e-5 * max(1.0, float(ya.grad.abs().max()))
  assert errs[2] < 1e-6
  assert errs[3] < 1e-4 * max(1.0, float(ref_bn.weight.grad.abs().max()))
  assert errs[4] < 1e-4 * max(1.0, float(ref_bn.bias.grad.abs().max()))
  assert errs[5] < 1e-5 and errs[6] < 1e-4
  assert int(dev_bn.num_batches_tracked) == 1


@pytest.mark.parametrize('B', [2047, 2048], ids=['inside', 'beyond'])
def test_statistics_epilogue_on_both_sides_of_its_grid_limit(B, recorder):
  """conv3d_stats_supported: B * Co < 65536.  B = 2047 at 8 -> 32 takes the BatchNorm statistics in the convolution's epilogue, B = 2048
  runs the convolution and then the BatchNorm composition (itself beyond bn_supported: the torch module); both against float64 under the
  bounds of tests/test_gpu_kernels.py::test_conv3d_with_batchnorm_statistics_in_its_epilogue.

  Of that test's two configurations this takes the one with a residual and WITHOUT the ReLU.  The batch is 33.5 million activations: with
  a ReLU about a dozen of them land within fp32 rounding of zero (|bn(y)| < ~5e-7: a fraction of 4e-7 of a unit normal), the float64
  reference and the fp32 kernel then disagree on their mask, and ONE such element moves the input gradient by ~0.03 against a bound of
  5e-4 -- a property of the reference at this size, not of either path (the existing test's largest case has 0.26 million)."""
  Ci, Co, D, H, W = 8, 32, 2, 8, 32
  inside = B * Co < 65536
  HF.CONV3D_BN_STATS = True
  seq64 = nn.Sequential(nn.Conv3d(Ci, Co, 3, 1, 1, bias=False), nn.BatchNorm3d(Co)).double()
  seq = nn.Sequential(nn.Conv3d(Ci, Co, 3, 1, 1, bias=False), nn.BatchNorm3d(Co)).to(DEV)
  w = _randn((Co, Ci, 3, 3, 3), 1152, (2.0 / (27 * Ci))**0.5) + 0.02
  with torch.no_grad():
    seq[0].weight.copy_(w)
    seq64[0].weight.copy_(w.cpu().double())
  x = _randn((B, Ci, D, H, W), 1151) + 3.0
  gout = _randn((B, Co, D, H, W), 1153)
  add = _randn((B, Co, D, H, W), 1154)
  xa = x.cpu().double().requires_grad_(True)
  o = seq64(xa) + add.cpu().double()
  o.backward(gout.cpu().double())
  xd = x.clone().requires_grad_(True)
  assert HF.conv3d_stats_supported(xd, seq[0].weight, seq[1]) == inside
  del recorder.names[:]
  out = stage3d.conv_bn(seq, xd, relu=False, add=add)
  out.backward(gout)
  ran = [n for n in recorder.names if n.startswith('mode_conv3d_fwd')]
  assert ran == (['mode_conv3d_fwd_split_stats'] if inside else ['mode_conv3d_fwd_split_f16' if HF.CONV3D_S1_F16 else 'mode_conv3d_fwd_split']), ran
  conv64, bn64, bn = seq64[0], seq64[1], seq[1]
  errs = (_err(out, o.detach()), _err(xd.grad, xa.grad), _err(seq[0].weight.grad, conv64.weight.grad), _err(bn.weight.grad, bn64.weight.grad),
          _err(bn.running_mean, bn64.running_mean), _err(bn.running_var, bn64.running_var))
  print('conv + BatchNorm statistics B = %d %s: out %.2e gx %.2e gw %.2e ggamma %.2e mean %.2e var %.2e' % ((B, ran) + errs))
  assert errs[0] < 2e-4 * max(1.0, float(o.detach().abs().max()))
  assert errs[1] < 2e-4 * max(1.0, float(xa.grad.abs().max()))
  assert errs[2] < 2e-4 * max(1.0, float(conv64.weight.grad.abs().max()))
  assert errs[3] < 2e-4 * max(1.0, float(bn64.weight.grad.abs().max()))
  assert errs[4] < 1e-4 * max(1.0, float(bn64.running_mean.abs().max()))
  assert errs[5] < 1e-3 * max(1.0, float(bn64.running_var.abs().max()))
  assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize('W', [849, 850], ids=['inside', 'beyond'])
def test_folded_cost_volume_convolution_on_both_sides_of_its_lds_limit(W, recorder):
  """cost_conv_supported: the adjoint keeps D4 gradient rows of W + 4 floats (+ 4) in LDS -- 163 792 B at D4 = 48, W = 849, within the
  160 KiB of a CU, 163 984 B at W = 850.  Inside, HF.cost_conv; beyond, what the model then runs -- the volume and the convolution on it
  (the two-kernel path); forward and the gradients of both feature maps and of the weight against float64, as
  tests/test_gpu_kernels.py::test_cost_conv_equals_conv3d_of_the_cost_volume does."""
  B, C, Co, D4, H = 1, 4, 8, 48, 3
  assert 4 * (4 + D4 * (849 + 4)) == 163792 <= 160 * 1024 < 163984 == 4 * (4 + D4 * (850 + 4))
  ref, tgt = _randn((B, C, H, W), 1161), _randn((B, C, H, W), 1162)
  w = _randn((Co, 2 * C, 3, 3, 3), 1163, 0.2)
  ra, ta, wa = (t.cpu().double().requires_grad_(True) for t in (ref, tgt, w))
  y_ref = F.conv3d(mode_ref.cost_volume(ra, ta, D4), wa, None, 1, 1)
  gy = _randn(tuple(y_ref.shape), 1164)
  y_ref.backward(gy.cpu().double())
  rd, td, wd = (t.clone().requires_grad_(True) for t in (ref, tgt, w))
  inside = W == 849
  assert HF.cost_conv_supported(rd, D4, Co) == inside
  del recorder.names[:]
  if inside:
    y = HF.cost_conv(rd, td, wd, D4)
  else:
    y = HF.conv3d(HF.cost_volume(rd, td, D4), wd, 1)
  y.backward(gy)
  ran = collections.Counter(n for n in recorder.names if 'cost' in n)
  assert (ran['mode_cost_conv_assemble_fwd'], ran['mode_cost_conv_assemble_bwd'], ran['mode_cost_volume_fwd'], ran['mode_cost_volume_bwd']) == \
      ((1, 1, 0, 0) if inside else (0, 0, 1, 1)), ran
  tol = 2e-6 * (2 * C * 27)
  errs = (_err(y, y_ref.detach()), _err(rd.grad, ra.grad), _err(td.grad, ta.grad), _err(wd.grad, wa.grad))
  print('cost_conv W = %d: y %.2e gref %.2e gtgt %.2e gw %.2e' % ((W,) + errs))
  assert errs[0] < tol * max(1.0, float(y_ref.abs().max()))
  for e, want in zip(errs[1:], (ra.grad, ta.grad, wa.grad)):
    assert e < 1e-5 * max(1.0, float(want.abs().max()))
