"""GPU (-m gpu): the split-operand MFMA kernels against the precision contract of csrc/split_arith.h, COMPONENTWISE: three bf16 pieces
keep 24 bits of every element whatever its size next to the rest of its tensor, two fp16 pieces 22 bits down to ~2^-17 of the tensor's
maximum.

Each shared case of tests/split_ref.py runs through mode_hip.functional, the entry that launched is asserted (a recording stand-in for
the ctypes handle, as tests/test_gpu_size_contracts.py), and the result is measured as u = |got - want| / (operator on |a|, |b|) in units
of 2^-24 / 2^-22 against the float64 operator.  Asserted: the whole-tensor rms of u and the worst rms over slices along every axis of the
output are both <= T, where T is a third of what the mildest emulated mutant of the arithmetic -- one partial product lost; on fp16
pieces also an operand scaled 2^4 too low -- gives on the same inputs (computed on the host, never from a kernel's output).
tests/test_split_ref_host.py shows on the CPU that a faithful kernel with an fp32 accumulator stays below T / 1.5 and a mutant confined to
one channel or one column tile exceeds T, on every one of these cases.  A role whose layer the split kernel does not take at that shape
(an input gradient over 20 or 40 output channels, a spherical forward with 6 input channels per group -- which the split ENTRY runs on
its fp32 kernels --, ...) is not judged here: it prints a line (with the case of tests/test_gpu_grad32_precision.py that judges it), and the roles that ARE judged are written out per shape (JUDGED) and
asserted, so that a probe or planner that starts to say no cannot quietly empty a case.

What the spherical entries are judged on: the windowed forward at 16 -> 32 and 128 -> 128 (64 x 128 table), 32 -> 64 with groups 2
(33 x 66, ragged tiles) and 16 -> 32 (16 x 32); the windowed weight gradient on the same four and at 12 -> 40 with groups 2 (33 x 66),
its six-decades kind at 16 x 32 only; the windowed input gradient at 128 -> 128 and 64 -> 64 on the 32 x 64 table, the only one here with
an adjoint plan.  Two of these rows are recorded findings (KNOWN below): expected failures, not passes.

Three bf16 pieces: CONV_ARITH = 'bf16x6' with CONV3D_S1_F16, CONV2D_F16, SPHERE_FWD_F16 and SPHERE_BWD_F16 off -- the 24-bit opt-out of
inference and of `--no-conv3d-f16`.  Two fp16 pieces: the default switches; stride-1 3-D and 3 x 3 layers (the spherical fp16 entries, whose weight and input
gradients mix arithmetics tile by tile, are judged part by part in tests/test_gpu_sphere_f16_precision.py).

MEASURED on an MI355X (one run of this file; T is computed, rms and worst slice are measured; for each family, role, arithmetic and kind of
data the case with the least room, i.e. the largest worst slice / T, and over how many shapes):

family     role                  pieces    data                          T    rms  worst  at the shape (of n), slice
conv3d_s1  forward               3 x bf16  unit variance             0.621  0.404  0.446  1x64x32x4x8x32 (5), axis 4 @ 23
conv3d_s1  input gradient        3 x bf16  unit variance             0.832  0.400  0.424  1x32x32x6x10x40 (4), axis 4 @ 21
conv3d_s1  input gradient + acc  3 x bf16  unit variance             0.828  0.399  0.422  1x32x32x6x10x40 (4), axis 4 @ 21
conv3d_s1  weight gradient       3 x bf16  unit variance             0.490  0.063  0.068  1x32x32x6x10x40 (5), axis 0 @ 13
conv3d_s1  forward               3 x bf16  six decades along a row   0.923  0.569  0.781  1x64x32x4x8x32 (5), axis 1 @ 9
conv3d_s1  input gradient        3 x bf16  six decades along a row   1.210  0.564  0.733  1x32x32x6x10x40 (4), axis 1 @ 5
conv3d_s1  input gradient + acc  3 x bf16  six decades along a row   1.208  0.564  0.734  1x32x32x6x10x40 (4), axis 1 @ 5
conv3d_s1  weight gradient       3 x bf16  six decades along a row   3.486  1.112  1.215  1x32x32x6x10x40 (5), axis 0 @ 14
conv3d_s1  input gradient        3 x bf16  gradient-sized            0.870  0.395  0.440  1x64x32x4x8x32 (4), axis 1 @ 39
conv3d_s1  input gradient + acc  3 x bf16  gradient-sized            0.865  0.395  0.437  1x64x32x4x8x32 (4), axis 1 @ 22
conv3d_s1  weight gradient       3 x bf16  gradient-sized            0.490  0.063  0.070  1x32x32x6x10x40 (5), axis 0 @ 3
conv3d_s1  forward               2 x fp16  unit variance            13.027  0.074  0.081  1x64x32x4x8x32 (5), axis 1 @ 7
conv3d_s1  input gradient        2 x fp16  unit variance            18.554  0.074  0.084  1x64x32x4x8x32 (4), axis 1 @ 22
conv3d_s1  input gradient + acc  2 x fp16  unit variance            18.447  0.074  0.084  1x64x32x4x8x32 (4), axis 1 @ 22
conv3d_s1  weight gradient       2 x fp16  unit variance            10.718  0.022  0.024  2x16x20x5x7x33 (5), axis 1 @ 14
conv3d_s1  forward               2 x fp16  six decades along a row   0.201  0.111  0.157  1x64x32x4x8x32 (5), axis 1 @ 9
conv3d_s1  input gradient        2 x fp16  six decades along a row   0.275  0.110  0.134  1x64x32x4x8x32 (4), axis 1 @ 13
conv3d_s1  input gradient + acc  2 x fp16  six decades along a row   0.275  0.110  0.134  1x64x32x4x8x32 (4), axis 1 @ 13
conv3d_s1  weight gradient       2 x fp16  six decades along a row  71.799  0.313  0.355  1x32x32x6x10x40 (5), axis 1 @ 27
conv3d_s1  input gradient        2 x fp16  gradient-sized           17.706  0.074  0.080  1x32x32x6x10x40 (4), axis 4 @ 21
conv3d_s1  input gradient + acc  2 x fp16  gradient-sized           17.609  0.074  0.079  1x32x32x6x10x40 (4), axis 4 @ 21
conv3d_s1  weight gradient       2 x fp16  gradient-sized           10.342  0.021  0.023  1x32x32x6x10x40 (5), axis 0 @ 20
conv3d_s2  forward               3 x bf16  unit variance             0.595  0.283  0.315  1x64x64x6x8x24 (2), axis 1 @ 54
conv3d_s2  input gradient        3 x bf16  unit variance             1.567  0.392  0.432  3x64x128x2x4x8 (3), axis 1 @ 22
conv3d_s2  weight gradient       3 x bf16  unit variance             2.029  0.230  0.249  1x64x64x6x8x24 (3), axis 0 @ 55
conv3d_s2  forward               3 x bf16  six decades along a row   0.919  0.420  0.533  1x64x64x6x8x24 (2), axis 1 @ 50
conv3d_s2  input gradient        3 x bf16  six decades along a row   2.506  0.598  0.699  3x64x128x2x4x8 (3), axis 4 @ 3
conv3d_s2  weight gradient       3 x bf16  six decades along a row   5.403  0.920  1.025  2x32x64x8x12x32 (3), axis 0 @ 48
conv3d_s2  input gradient        3 x bf16  gradient-sized            1.574  0.383  0.440  3x64x128x2x4x8 (3), axis 1 @ 0
conv3d_s2  weight gradient       3 x bf16  gradient-sized            2.026  0.229  0.249  1x64x64x6x8x24 (3), axis 0 @ 55
deconv3d   forward               3 x bf16  unit variance             1.928  0.385  0.429  2x64x64x3x4x8 (2), axis 1 @ 13
deconv3d   input gradient        3 x bf16  unit variance             0.610  0.281  0.312  2x64x64x3x4x8 (2), axis 1 @ 60
deconv3d   weight gradient       3 x bf16  unit variance             0.848  0.098  0.105  2x64x32x4x6x16 (2), axis 0 @ 31
deconv3d   forward               3 x bf16  six decades along a row   2.884  0.586  0.708  2x64x64x3x4x8 (2), axis 1 @ 62
deconv3d   input gradient        3 x bf16  six decades along a row   1.012  0.457  0.544  2x64x64x3x4x8 (2), axis 1 @ 50
deconv3d   weight gradient       3 x bf16  six decades along a row   5.368  0.920  0.969  2x64x32x4x6x16 (2), axis 0 @ 48
deconv3d   input gradient        3 x bf16  gradient-sized            0.610  0.286  0.313  2x64x64x3x4x8 (2), axis 1 @ 30
deconv3d   weight gradient       3 x bf16  gradient-sized            0.850  0.098  0.105  2x64x32x4x6x16 (2), axis 0 @ 16
conv2d     forward               3 x bf16  unit variance             0.990  0.393  0.447  1x64x64x12x32x2 (4), axis 1 @ 59
conv2d     input gradient        3 x bf16  unit variance             0.773  0.404  0.448  1x32x96x18x70x2 (3), axis 3 @ 67
conv2d     input gradient + acc  3 x bf16  unit variance             0.769  0.403  0.448  1x32x96x18x70x2 (3), axis 3 @ 67
conv2d     weight gradient       3 x bf16  unit variance             1.186  0.201  0.231  1x64x64x12x32x2 (4), axis 0 @ 24
conv2d     forward               3 x bf16  six decades along a row   1.653  0.653  1.045  1x64x64x12x32x2 (4), axis 1 @ 59
conv2d     input gradient        3 x bf16  six decades along a row   1.144  0.567  0.718  1x32x96x18x70x2 (3), axis 1 @ 19
conv2d     input gradient + acc  3 x bf16  six decades along a row   1.143  0.568  0.722  1x32x96x18x70x2 (3), axis 1 @ 19
conv2d     weight gradient       3 x bf16  six decades along a row   5.371  0.994  1.143  2x32x32x16x64x1 (4), axis 1 @ 26
conv2d     input gradient        3 x bf16  gradient-sized            0.773  0.399  0.453  1x32x96x18x70x2 (3), axis 3 @ 49
conv2d     input gradient + acc  3 x bf16  gradient-sized            0.769  0.398  0.453  1x32x96x18x70x2 (3), axis 3 @ 49
conv2d     weight gradient       3 x bf16  gradient-sized            1.186  0.202  0.229  1x64x64x12x32x2 (4), axis 1 @ 49
conv2d     forward               2 x fp16  unit variance            20.800  0.076  0.084  1x64x64x12x32x2 (4), axis 1 @ 63
conv2d     input gradient        2 x fp16  unit variance            16.386  0.074  0.082  1x32x96x18x70x2 (3), axis 3 @ 62
conv2d     input gradient + acc  2 x fp16  unit variance            16.306  0.074  0.082  1x32x96x18x70x2 (3), axis 3 @ 62
conv2d     weight gradient       2 x fp16  unit variance            24.979  0.048  0.053  1x64x64x12x32x2 (4), axis 1 @ 22
conv2d     forward               2 x fp16  six decades along a row   0.258  0.132  0.209  1x64x64x12x32x2 (4), axis 1 @ 59
conv2d     input gradient        2 x fp16  six decades along a row   0.249  0.128  0.193  1x64x64x12x32x2 (3), axis 1 @ 19
conv2d     input gradient + acc  2 x fp16  six decades along a row   0.249  0.128  0.192  1x64x64x12x32x2 (3), axis 1 @ 19
conv2d     weight gradient       2 x fp16  six decades along a row  109.369  0.285  0.340  2x32x32x16x64x1 (4), axis 1 @ 11
conv2d     input gradient        2 x fp16  gradient-sized           16.386  0.075  0.085  1x32x96x18x70x2 (3), axis 3 @ 49
conv2d     input gradient + acc  2 x fp16  gradient-sized           16.306  0.075  0.085  1x32x96x18x70x2 (3), axis 3 @ 49
conv2d     weight gradient       2 x fp16  gradient-sized           24.979  0.048  0.053  1x64x64x12x32x2 (4), axis 1 @ 10
sphere     forward               3 x bf16  unit variance             0.565  0.363  0.411  64x128x1x128x128x1 (4), axis 3 @ 28
sphere     weight gradient       3 x bf16  unit variance             0.212  0.055  0.061  64x128x1x16x32x1 (5), axis 3 @ 1
sphere     forward               3 x bf16  six decades along a row   0.832  0.541  0.911  64x128x1x128x128x1 (4), axis 1 @ 58
sphere     weight gradient       3 x bf16  gradient-sized            0.214  0.056  0.062  64x128x1x16x32x1 (5), axis 3 @ 1
sphere     input gradient        3 x bf16  unit variance             0.591  0.357  0.471  32x64x1x128x128x1 (2), axis 3 @ 0
sphere     input gradient        3 x bf16  six decades along a row   0.885  0.553  0.919  32x64x1x128x128x1 (2), axis 1 @ 115
sphere     input gradient        3 x bf16  gradient-sized            0.591  0.358  0.490  32x64x1x128x128x1 (2), axis 3 @ 0
sphere     weight gradient       3 x bf16  six decades along a row   4.963  2.669  3.006  16x32x1x16x32x1 (1), axis 1 @ 3

(sphere, six decades: the forward's 0.911 > T 0.832 and the input gradient's 0.919 > T 0.885 are the two findings recorded at KNOWN below,
both at 128 -> 128; every other case is inside T, the same entries at shorter reductions among them.)
"""
import pytest
import torch

import cpu_threads
import mode_hip
import split_ref as S
from mode_hip import functional as HF
from test_gpu_size_contracts import recorder  # noqa: F401  (the fixture that records the launching entries by name)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('CONV3D_S1_F16', 'CONV2D_F16', 'SPHERE_FWD_F16', 'SPHERE_BWD_F16', 'SPHERE_FWD_MIN_WG', 'SPHERE_BWD_SPLIT_MIN_WG')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  mode_hip.lib()
  torch.set_num_threads(cpu_threads.usable_cores())


@pytest.fixture
def switches():
  """The arithmetic switches of mode_hip.functional, restored after the case."""
  keep = (HF.CONV_ARITH,) + tuple(getattr(HF, n) for n in SWITCHES)
  yield
  HF.set_conv_arith(keep[0])
  for n, v in zip(SWITCHES, keep[1:]):
    setattr(HF, n, v)


def _set_arith(arith):
  HF.set_conv_arith('bf16x6')
  f16 = arith == 'f16x3'
  HF.CONV3D_S1_F16 = HF.CONV2D_F16 = f16
  if not f16:
    HF.SPHERE_FWD_F16 = HF.SPHERE_BWD_F16 = False
  HF.SPHERE_FWD_MIN_WG = HF.SPHERE_BWD_SPLIT_MIN_WG = 0  # the small spherical cases too (tests/test_gpu_kernels.py routes them so)


def _launch(case, role, t):
  """(the entry that must run, a callable that runs the role on the device) -- or (None, None) where the split kernels do not take this
  layer at this shape.  role.a / role.b are the operands of the convolutions; the sphere starts from x (its operand is sampled)."""
  lib = mode_hip.lib()
  fam, name, f16 = case.family, role.name, case.arith == 'f16x3'
  sfx = '_f16' if f16 else ''
  d = lambda v: v.to(DEV)
  if fam in ('conv3d_s1', 'conv3d_s2'):
    stride = 1 if fam == 'conv3d_s1' else 2
    s2 = '_s2' if stride == 2 else ''
    if name == 'forward':
      B, Ci, D, H, W = role.a.shape
      ok = lib.mode_conv3d_split_shape_supported(Ci, role.b.shape[0], D, H, W, stride, 0) == 1
      return ('mode_conv3d_fwd%s_split%s' % (s2, sfx), lambda: HF.conv3d_fwd(d(role.a), d(role.b), stride)) if ok else (None, None)
    if name.startswith('input gradient'):
      xs = tuple(t['x'].shape)
      Co, Ci = role.b.shape[:2]
      ok = lib.mode_conv3d_split_shape_supported(Ci, Co, xs[2], xs[3], xs[4], stride, 1) == 1
      if role.acc is None:
        return ('mode_conv3d_bwd_data%s_split%s' % (s2, sfx), lambda: HF.conv3d_bwd_data(d(role.a), d(role.b), xs, stride)) if ok else (None, None)
      ok = ok and lib.mode_conv3d_bwd_data_split_acc_supported(Ci, Co, stride) == 1
      entry = 'mode_conv3d_bwd_data_split' + ('_f16' if f16 else '_acc')
      return (entry, lambda: HF.conv3d_bwd_data(d(role.a), d(role.b), xs, stride, acc=d(role.acc))) if ok else (None, None)
    B, Ci, D, H, W = role.b.shape
    ok = lib.mode_conv3d_split_shape_supported(Ci, role.a.shape[1], D, H, W, stride, 2) == 1
    return ('mode_conv3d_bwd_weight%s_split%s' % (s2, sfx), lambda: HF.conv3d_bwd_weight(d(role.a), d(role.b), stride)) if ok else (None, None)
  if fam == 'deconv3d':
    B, cin, cout, D, H, W = case.shape
    vol = (2 * D, 2 * H, 2 * W)
    if name == 'forward':
      ok = lib.mode_conv3d_split_shape_supported(cout, cin, vol[0], vol[1], vol[2], 2, 1) == 1
      return ('mode_deconv3d_fwd_split', lambda: HF.deconv3d_fwd(d(role.a), d(role.b))) if ok else (None, None)
    if name == 'input gradient':  # the stride-2 convolution of gy with the same weights (Deconv3dFunction.backward)
      ok = lib.mode_conv3d_split_shape_supported(cout, cin, vol[0], vol[1], vol[2], 2, 0) == 1
      return ('mode_conv3d_fwd_s2_split', lambda: HF.conv3d_fwd(d(role.a), d(role.b), 2)) if ok else (None, None)
    ok = lib.mode_conv3d_split_shape_supported(cout, cin, vol[0], vol[1], vol[2], 2, 2) == 1
    return ('mode_conv3d_bwd_weight_s2_split', lambda: HF.conv3d_bwd_weight(d(role.a), d(role.b), 2)) if ok else (None, None)
  if fam == 'conv2d':
    dil = case.shape[5]
    if name == 'forward':
      B, Ci, H, W = role.a.shape
      ok = lib.mode_conv2d_split_shape_supported(Ci, role.b.shape[0], H, W, dil, 0) == 1
      return ('mode_conv2d_fwd_split' + sfx, lambda: HF.conv2d_fwd(d(role.a), d(role.b), dil, f16=f16)) if ok else (None, None)
    if name.startswith('input gradient'):
      Co, Ci = role.b.shape[:2]
      ok = lib.mode_conv2d_split_shape_supported(Ci, Co, role.a.shape[2], role.a.shape[3], dil, 1) == 1
      if role.acc is None:
        return ('mode_conv2d_bwd_data_split' + sfx, lambda: HF.conv2d_bwd_data(d(role.a), d(role.b), dil)) if ok else (None, None)
      entry = 'mode_conv2d_bwd_data_split' + ('_f16' if f16 else '_acc')
      return (entry, lambda: HF.conv2d_bwd_data(d(role.a), d(role.b), dil, acc=d(role.acc))) if ok else (None, None)
    B, Ci, H, W = role.b.shape
    ok = lib.mode_conv2d_split_shape_supported(Ci, role.a.shape[1], H, W, dil, 2) == 1
    return ('mode_conv2d_bwd_weight_split' + sfx, lambda: HF.conv2d_bwd_weight(d(role.a), d(role.b), dil)) if ok else (None, None)
  assert fam == 'sphere'
  ih, iw, B, ci, co, g = case.shape
  pos = d(t['pos'])
  H, W = pos.shape[2:]
  plan = HF.sphere_plan(pos, 3, 3)
  if name == 'forward':
    # (csrc/sphere_win_fwd.hip, sphere_conv_fwd_win_impl: the split kernel takes 16 input channels of a group per chunk; with fewer the
    # SAME entry runs the fp32 window kernels, so the entry's name proves nothing there and the role is not judged)
    ok = HF._plan_usable(plan) and (ci // g) % 16 == 0
    return ('mode_sphere_conv_fwd_win_split',
            lambda: HF.sphere_conv_fwd(d(t['x']), pos, d(t['w']), torch.full((B, co, H, W), float('nan'), device=DEV), (1, 1), g)) if ok else (None, None)
  if name == 'weight gradient':
    ok = HF._plan_usable(plan)
    return ('mode_sphere_conv_bwd_weight_win_split',
            lambda: HF.sphere_conv_bwd_weight(d(t['gy']), pos, d(t['x']), torch.zeros((co, ci // g, 3, 3), device=DEV), (1, 1), g)) if ok else (None, None)
  ok = lib.mode_sphere_conv_bwd_data_win_supported(ci, co, g) == 1 and HF.sphere_adjplan(pos, 3, 3) is not None

  def run():  # on plane-transposed storage, as the model runs it (tests/test_gpu_split.py::test_split_sphere_input_gradient_against_float64)
    gxt = torch.full((B, ci, W, H), float('nan'), device=DEV)
    HF.sphere_conv_bwd_data_t(HF.transpose_planes(d(t['gy'])), pos, d(t['w']), gxt, g)
    return HF.transpose_planes(gxt)

  return ('mode_sphere_conv_bwd_data_win_split', run) if ok else (None, None)


COMPUTE = ('mode_conv', 'mode_deconv', 'mode_sphere_conv')  # (maximum passes, plane transposes and the like are not what is asserted)


# The roles of each shape that reach a split kernel, written out: a `*_supported` probe or a planner that starts to say no must fail the
# test, not quietly empty it.  (The 'gradient-sized' kind has no forward, the spherical six-decades kind a weight gradient at 16 x 32 only:
# tests/split_ref.py.)  What is NOT here is not judged HERE -- each such role prints a line, which names the case of
# tests/test_gpu_grad32_precision.py that judges it on the fp32 kernel it runs on, where there is one:
#   3-D 16 -> 20 and 3 x 3 16 -> 40: the input gradient reduces over 20 / 40 channels, off the kernels' 8 / 16 grid (fp32 kernels);
#   stride-2 64 -> 128: the forward's 128 output channels, which NO kernel takes (the operator raises; asserted there);
#   sphere: see SPHERE in tests/split_ref.py (compact tiles, 16 input channels per group, an adjoint plan).
ALL4 = ('forward', 'input gradient', 'input gradient + acc', 'weight gradient')
ALL3 = ('forward', 'input gradient', 'weight gradient')
JUDGED = {
    ('conv3d_s1', (2, 16, 20, 5, 7, 33)): ('forward', 'weight gradient'),
    ('conv3d_s2', (3, 64, 128, 2, 4, 8)): ('input gradient', 'weight gradient'),
    ('conv2d', (2, 16, 40, 7, 33, 1)): ('forward', 'weight gradient'),
    ('sphere', (64, 128, 1, 16, 32, 1)): ('forward', 'weight gradient'),
    ('sphere', (33, 66, 1, 12, 40, 2)): ('weight gradient',),
    ('sphere', (33, 66, 1, 32, 64, 2)): ('forward', 'weight gradient'),
    ('sphere', (32, 64, 1, 128, 128, 1)): ('input gradient',),
    ('sphere', (32, 64, 1, 64, 64, 1)): ('input gradient',),
    ('sphere', (64, 128, 1, 128, 128, 1)): ('forward', 'weight gradient'),
    ('sphere', (16, 32, 1, 16, 32, 1)): ('forward', 'weight gradient'),
}
DEFAULT_JUDGED = {'conv3d_s1': ALL4, 'conv3d_s2': ALL3, 'deconv3d': ALL3, 'conv2d': ALL4}


def _judged(case):
  return JUDGED.get((case.family, case.shape), DEFAULT_JUDGED.get(case.family))


# FINDINGS (kept in, strict: if a kernel starts to meet T the test fails until its entry is taken out; any OTHER role of these cases that
# misses T fails the test as usual).  Both are the 1152-term reductions (128 channels x 9 taps) on the six-decades data, both miss in
# their worst CHANNEL only, and in both the fp32 kernels -- no split arithmetic at all -- are worse on the same inputs and peak on the
# same channels, while torch's blocked fp32 product on the host has the same profile at half the level:
#   windowed input gradient, 32 x 64 table, 128 -> 128: T 0.885, rms 0.553, worst slice 0.919 (channel 115; then 34, 50, 73, 124, 70 at
#     0.82 - 0.87; median channel 0.51).  fp32 gather kernel (functional.SPHERE_BWD_DATA_SPLIT = False): rms 0.606, channel 115 at 1.017.
#     Host fp32: rms 0.258, channel 115 at 0.324, its worst 0.385.
#   windowed forward, 64 x 128 table, 128 -> 128: T 0.832, rms 0.541, worst slice 0.911 (channel 58; then 43, 125, 111, 8 at 0.77 - 0.82;
#     median 0.50).  fp32 window kernel (CONV_ARITH = 'f32'): rms 0.579, channel 58 at 0.951; fp32 gather kernel: 0.576 / 0.929.  Host
#     fp32: rms 0.247, channel 58 at 0.297, its worst 0.317.
# Both kernels were read against the term list of csrc/split_arith.h and keep it (per K-step the six products a1 b1, a1 b2, a2 b1, a2 b2,
# a1 b3, a3 b1 into one accumulator; the operand they split is the sampled / adjoint-sampled tensor, formed by an fma chain over its
# sources, which the emulation splits too).  The excess is fp32 ACCUMULATION: on non-negative data (relu) a channel whose 1152 weights do
# not sum to ~0 has partial sums that grow with the term count, and every addition rounds at their size -- a running sum over 1152 terms
# is measurably noisier there than a blocked one.  The host tier's condition (plain fp32 <= T / 1.5) holds for both cases, so their
# reductions are not shortened; instead the SAME entries on the same kind of data with shorter reductions are cases of their own and
# must pass -- input gradient 64 -> 64 at 32 x 64 (576 terms: worst slice 0.98 of T 1.29), forward 32 -> 64 with groups 2 at 33 x 66 (144)
# and 16 -> 32 (144) -- and that is where the six-decades contract of these entries is asserted.  Unit-variance and gradient-sized data
# pass at 128 -> 128.
KNOWN = {
    ('sphere-32x64x1x128x128x1-bf16x6-six_decades_along_a_row', 'input gradient', 'mode_sphere_conv_bwd_data_win_split'):
        'fp32 accumulation over 1152 terms on non-negative data: worst channel 0.919 > T 0.885 (the fp32 gather kernel: 1.017)',
    ('sphere-64x128x1x128x128x1-bf16x6-six_decades_along_a_row', 'forward', 'mode_sphere_conv_fwd_win_split'):
        'fp32 accumulation over 1152 terms on non-negative data: worst channel 0.911 > T 0.832 (the fp32 window kernel: 0.951)',
}


@pytest.mark.parametrize('case', S.CASES, ids=S.case_id)
def test_split_kernel_keeps_the_componentwise_contract(case, switches, recorder):
  _set_arith(case.arith)
  roles, tensors = S.roles(case)
  judged, missed, expected_misses = [], [], []
  shape = 'x'.join(str(v) for v in case.shape)
  if case.family == 'sphere':  # (tests/split_ref.py builds the roles of SPHERE_ROLES alone)
    for name in ALL3:
      if name not in S.SPHERE_ROLES[case.shape]:
        print('SPLITPREC-NOT-JUDGED | %s | %s | %s | %s | %s | no split kernel takes this role on this table' % (case.family, shape, name, case.arith, case.kind))
  for role in roles:
    entry, run = _launch(case, role, tensors)
    if entry is None:
      print('SPLITPREC-NOT-JUDGED | %s | %s | %s | %s | %s | no split kernel takes this role at this shape%s' %
            (case.family, shape, role.name, case.arith, case.kind, S.grad32_judges(case.family, case.shape, role.name, case.kind)))
      continue
    del recorder.names[:]
    got = run()
    torch.cuda.synchronize()
    ran = [n for n in recorder.names if n.startswith(COMPUTE)]
    expect = [entry] + (['mode_sphere_conv_bwd_data_adj_list'] if (ran[1:] == ['mode_sphere_conv_bwd_data_adj_list']) else [])
    assert ran == expect, (S.case_id(case), role.name, ran)
    ref = S.reference(case, role)
    whole, worst, rest = S.measure(case, role, ref, got)
    judged.append(role.name)
    print('SPLITPREC | %s | %s | %s | %s | %s | %s | T %.3f | rms %.3f | worst slice %.3f (axis %d @ %d)%s' %
          (case.family, shape, role.name, case.arith, case.kind, entry, ref.T, whole, worst.rms, worst.axis, worst.index,
           '' if rest is None else ' | columns past the contract, not judged: rms %.2f' % rest))
    ok = whole <= ref.T and worst.rms <= ref.T
    known = KNOWN.get((S.case_id(case), role.name, entry))
    if known is not None:
      assert not ok, 'this role now meets T (%.3f, worst slice %.3f): take it out of KNOWN' % (ref.T, worst.rms)
      expected_misses.append(known)
    elif not ok:
      missed.append((role.name, entry, 'T %.3f' % ref.T, 'rms %.3f' % whole, worst))
  want_judged = [r.name for r in roles if r.name in _judged(case)]
  assert judged == want_judged and judged, (S.case_id(case), judged, want_judged)
  assert not missed, (S.case_id(case), missed)
  if expected_misses:
    pytest.xfail('; '.join(expected_misses))
