"""GPU (-m gpu): the INFERENCE entries -- convolution + folded eval BatchNorm (+ residual) (+ ReLU) in one launch -- against the
componentwise precision contract that tests/test_gpu_split_precision.py holds the training entries to.

Each eval case of tests/split_ref.py (EVAL_CASES) runs through the public route (functional.conv3d_bn_eval, deconv3d_bn_eval,
conv2d_bn_eval, cost_conv_bn_eval; models.stage3d.conv_bn for the 1 x 1, stem and integer-table layers; SphereConv.forward_bn behind
an NCHW caller and on plane-transposed storage) under torch.no_grad(), in every epilogue variant the case lists.  Asserted per variant:
  * the entry that launched, by name (ENTRY; a recording stand-in for the ctypes handle): a probe or planner that starts to say no
    fails the test instead of emptying it;
  * whole-tensor rms and worst slice of u = |got - want| / den, in units of 2^-24 (2^-22 on two fp16 pieces), both <= T.  want is the
    float64 value of the UNFOLDED layer, den = op(|a|, |w'|) + |beta| + |mean s| + |add|, T a third of the mildest emulated mutant of the
    arithmetic on the case's own inputs (computed on the host, never from a kernel's output).  The fp32 entries are judged under the
    three-piece T of the same inputs.  tests/test_split_ref_host.py shows on the CPU that a faithful kernel with an fp32 accumulator stays
    below T / 1.5 and that an arithmetic fault in one channel or one column tile, one channel's fold scale off by 2^-12, a shift taken
    from the neighbouring channel and a residual read from the wrong channel block all exceed T, for every one of these variants;
  * the kept pack: a second call on the same BatchNorm module hits the packed-weight cache (it runs under mode_weight_pack_reuse; on
    fp16 it reuses the folded weights' maximum in the workspace) and returns the same bits; after bn.weight.mul_(2) the third call is
    within T of the NEW reference (every folded quantity doubles exactly), so a stale pack would have been seen;
  * the maximum tag: where the entry writes one, abs_max_value(known_abs_max(y)) is the largest finite |y| exactly; where it writes none,
    known_abs_max(y) is None.

The eval instantiations, read from the launch code of csrc/*, and the case that reaches each:
  conv3d_split.hip      conv3d_split_kernel<MT, EPI 1 | 2, F16 false>: shift / shift + residual store on three bf16 pieces
                          (mode_conv3d_fwd_split with an epilogue)                                    conv3d_s1 * route split
                        conv3d_split_kernel<MT, 1 | 2, F16 true, 8, AMAX true>: the same on two fp16 pieces, the output's maximum
                          taken in the store (mode_conv3d_fwd_split_f16_bn)                           conv3d_s1 * route f16
                        conv3d_split_kernel<MT, 1, true, 16, true>: the 16-row tile -- no residual, H % 16 == 0 and
                          B cdiv(D, 2) (H / 8) cdiv(W, 32) >= 4 x 256                                 the tall-tile test below
  conv3d_split_s2.hip   the stride-2 kernel's epilogue forms with the maximum (mode_conv3d_fwd_s2_split_amax)  conv3d_s2 * route split
  conv3d_split_deconv.hip  the transposed kernel's own epilogue instantiation, residual values requested ahead of their stores
                          (mode_deconv3d_fwd_split_bn_amax)                                           deconv3d * route split
  conv2d_split.hip      the 3 x 3 kernel, dilation 1 | 2, epilogue forms on three bf16 pieces (mode_conv2d_fwd_split) and on two fp16
                          pieces with the maximum (mode_conv2d_fwd_split_f16_bn)                      conv2d * route split | f16
  sphere_win_fwd.hip    the windowed split kernel with the epilogue, NCHW caller (plane-transposed copies) and transposed storage
                          (mode_sphere_conv_fwd_win_split)                                            sphere * route split
  conv3d.hip            the fp32 MFMA kernels' folded forms: stride 1, stride 2 (mode_conv3d_fwd_bn), transposed with one and two
                          output tiles (mode_deconv3d_fwd_bn)                                         conv3d_s1 | conv3d_s2 | deconv3d * route f32
  conv2d_f32_fwd.hip    the fp32 3 x 3 kernel, dilation 1 | 2 (mode_conv2d_fwd_bn)                    conv2d * route f32
  conv1x1.hip           the 1 x 1 GEMM, stride 1 | 2, channels off the 8 / 32 blocks (mode_conv1x1_fwd_bn)    conv2d_gen k = 1
  conv_stem.hip         the 7 x 7 stride-2 stem (mode_conv_stem_fwd_bn)                               conv2d_gen k = 7
  sphere_conv.hip       the general gather kernel with the epilogue (mode_sphere_conv_fwd_bn): integer tables (3 x 3 stride 2, 5 x 5),
                          ERP stride 1 | 2, Cassini with groups 2                                     conv2d_gen k = 3 | 5, sphere_gen
  cost_conv.hip         the assembly with scale, shift, ReLU and maximum (mode_cost_conv_assemble_fwd_bn_amax): the scale multiplies
                          the assembled sum there, den = |s| op(|volume|, |w|)                        cost_conv

MEASURED on an MI355X (one run of this file; T is computed, rms and worst slice are measured; for each family, entry, arithmetic, kind
of data and BatchNorm kind the shape and epilogue variant with the least room, i.e. the largest worst slice / T, and over how many
measured variants -- the sphere's two routes count separately, the calls on the kept pack and after gamma x 2 do not):

family     entry                                pieces   data                     BN kind          T    rms  worst  at the shape, variant (of n measured), slice
conv3d_s1  conv3d_fwd_split                     3 x bf16 unit variance            typical      0.610  0.397  0.446  1x64x32x4x8x32, relu 0 add 0 (12), axis 1 @ 3
conv3d_s1  conv3d_fwd_split                     3 x bf16 six decades along a row  zero shift   0.640  0.429  0.954  1x64x32x4x8x32, relu 1 add 1 (12), axis 1 @ 2
conv3d_s1  conv3d_fwd_split_f16_bn              2 x fp16 unit variance            typical      9.038  0.051  0.063  1x64x32x4x8x32, relu 1 add 1 (12), axis 1 @ 20
conv3d_s1  conv3d_fwd_split_f16_bn              2 x fp16 six decades along a row  zero shift   0.137  0.083  0.189  1x64x32x4x8x32, relu 1 add 1 (12), axis 1 @ 2
conv3d_s1  conv3d_fwd_split                     3 x bf16 unit variance            spread       0.568  0.277  0.303  1x32x32x6x10x40, relu 1 add 1 (2), axis 4 @ 10
conv3d_s1  conv3d_fwd_split_f16_bn              2 x fp16 unit variance            spread      12.084  0.052  0.057  1x32x32x6x10x40, relu 1 add 1 (2), axis 1 @ 20
conv3d_s2  conv3d_fwd_s2_split_amax             3 x bf16 unit variance            typical      0.401  0.198  0.240  1x64x64x6x8x24, relu 1 add 1 (6), axis 1 @ 38
conv3d_s2  conv3d_fwd_s2_split_amax             3 x bf16 six decades along a row  zero shift   0.661  0.297  0.424  1x64x64x6x8x24, relu 1 add 1 (6), axis 1 @ 32
deconv3d   deconv3d_fwd_split_bn_amax           3 x bf16 unit variance            typical      1.039  0.244  0.383  2x64x64x3x4x8, relu 1 add 1 (6), axis 1 @ 60
deconv3d   deconv3d_fwd_split_bn_amax           3 x bf16 six decades along a row  zero shift   2.091  0.428  0.604  2x64x64x3x4x8, relu 1 add 1 (6), axis 1 @ 23
conv2d     conv2d_fwd_split                     3 x bf16 unit variance            typical      0.632  0.262  0.346  1x64x64x12x32x2, relu 1 add 1 (10), axis 1 @ 34
conv2d     conv2d_fwd_split                     3 x bf16 six decades along a row  zero shift   1.155  0.480  1.003  1x64x64x12x32x2, relu 1 add 1 (10), axis 1 @ 21
conv2d     conv2d_fwd_split_f16_bn              2 x fp16 unit variance            typical     13.478  0.050  0.065  1x64x64x12x32x2, relu 1 add 1 (10), axis 1 @ 20
conv2d     conv2d_fwd_split_f16_bn              2 x fp16 six decades along a row  zero shift   0.177  0.096  0.195  1x64x64x12x32x2, relu 1 add 1 (10), axis 1 @ 0
conv2d     conv2d_fwd_split                     3 x bf16 unit variance            spread       0.655  0.267  0.332  1x64x64x12x32x2, relu 1 add 1 (2), axis 1 @ 59
conv2d     conv2d_fwd_split_f16_bn              2 x fp16 unit variance            spread      14.141  0.052  0.061  1x64x64x12x32x2, relu 1 add 1 (2), axis 1 @ 56
sphere     sphere_conv_fwd_win_split            3 x bf16 unit variance            typical      0.389  0.251  0.305  64x128x1x128x128x1, relu 1 add 1 NCHW caller (20), axis 1 @ 50
sphere     sphere_conv_fwd_win_split            3 x bf16 six decades along a row  zero shift   1.738  0.444  0.983  33x66x1x32x64x2, relu 1 add 1 NCHW caller (16), axis 1 @ 50
conv3d_s1  conv3d_fwd_bn                        fp32     unit variance            typical      0.667  0.303  0.361  1x20x40x6x10x36, relu 1 add 1 (4), axis 1 @ 22
conv3d_s1  conv3d_fwd_bn                        fp32     six decades along a row  zero shift   1.106  0.342  0.590  1x20x40x6x10x36, relu 1 add 1 (4), axis 1 @ 15
conv3d_s2  conv3d_fwd_bn                        fp32     unit variance            typical      0.900  0.332  0.441  2x12x24x6x10x36, relu 1 add 0 (4), axis 1 @ 14
conv3d_s2  conv3d_fwd_bn                        fp32     six decades along a row  zero shift   1.323  0.355  0.837  2x12x24x6x10x36, relu 1 add 1 (4), axis 1 @ 17
deconv3d   deconv3d_fwd_bn                      fp32     unit variance            typical      1.391  0.272  0.362  2x24x40x3x5x34, relu 1 add 1 (6), axis 1 @ 25
deconv3d   deconv3d_fwd_bn                      fp32     six decades along a row  zero shift   2.985  0.387  0.501  2x24x40x3x5x34, relu 1 add 1 (6), axis 1 @ 21
conv2d     conv2d_fwd_bn                        fp32     unit variance            typical      1.023  0.300  0.409  2x20x40x9x40x1, relu 1 add 1 (6), axis 1 @ 23
conv2d     conv2d_fwd_bn                        fp32     six decades along a row  zero shift   1.606  0.324  0.690  2x20x40x9x40x1, relu 1 add 1 (6), axis 1 @ 34
conv2d_gen conv1x1_fwd_bn                       fp32     unit variance            typical      1.574  0.310  0.470  2x64x64x16x32x1x2x0, relu 1 add 1 (8), axis 1 @ 3
conv2d_gen conv1x1_fwd_bn                       fp32     six decades along a row  zero shift   2.631  0.365  0.856  2x64x64x16x32x1x2x0, relu 1 add 1 (8), axis 1 @ 34
conv2d_gen conv_stem_fwd_bn                     fp32     unit variance            typical      1.107  0.297  0.356  2x3x20x26x70x7x2x3, relu 1 add 1 (2), axis 3 @ 2
conv2d_gen conv_stem_fwd_bn                     fp32     six decades along a row  zero shift   2.027  0.399  0.728  2x3x20x26x70x7x2x3, relu 1 add 1 (2), axis 1 @ 15
conv2d_gen sphere_conv_fwd_bn                   fp32     unit variance            typical      1.172  0.298  0.409  2x6x40x16x24x5x1x2, relu 1 add 1 (4), axis 1 @ 30
conv2d_gen sphere_conv_fwd_bn                   fp32     six decades along a row  zero shift   2.097  0.423  0.907  2x6x40x16x24x5x1x2, relu 1 add 1 (4), axis 1 @ 33
sphere_gen sphere_conv_fwd_bn                   fp32     unit variance            typical      0.912  0.253  0.318  ERPx16x32x2x16x32x1x2, relu 1 add 1 NCHW caller (8), axis 1 @ 17
sphere_gen sphere_conv_fwd_bn                   fp32     six decades along a row  zero shift   2.185  0.552  0.955  ERPx16x32x2x16x32x1x1, relu 1 add 1 NCHW caller (8), axis 2 @ 1
cost_conv  cost_conv_assemble_fwd_bn_amax       fp32     unit variance            typical      1.238  0.182  0.290  2x8x12x5x6x20, relu 0 add 0 (2), axis 4 @ 0
cost_conv  cost_conv_assemble_fwd_bn_amax       fp32     six decades along a row  zero shift   1.778  0.209  0.315  2x8x12x5x6x20, relu 1 add 0 (2), axis 1 @ 10

(the tall-tile form, conv3d_fwd_split_f16_bn at 1x8x8x15x64x500, unit variance, typical, relu 1 add 0: T 21.366, rms 0.059, worst slice
0.080 -- and the same bits as the 8-row form.  Four variants miss T and are recorded findings, KNOWN below: all at 64 input channels
on the six-decades data; every other variant is inside T, the same entries at 8, 16 and 32 input channels among them.)"""
import pytest
import torch

import cpu_threads
import mode_hip
import split_ref as S
from mode_hip import functional as HF
from test_gpu_size_contracts import recorder  # noqa: F401  (the fixture that records the launching entries by name)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('CONV3D_EVAL_F16', 'CONV2D_EVAL_F16', 'SPHERE_FWD_MIN_WG')

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


def _set_route(case):
  HF.set_conv_arith('bf16x6')
  f16 = case.route == 'f16'
  if case.family == 'conv3d_s1':
    HF.CONV3D_EVAL_F16 = f16  # (the other 3-D entries keep the default: their epilogues take the maximum for the fp16 layer behind them)
  if case.family == 'conv2d':
    HF.CONV2D_EVAL_F16 = f16
  if case.family == 'sphere':
    HF.SPHERE_FWD_MIN_WG = 0  # the small tables too (the general cases, sphere_gen, keep the default: too few tiles -> the gather kernel)


# The entry every case of a (family, route) must launch -- conv2d_gen by its kernel size.
ENTRY = {
    ('conv3d_s1', 'split'): 'mode_conv3d_fwd_split',
    ('conv3d_s2', 'split'): 'mode_conv3d_fwd_s2_split_amax',
    ('deconv3d', 'split'): 'mode_deconv3d_fwd_split_bn_amax',
    ('conv2d', 'split'): 'mode_conv2d_fwd_split',
    ('sphere', 'split'): 'mode_sphere_conv_fwd_win_split',
    ('conv3d_s1', 'f16'): 'mode_conv3d_fwd_split_f16_bn',
    ('conv2d', 'f16'): 'mode_conv2d_fwd_split_f16_bn',
    ('conv3d_s1', 'f32'): 'mode_conv3d_fwd_bn',
    ('conv3d_s2', 'f32'): 'mode_conv3d_fwd_bn',
    ('deconv3d', 'f32'): 'mode_deconv3d_fwd_bn',
    ('conv2d', 'f32'): 'mode_conv2d_fwd_bn',
    ('conv2d_gen', 1): 'mode_conv1x1_fwd_bn',
    ('conv2d_gen', 7): 'mode_conv_stem_fwd_bn',
    ('conv2d_gen', 3): 'mode_sphere_conv_fwd_bn',
    ('conv2d_gen', 5): 'mode_sphere_conv_fwd_bn',
    ('sphere_gen', 'f32'): 'mode_sphere_conv_fwd_bn',
    ('cost_conv', 'f32'): 'mode_cost_conv_assemble_fwd_bn_amax',
}
WRITES_MAXIMUM = ('mode_conv3d_fwd_s2_split_amax', 'mode_deconv3d_fwd_split_bn_amax', 'mode_conv3d_fwd_split_f16_bn', 'mode_conv2d_fwd_split_f16_bn',
                  'mode_cost_conv_assemble_fwd_bn_amax')
NO_KEPT_PACK = ('mode_cost_conv_assemble_fwd_bn_amax',)  # (its weights go through the tap-product GEMMs: nothing is packed with the fold)
COMPUTE = ('mode_conv', 'mode_deconv', 'mode_sphere_conv', 'mode_cost_conv')  # (maximum passes and plane transposes are not what is asserted)
TAP_PRODUCTS = 'mode_sphere_conv_fwd'  # cost_conv: the two 3 x 1 tap-product convolutions in front of the assembly


def _entry_of(case):
  return ENTRY[(case.family, case.shape[5])] if case.family == 'conv2d_gen' else ENTRY[(case.family, case.route)]


def _bn_module(lin, dims):
  C = lin.gamma.numel()
  bn = (torch.nn.BatchNorm3d if dims == 3 else torch.nn.BatchNorm2d)(C, eps=S.BN_EPS).to(DEV).eval()
  with torch.no_grad():
    for p, v in ((bn.weight, lin.gamma), (bn.bias, lin.beta), (bn.running_mean, lin.mean), (bn.running_var, lin.var)):
      p.copy_(v)
  return bn


def _runners(case, lin):
  """[(label, bn, run(relu, add))]: the public routes of the case (two for the sphere), each on a BatchNorm module of its own."""
  fam = case.family
  d = lambda v: v.to(DEV)
  w = d(lin.w)  # the layer's own, unfolded weights
  if fam in ('conv3d_s1', 'conv3d_s2', 'deconv3d', 'cost_conv'):
    bn = _bn_module(lin, 3)
    if fam == 'cost_conv':
      fr, ft, d4 = d(lin.tensors['ref']), d(lin.tensors['tgt']), case.shape[3]
      return [('', bn, lambda relu, add: HF.cost_conv_bn_eval(fr, ft, w, d4, bn, relu))]
    x = d(lin.role.a)
    if fam == 'deconv3d':
      return [('', bn, lambda relu, add: HF.deconv3d_bn_eval(x, w, bn, add, relu))]
    stride = 1 if fam == 'conv3d_s1' else 2
    return [('', bn, lambda relu, add: HF.conv3d_bn_eval(x, w, bn, stride, add, relu))]
  if fam == 'conv2d':
    bn, x, dil = _bn_module(lin, 2), d(lin.role.a), case.shape[5]
    return [('', bn, lambda relu, add: HF.conv2d_bn_eval(x, w, bn, dil, add, relu))]
  if fam == 'conv2d_gen':
    from models import stage3d
    B, Ci, Co, H, W, k, stride, pad = case.shape
    conv = torch.nn.Conv2d(Ci, Co, k, stride, pad, bias=False).to(DEV)
    with torch.no_grad():
      conv.weight.copy_(w)
    bn, x = _bn_module(lin, 2), d(lin.role.a)
    seq = torch.nn.Sequential(conv, bn).eval()
    return [('', bn, lambda relu, add: stage3d.conv_bn(seq, x, relu, add))]
  from models.basic import SphereConv
  from models.basic.spherical_conv import sphere_conv as sc
  if fam == 'sphere':
    ih, iw, B, ci, co, g = case.shape
    typ, stride = 'Cassini', 1
  else:
    typ, ih, iw, B, ci, co, g, stride = case.shape
  m = SphereConv(ih, iw, typ, ci, co, 3, stride, 1, 1, g, False).to(DEV)
  assert torch.equal(m.position.cpu(), lin.tensors['pos'])  # the module's table is the reference's
  with torch.no_grad():
    m.weight.copy_(w)
  x = d(lin.tensors['x'])
  bn = _bn_module(lin, 2)
  out = [('NCHW caller', bn, lambda relu, add: m.forward_bn(x, bn, add, relu))]
  if fam == 'sphere':
    assert m.supports_transposed_io(B, x.device), S.eval_case_id(case)
    bn_t, xt = _bn_module(lin, 2), HF.transpose_planes(x)

    def run_t(relu, add):
      with sc.transposed_io():
        yt = m.forward_bn(xt, bn_t, HF.transpose_planes(add) if add is not None else None, relu)
      return HF.transpose_planes(yt)

    out.append(('transposed storage', bn_t, run_t))
  return out


def _doubled(lin):
  """The EvalLin of the same case after bn.weight.mul_(2): every folded quantity doubles exactly (a power of two)."""
  return lin._replace(gamma=lin.gamma * 2, s32=lin.s32 * 2, s64=lin.s64 * 2, wf=lin.wf * 2, lin64=lin.lin64 * 2, lin_den=lin.lin_den * 2,
                      emu_lin={k: v * 2 for k, v in lin.emu_lin.items()}, folded64=lin.folded64 * 2)


def _check_tag(entry, y, tag):
  am = HF.known_abs_max(y)
  if entry in WRITES_MAXIMUM:
    assert am is not None, tag
    assert HF.abs_max_value(am) == float(y[torch.isfinite(y)].abs().max()), tag
  else:
    assert am is None, tag


def _ran(recorder, case, entry):
  names = [n for n in recorder.names if n.startswith(COMPUTE)]
  if case.family == 'cost_conv':
    names = [n for n in names if n != TAP_PRODUCTS]
  return names


def _judge(case, lin, relu, with_add, got, line):
  ref = S.eval_reference(case, lin, relu, with_add)
  whole, worst, rest = S.measure(case, lin.role, ref, got)
  print(line + ' | T %.3f | rms %.3f | worst slice %.3f (axis %d @ %d)%s' %
        (ref.T, whole, worst.rms, worst.axis, worst.index, '' if rest is None else ' | columns past the contract, not judged: rms %.2f' % rest))
  return (whole <= ref.T and worst.rms <= ref.T), ('T %.3f' % ref.T, 'rms %.3f' % whole, worst)


CASES = [c for c in S.EVAL_CASES if c.shape != S.TALL]

# FINDINGS (kept in, strict: a variant listed here that starts to meet T fails the test until it is taken out; any OTHER variant of these
# cases that misses T fails as usual; the call after gamma x 2 carries the same figures and is held the same way).  All four are the
# 64-input-channel reductions (1728 terms in 3-D, 576 in 2-D) on the six-decades data, all miss in their worst CHANNEL only, and in all of
# them the fp32 kernel of the same layer (CONV_ARITH = 'f32': exact products, no split arithmetic at all) is at or over 0.85 T on the same
# inputs and peaks on the same channel, while torch's blocked fp32 sum on the host has the same profile at a third of the level.  Worst
# channel: own entry / fp32 kernel / host fp32, against T (whole-tensor rms of the own entry in brackets):
#   A  conv3d_fwd_split, 64 -> 32, 4 x 8 x 32        relu, add: channel 2: 0.954 / 0.846 / 0.211, T 0.640 (0.429; median channel 0.361)
#                                                    plain:     channel 2: 0.955 / 0.850 / under 0.205 (the host's worst there: channel 19 at 0.225), T 0.916 (0.587)
#   B  conv3d_fwd_split_f16_bn, the same layer       relu, add: channel 2: 0.189 / 0.212 / 0.052, T 0.137 (0.083) -- units of 2^-22; the
#                                                    plain variant PASSES: 0.188 against T 0.189 (fp32 kernel 0.213)
#   C  conv2d_fwd_split_f16_bn, 64 -> 64, dilation 2 relu, add: channel 0: 0.195 / 0.215 / 0.103, T 0.177 (0.096); plain passes: 0.193 / 0.263
#      (the three-piece entry on the same inputs passes: channel 21 at 1.003 of T 1.155; fp32 kernel 0.829, host 0.378)
# The excess is fp32 ACCUMULATION, as in the two findings of tests/test_gpu_split_precision.py: on non-negative data (relu) a channel whose
# weights do not sum to ~0 has partial sums that grow with the term count, every addition rounds at their size, and a running sum is
# noisier there than a blocked one.  ReLU in the store then halves the mutants' signal (T falls from 0.916 to 0.640 in A) but not the noise
# of the channel's positive outputs, which is why the (relu, add) variants miss first.  The host tier's condition holds for all four, so
# the reductions are not shortened; the SAME entries on the same kind of data pass at 8, 16 and 32 input channels (216 - 864 terms; 3 x 3:
# 144 - 288), and that is where their six-decades contract is asserted.
KNOWN = {
    ('conv3d_s1-1x64x32x4x8x32-split-bf16x6-six_decades_along_a_row-zero_shift', 'relu 1 add 1'): 'KNOWN-A',
    ('conv3d_s1-1x64x32x4x8x32-split-bf16x6-six_decades_along_a_row-zero_shift', 'relu 0 add 0'): 'KNOWN-A',
    ('conv3d_s1-1x64x32x4x8x32-f16-f16x3-six_decades_along_a_row-zero_shift', 'relu 1 add 1'): 'KNOWN-B',
    ('conv2d-1x64x64x12x32x2-f16-f16x3-six_decades_along_a_row-zero_shift', 'relu 1 add 1'): 'KNOWN-C',
}


@pytest.mark.parametrize('case', CASES, ids=S.eval_case_id)
def test_eval_entry_keeps_the_componentwise_contract(case, switches, recorder):
  _set_route(case)
  lin = S.eval_linear(case)
  lin2 = _doubled(lin)
  entry = _entry_of(case)
  shape = 'x'.join(str(v) for v in case.shape)
  missed, expected_misses = [], []

  def record(ok, tag, figures):
    known = KNOWN.get(tag[:2])
    if known is not None:
      assert not ok, (tag, 'this variant now meets T: take it out of KNOWN', figures)
      expected_misses.append(known)
    elif not ok:
      missed.append(tag + figures)

  with torch.no_grad():
    for relu, with_add in case.epilogues:
      add = lin.add.to(DEV) if with_add else None
      for label, bn, run in _runners(case, lin):
        tag = (S.eval_case_id(case), 'relu %d add %d' % (relu, with_add), label)
        line = 'EVALPREC | %s | %s | %s | %s | %s | %s | relu %d add %d %s | %s' % (case.family, shape, case.route, case.arith, case.kind, case.bn, relu,
                                                                              with_add, label, entry)
        del recorder.names[:]
        y1 = run(relu, add)
        torch.cuda.synchronize()
        assert _ran(recorder, case, entry) == [entry], (tag, recorder.names)
        assert 'mode_weight_pack_reuse' not in recorder.names, tag  # a fresh module: packed here
        _check_tag(entry, y1, tag)
        ok, figures = _judge(case, lin, relu, with_add, y1, line)
        record(ok, tag, figures)
        # the kept pack: a hit, the same bits
        del recorder.names[:]
        y2 = run(relu, add)
        torch.cuda.synchronize()
        assert _ran(recorder, case, entry) == [entry], (tag, recorder.names)
        if entry not in NO_KEPT_PACK:
          assert 'mode_weight_pack_reuse' in recorder.names, (tag, 'the second call did not hit the packed-weight cache')
        assert torch.equal(y1, y2), (tag, 'the call on the kept pack differs', float((y1 - y2).abs().max()))
        _check_tag(entry, y2, tag)
        # ... and not a stale one: the BatchNorm scale doubled in place -> within T of the new reference
        bn.weight.mul_(2)
        y3 = run(relu, add)
        torch.cuda.synchronize()
        ok, figures = _judge(case, lin2, relu, with_add, y3, line + ' | gamma x 2')
        record(ok, tag, ('gamma x 2',) + figures)
        _check_tag(entry, y3, tag)
  assert not missed, missed
  if expected_misses:
    pytest.xfail('; '.join(sorted(set(expected_misses))))


def test_the_tall_tile_eval_form_keeps_the_contract_and_the_order_of_the_8_row_tile(switches, recorder):
  """conv3d_split_kernel<MT, 1, true, 16, true> (csrc/conv3d_split.hip, conv3d_s1_split): the 16-row tile with shift epilogue and maximum --
  the form every stride-1 3-D layer without a residual takes in a real inference forward.  It is chosen when the fp16 arithmetic is on,
  there is no residual, H % 16 == 0 and B cdiv(D, 2) (H / 8) cdiv(W, 32) >= 4 x 256.  8 -> 8 at 1 x 15 x 64 x 500 meets it exactly:
  cdiv(15, 2) (64 / 8) cdiv(500, 32) = 8 x 8 x 16 = 1024 tiles, with a ragged W and an odd D.  Asserted: the residual-free result is within T,
  carries the exact maximum, and is bit-identical to the same call with a ZERO residual, which forces the 8-row EPI 2 form -- the same sums
  in the same order (the device of tests/test_gpu_f16.py::test_the_16_row_tile_is_the_8_row_tile_bit_for_bit)."""
  case = next(c for c in S.EVAL_CASES if c.shape == S.TALL)
  B, Ci, Co, D, H, W = case.shape
  assert H % 16 == 0 and B * -(-D // 2) * (H // 8) * -(-W // 32) == 4 * 256
  _set_route(case)
  lin = S.eval_linear(case)
  entry = _entry_of(case)
  (relu, with_add), = case.epilogues
  assert not with_add
  with torch.no_grad():
    (label, bn, run), = _runners(case, lin)
    del recorder.names[:]
    y = run(relu, None)
    torch.cuda.synchronize()
    assert _ran(recorder, case, entry) == [entry], recorder.names
    _check_tag(entry, y, 'tall')
    ok, figures = _judge(case, lin, relu, False, y, 'EVALPREC | conv3d_s1 | %s | f16 | f16x3 | %s | %s | relu %d add 0 tall tile | %s' %
                         ('x'.join(str(v) for v in case.shape), case.kind, case.bn, relu, entry))
    assert ok, figures
    y8 = run(relu, torch.zeros_like(y))
    torch.cuda.synchronize()
    assert torch.equal(y, y8), float((y - y8).abs().max())
    _check_tag(entry, y8, 'tall, zero residual')
