"""GPU (-m gpu): the fusion network's gradients against float64, tensor by tensor, ON THE RUN'S OWN DECISIONS.

ModeFusion / Baseline (models/mode_fusion.py) run one training step on the device -- forward, HF.silog_loss (what
ModeMultiView.fusion_loss uses) or a linear probe, backward -- with the depth, confidence and rgb maps as leaves, so that the first
layers' input gradients and every `cat` are on the path.  The signs of the ReLUs and the argmax of every pooling window are read off
the run (stage3d.conv_bn / stage3d.bn_act / HF.maxpool2x2 wrapped as models.mode_fusion calls them; the pool's argmax by torch's rule
on the host from the pool's input: the kernel's rule, tests/test_fusion.py::test_gpu_maxpool2x2_is_torchs), and the float64 oracle is
evaluated on THOSE decisions (tests/fusion_grad_ref.py): the run's backward must be the exact derivative of the piecewise-linear
function its forward evaluated, which holds at rounding level.  A free comparison does not: one ReLU of 202 080 that lands on the other
side of zero moves a BatchNorm bias gradient by 3e-3 .. 1e-2 (tests/test_fusion_grad_host.py keeps that case).

Asserted per case, loss and arithmetic (own_t: the fp32 oracle's error on the same decisions):
  * the call sequence is the oracle's; a decision that differs from the float64 run's own lies within tau of its kink, tau = 10 x the
    fp32 oracle's largest pre-activation error over rms (a differing decision far from a kink is a wrong forward);
  * the loss within 5 x the oracle's own loss error (floor 2^-22 relative; nine recorded misses, KNOWN below) -- and its two parts, for
    EVERY combination: the loss operator within 4 fp32 roundings of what it sums, against float64 on the run's own prediction, and the
    prediction's relative L2 error within 5 x the oracle's;
  * every parameter and every input map but the three structural zeros: relative L2 error <= K max(own_t, median_t own), and <= 1e-3
    whatever the arithmetic (the oracle alone stays <= 2.2e-4; one dropped term or flipped element shows as >= 2.5e-3);
  * the three structural zeros (ConvTranspose biases in front of a train-mode BatchNorm): |g|_inf / max_o sum|gy_o| within 5 x the
    fp32 oracle's;
  * the step run again returns the same bits for the loss and every gradient;
  * the entries that ran, by name and count: the fusion operators, the 1x1 GEMM behind deconv2x2, and all 38 (Baseline: 18) 3x3 layers
    on the package's entries in each of the three passes, those of the arithmetic among them.

Arithmetics: 'f32' (fp32 MFMA), 'bf16x6' with CONV2D_F16 off (three bf16 pieces, 24 bits), 'default' (two fp16 pieces in the forward
and input gradient of the 3x3 layers of a training step).  K = 5 on the two 24-bit arithmetics (the factor tests/test_gpu_parity.py
gives the reference's own error); K for the fp16 pieces: see K_F16 below.

All cases but two run forward and backward under no_vendor_arithmetic(): 1x24x40, whose deepest planes are 5 and 10 wide -- deconv2x2
needs W % 4 == 0, so the first TWO up-layers are the torch module and the third is deconv2x2, the dispatcher's mixed route in
mode_fusion._run -- and the Baseline under 'f32', whose 256-channel layers are beyond the fp32 kernels' 128 (HF._conv2d_own) and run as
the torch module by design (forward and input gradient of those three layers; the other 15 layers, and all 18 weight gradients, are
counted on the package's entries).  Those vendor convolutions are not bit-repeatable (the loss of two identical steps: 0.19216204 and
0.19216199), so the Baseline under 'f32' is also the one combination whose repeat is not asserted; 1x24x40 repeats and is held to it.

MEASURED (MI355X).  Per case and loss, for f32 / bf16x6 / default: the worst err_t / max(own_t, median own) over the judged tensors
(bound: K = 5), the largest err_t in units of 1e-5 (bound: 1e-3 = 100), and beside them the fp32 oracle's own worst tensor, the count of
decisions that differ from the float64 run's own with the farthest of them from its kink over tau, and the largest structural-zero
ratio as a multiple of the fp32 oracle's (bound: 5):

  case              loss    worst err/own       largest err (1e-5)   oracle   differing (of)          farthest / tau   zeros
  2x64x32           silog   2.06  1.97  2.04    3.04  3.02  3.01     2.85     0 0 0 (862 208)         -                1.0
  2x64x32           linear  1.34  1.41  1.70    3.27  3.00  3.52     3.70     0 0 0                   -                0.8
  1x24x32           silog   1.77  1.77  1.58    3.30  3.57  3.02     3.60     0 0 0 (161 664)         -                2.1
  1x24x32           linear  3.47  2.38  1.83    5.83  4.56  4.76     4.09     0 0 0                   -                1.7
  1x8x32            silog   2.15  2.01  2.53    5.89  5.52  6.93     4.45     0 0 0 (53 888)          -                3.0
  1x8x32            linear  1.66  1.45  2.00    8.22  7.80  12.1     12.1     0 0 0                   -                2.0
  3x16x32           silog   2.48  2.64  2.68    3.64  4.02  4.18     2.52     1 1 0 (323 328)         0.027            1.2
  3x16x32           linear  1.67  2.13  1.68    4.02  5.11  3.97     3.33     1 1 0                   0.027            1.0
  1x24x40           silog   1.27  1.22  1.12    4.31  2.57  2.42     3.96     0 0 0 (202 080)         -                1.7
  1x24x40           linear  1.43  1.37  1.85    2.87  2.55  3.46     4.26     0 0 0                   -                2.3
  baseline 2x16x32  silog   1.54  1.96  1.53    2.24  3.01  2.36     1.54     0 1 1 (1 572 864)       0.011            (none)
  baseline 2x16x32  linear  1.82  3.52  2.04    5.37  9.11  5.28     3.15     0 1 1                   0.011            (none)

K_F16: the two fp16 pieces stay inside K = 5 with the same room as the 24-bit arithmetics (worst 2.68 against 3.47 and 3.52), so K is
not raised.  tau is 4.4e-4 .. 8.0e-4 here (the fp32 oracle's pre-activation error 4.4e-5 .. 8.0e-5 of a tensor's rms); the three
differing decisions lie 5e-6 .. 1.7e-5 rms from their kinks.

KNOWN (the loss assertion, recorded misses: expected failures of that one assertion.  A listed combination must still miss -- one that
meets the bound fails the test until it is taken out -- and is held to twice its recorded error; everything else is asserted for these
combinations too, the two parts of the loss error included.)  The loss is ONE number: the
forward's rounding errors projected on one direction, so the fp32 oracle's own loss error is a single draw of a quantity that scatters
around zero -- it ranged from 2.2e-8 to 1.2e-5 over the twelve (case, loss) pairs -- and 5 x one draw bounds another draw of the SAME
distribution only with probability 1 - (2 / pi) atan(1 / 5) = 87 %: 4.5 misses of 36 are expected of a perfect implementation.  Nine
are seen.  What was checked for them: the run's prediction is as close to float64 as the oracle's (relative L2 1.00e-5 .. 1.38e-5
against 0.83e-5 .. 1.05e-5), and the float64 loss OF THE RUN'S OWN PREDICTION differs from the run's loss by at most 2.4e-7 (silog,
7.1 .. 8.3: one fp32 rounding of the result) / 4.9e-8 (linear) -- the loss operator adds nothing, the miss is the forward's rounding.
  case, loss, arithmetic              loss error   5 x the oracle's own
  2x64x32 linear f32                  1.51e-06     1.11e-07   (the oracle's draw, 2.2e-8, lies at the floor)
  2x64x32 linear bf16x6               1.09e-06     1.11e-07
  2x64x32 linear default              1.46e-06     1.11e-07
  1x24x32 silog bf16x6                9.97e-06     9.32e-06
  3x16x32 linear f32                  1.83e-06     9.68e-07
  3x16x32 linear bf16x6               1.88e-06     9.68e-07
  3x16x32 linear default              1.78e-06     9.62e-07
  baseline 2x16x32 silog f32          2.00e-05     1.41e-05
  baseline 2x16x32 silog default      1.76e-05     1.41e-05
"""
import collections
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fusion_grad_ref as G
from test_gpu_size_contracts import recorder  # noqa: F401  (the fixture that records the launching entries by name)

from mode_hip import functional as HF
from mode_hip import no_vendor
from models import mode_fusion, stage3d

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARITHS = ('f32', 'bf16x6', 'default')
K_24BIT = 5.0
K_F16 = 5.0  # (two fp16 pieces: may rise to at most 20 = 5 x 2^2 with a measured basis; 5 holds, see MEASURED)
CAP = 1e-3
SWITCHES = ('CONV2D_F16',)
# (case, loss, arithmetic) whose loss error exceeds 5 x the oracle's own draw -> the recorded error (KNOWN in the docstring).  An entry
# is an EXPECTED failure of that one assertion: it must still miss (else: take it out), and it is held to twice its recorded value.
# Every combination, listed or not, is held to the well-posed pair below the loss assertion: the loss operator's own error and the
# prediction's.
KNOWN = {
    ('2x64x32', 'linear', 'f32'): 1.51e-6, ('2x64x32', 'linear', 'bf16x6'): 1.09e-6, ('2x64x32', 'linear', 'default'): 1.46e-6,
    ('1x24x32', 'silog', 'bf16x6'): 9.97e-6,
    ('3x16x32', 'linear', 'f32'): 1.83e-6, ('3x16x32', 'linear', 'bf16x6'): 1.88e-6, ('3x16x32', 'linear', 'default'): 1.78e-6,
    ('baseline 2x16x32', 'silog', 'f32'): 2.09e-5, ('baseline 2x16x32', 'silog', 'default'): 1.76e-5,
}
KNOWN_CEILING = 2.0
LOSS_OP_ROUNDINGS = 4.0  # the loss operator: this many fp32 roundings (2^-24) of what the loss sums up (_loss_scale)
PRED_K = 5.0  # the prediction's relative L2 error: within this factor of the fp32 oracle's on the same decisions


def _loss_scale(loss, pred, gt, R):
  """The size of what a loss adds up -- its roundings scale with this, not with a result that cancels: mean |pred R| for the linear
  probe, mean(d^2) + lamda mean(d)^2 for silog (d = log pred - log gt over the selected elements, train_fusion.py:82-88)."""
  if loss == 'linear':
    return float((pred * R).abs().mean())
  m = gt <= G.MAXDEPTH
  o, g = torch.squeeze(pred, 1)[m], gt[m]
  m2 = (g > 0) * (o > 0)
  d = torch.log(o[m2]) - torch.log(g[m2])
  return float(d.pow(2).mean() + 0.5 * d.mean()**2)


@pytest.fixture
def switches():
  """The arithmetic switches of mode_hip.functional, restored after the case."""
  keep = (HF.CONV_ARITH,) + tuple(getattr(HF, n) for n in SWITCHES)
  yield
  HF.set_conv_arith(keep[0])
  for n, v in zip(SWITCHES, keep[1:]):
    setattr(HF, n, v)


def _set_arith(arith):
  if arith == 'f32':
    HF.set_conv_arith('f32')
  elif arith == 'bf16x6':
    HF.set_conv_arith('bf16x6')
    HF.CONV2D_F16 = False
  else:
    assert (HF.CONV_ARITH, HF.CONV2D_F16) == ('bf16x6', True)  # the default training step


def _guarded(case, arith):
  return not (case.name == '1x24x40' or (case.net == 'baseline' and arith == 'f32'))


def _repeatable(case, arith):
  """Bit for bit, wherever the 3x3 layers are the package's own (the vendor's 256-channel convolutions make no such promise)."""
  return not (case.net == 'baseline' and arith == 'f32')


def _record_decisions(monkeypatch, log):
  """Wrap the three calls through which models.mode_fusion reaches a ReLU or a pool; `log` receives ('relu', out > 0) and
  ('pool', the pool's input) on the host, in call order.  (conv_bn calls bn_act itself: the inner call is not a second ReLU.)"""
  conv_bn, bn_act, pool = stage3d.conv_bn, stage3d.bn_act, HF.maxpool2x2
  inside = [0]

  def conv_bn_rec(seq, x, relu=False, *a, **k):
    inside[0] += 1
    try:
      y = conv_bn(seq, x, relu, *a, **k)
    finally:
      inside[0] -= 1
    log.append(('relu' if relu else 'linear', (y.detach() > 0).cpu()))
    return y

  def bn_act_rec(bn, y, add=None, relu=False, *a, **k):
    out = bn_act(bn, y, add, relu, *a, **k)
    if not inside[0]:
      log.append(('relu' if relu else 'linear', (out.detach() > 0).cpu()))
    return out

  def pool_rec(x):
    log.append(('pool', x.detach().cpu()))
    return pool(x)

  monkeypatch.setattr(stage3d, 'conv_bn', conv_bn_rec)
  monkeypatch.setattr(stage3d, 'bn_act', bn_act_rec)
  monkeypatch.setattr(HF, 'maxpool2x2', pool_rec)


def _network(case):
  if case.net == 'baseline':
    net = mode_fusion.Baseline(G.MAXDEPTH)
  else:
    net = mode_fusion.ModeFusion(G.MAXDEPTH, G.CHANNELS, {'depth': 12, 'rgb': 12})
  net.load_state_dict(G.state(case.net))
  return net.to(DEV).train()


def _step(net, case, loss, guarded):
  """One training step from fresh leaves: (loss, {name: gradient}, prediction) on the device."""
  depthes, confs, rgbs, gt = G.inputs(case)
  leaf = lambda ts: [t.to(DEV).requires_grad_(True) for t in ts]
  depthes, confs, rgbs, gt = leaf(depthes), leaf(confs), leaf(rgbs), gt.to(DEV)
  R = G.probe(case).to(DEV)
  net.zero_grad(set_to_none=True)

  def run():
    pred = net(depthes) if case.net == 'baseline' else net(depthes, confs, rgbs)
    val = HF.silog_loss(pred, gt, gt <= G.MAXDEPTH, 0.5) if loss == 'silog' else (pred * R).sum() / pred.numel()
    val.backward()
    return val.detach(), pred.detach()

  if guarded:
    with no_vendor.no_vendor_arithmetic() as guard:
      val, pred = run()
    assert guard.seen > 0
  else:
    val, pred = run()
  grads = collections.OrderedDict((k, p.grad.detach().clone()) for k, p in net.named_parameters())
  ins = depthes if case.net == 'baseline' else depthes + confs + rgbs
  grads.update(zip(G.input_names(case), (t.grad.detach().clone() for t in ins)))
  return val, grads, pred


def _check_entries(case, arith, names):
  """The entries that ran in one step, by name: a route that goes elsewhere fails here instead of emptying the test."""
  n = collections.Counter(names)
  widths = [case.W // 8, case.W // 4, case.W // 2]
  pools = 5 if case.net == 'fusion' else 0
  ups = sum(w % 4 == 0 for w in widths) if case.net == 'fusion' else 0  # deconv2x2_supported: W % 4 == 0
  if case.net == 'fusion':
    assert ups == (1 if case.name == '1x24x40' else 3), (case, ups)
  want = {'mode_maxpool2x2_fwd': pools, 'mode_maxpool2x2_bwd': pools, 'mode_depth_to_space2': ups, 'mode_space_to_depth2': ups,
          'mode_conv1x1_sigmoid_fwd': 1, 'mode_conv1x1_sigmoid_bwd': 1,
          # the 1x1 GEMM behind deconv2x2: its forward is the GEMM's input-gradient entry, its input gradient the GEMM's forward entry
          'mode_conv1x1_bwd_data': ups, 'mode_conv1x1_fwd': ups, 'mode_conv1x1_bwd_weight': ups}
  got = {k: n[k] for k in want}
  assert got == want, (got, want)
  # the 3x3 layers: EVERY one of them on the package's kernels, all three passes (every input needs a gradient, the first layers' too) --
  # but the Baseline's three layers with 256 channels under 'f32', whose forward and input gradient are the vendor's (HF._conv2d_own;
  # the weight gradient is always the package's)
  layers = 38 if case.net == 'fusion' else 18
  own = layers - 3 if (case.net == 'baseline' and arith == 'f32') else layers
  c2 = sorted(k for k in n if k.startswith('mode_conv2d_'))
  passes = {p: sum(n[k] for k in c2 if k.startswith(p)) for p in ('mode_conv2d_fwd', 'mode_conv2d_bwd_data', 'mode_conv2d_bwd_weight')}
  assert passes == {'mode_conv2d_fwd': own, 'mode_conv2d_bwd_data': own, 'mode_conv2d_bwd_weight': layers}, (passes, c2)
  if arith == 'f32':
    assert c2 == ['mode_conv2d_bwd_data', 'mode_conv2d_bwd_weight', 'mode_conv2d_fwd'], c2
  elif arith == 'bf16x6':
    assert 'mode_conv2d_fwd_split' in c2 and 'mode_conv2d_bwd_weight_split' in c2 and any(k.startswith('mode_conv2d_bwd_data_split') for k in c2), c2
    assert not any('f16' in k for k in c2), c2
  else:
    assert 'mode_conv2d_fwd_split_f16' in c2 and 'mode_conv2d_bwd_data_split_f16' in c2 and 'mode_conv2d_bwd_weight_split_f16' in c2, c2
  return n


_TAU = {}  # case -> tau
_HOST = {}  # (case, loss, digest of the decisions) -> (float64 on them, fp32 on them)


def _tau(case):
  """10 x the fp32 oracle's own largest pre-activation error over rms (both runs on the float64 run's decisions; no loss enters)."""
  if case not in _TAU:
    r64 = G.reference(case, 'linear', torch.float64)
    r32 = G.reference(case, 'linear', torch.float32, r64.decisions)
    _TAU[case] = 10.0 * G.preactivation_error(r32, r64)
  return _TAU[case]


def _references(case, loss, decisions):
  """The float64 and the fp32 oracle on the given decisions, computed once per distinct set and left unchanged."""
  h = hashlib.sha1()
  for kind, d in decisions:
    h.update(kind.encode())
    h.update(np.ascontiguousarray(d.numpy()).tobytes())
  key = (case, loss, h.hexdigest())
  if key not in _HOST:
    _HOST[key] = (G.reference(case, loss, torch.float64, decisions), G.reference(case, loss, torch.float32, decisions))
  return _HOST[key]


@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('loss', G.LOSSES)
@pytest.mark.parametrize('case', G.CASES, ids=[c.name.replace(' ', '_') for c in G.CASES])
def test_gpu_fusion_gradients_on_own_decisions(case, loss, arith, switches, recorder, monkeypatch):
  _set_arith(arith)
  guarded = _guarded(case, arith)
  log = []
  _record_decisions(monkeypatch, log)
  net = _network(case)
  del recorder.names[:]
  val, grads, pred = _step(net, case, loss, guarded)
  names = list(recorder.names)
  _check_entries(case, arith, names)
  missed = []  # every figure is printed before anything is asserted on it

  # the run's decisions, and the two oracles on them
  decisions = [(kind, F.max_pool2d(t, 2, 2, return_indices=True)[1] if kind == 'pool' else t) for kind, t in log]
  assert all(kind in ('relu', 'pool') for kind, _ in decisions), [kind for kind, _ in decisions]
  r64, r32 = _references(case, loss, decisions)
  assert len(r64.decisions) == len(decisions)  # (the replay itself asserts kind and shape call by call)
  tau = _tau(case)
  differ, far = G.differing(decisions, r64.decisions, r64.pre)
  total = sum(d.numel() for _, d in decisions)
  if not far <= tau:
    missed.append('a decision differs %.2e rms from its kink (tau %.2e): a wrong forward' % (far, tau))

  # 1. the loss (beside it: the float64 loss of this run's own prediction, which tells the loss operator's error from the forward's)
  own_loss = max(abs(r32.loss - r64.loss), 2.0**-22 * abs(r64.loss))
  loss_err = abs(float(val) - r64.loss)
  gt64, R64 = G.inputs(case)[3].double(), G.probe(case).double()
  mid = float(G.loss_of(loss, pred.cpu().double(), gt64, R64))
  mid32 = float(G.loss_of(loss, r32.pred.double(), gt64, R64))
  print('LOSS %-16s %-6s %-7s %.9g, float64 %.9g: error %.2e = %.2e (loss operator) + %.2e (forward); oracle %.2e = %.2e + %.2e; prediction rel L2 %.2e, '
        'oracle %.2e' % (case.name, loss, arith, float(val), r64.loss, loss_err, abs(float(val) - mid), abs(mid - r64.loss), abs(r32.loss - r64.loss),
                         abs(r32.loss - mid32), abs(mid32 - r64.loss), G.rel_l2(pred, r64.pred), G.rel_l2(r32.pred, r64.pred)))
  recorded = KNOWN.get((case.name, loss, arith))
  if recorded is not None:
    print('KNOWN miss: loss error %.3e (recorded %.3e), 5 x the own error of the oracle %.3e' % (loss_err, recorded, 5.0 * own_loss))
    # (the Baseline under 'f32' does not repeat -- 1.86e-5, 2.00e-5, 2.09e-5 in three runs against 1.41e-5 -- so it may land either side)
    if loss_err <= 5.0 * own_loss and _repeatable(case, arith):
      missed.append('loss: error %.3e now meets 5 x the own error of the oracle %.3e: take this combination out of KNOWN' % (loss_err, 5.0 * own_loss))
    if not loss_err <= KNOWN_CEILING * recorded:
      missed.append('loss: error %.3e, a KNOWN miss recorded at %.3e' % (loss_err, recorded))
  elif not loss_err <= 5.0 * own_loss:
    missed.append('loss: error %.3e, 5 x the own error of the oracle %.3e' % (loss_err, 5.0 * own_loss))
  # the two parts of that error, each against a yardstick that is not one draw: the loss operator against float64 on the run's OWN
  # prediction, in roundings of what it sums; the prediction over all its entries against the oracle's
  op_err, op_bound = abs(float(val) - mid), LOSS_OP_ROUNDINGS * 2.0**-24 * _loss_scale(loss, pred.cpu().double(), gt64, R64)
  pred_err, pred_own = G.rel_l2(pred, r64.pred), G.rel_l2(r32.pred, r64.pred)
  print('LOSS parts: operator %.2e (bound %.2e), prediction %.2e (bound %.2e)' % (op_err, op_bound, pred_err, PRED_K * pred_own))
  if not op_err <= op_bound:
    missed.append('loss operator: %.3e from float64 on its own input, bound %.3e' % (op_err, op_bound))
  if not pred_err <= PRED_K * pred_own:
    missed.append('prediction: relative L2 error %.3e, %g x the own error of the oracle %.3e' % (pred_err, PRED_K, PRED_K * pred_own))

  # 2., 3. every judged tensor
  zeros = G.STRUCTURAL_ZEROS if case.net == 'fusion' else ()
  judged = [k for k in r64.grads if k not in zeros]
  assert set(grads) == set(r64.grads) and len(judged) == len(r64.grads) - len(zeros)
  own = {k: G.rel_l2(r32.grads[k], r64.grads[k]) for k in judged}
  err = {k: G.rel_l2(grads[k], r64.grads[k]) for k in judged}
  K = K_F16 if arith == 'default' else K_24BIT
  bound = G.bounds(own, K)
  ratio = {k: err[k] * K / bound[k] for k in judged}
  kr, ke = max(ratio, key=ratio.get), max(err, key=err.get)
  zr = [(k, G.zero_ratio(k, grads[k], r64.taps), G.zero_ratio(k, r32.grads[k], r64.taps)) for k in zeros]
  print('MEASURED %-16s %-6s %-7s worst err/own %.2f (%s) largest err %.2e (%s) oracle worst %.2e median %.2e | differing decisions %d of %d, '
        'farthest %.2e (tau %.2e) | zeros %s' % (case.name, loss, arith, ratio[kr], kr, err[ke], ke, max(own.values()), float(np.median(list(own.values()))),
                                                 differ, total, far, tau, ' '.join('%.2e/%.2e' % (a, b) for _, a, b in zr)))
  missed += ['%s: error %.3e, bound %.3e' % (k, err[k], min(bound[k], CAP)) for k in judged if not err[k] <= min(bound[k], CAP)]

  # 4. the structural zeros
  missed += ['%s: %.3e of the gradient it sums, the oracle %.3e' % z for z in zr if not z[1] <= 5.0 * z[2]]

  # 5. the whole step again: the same bits
  del log[:]
  val2, grads2, _ = _step(net, case, loss, guarded)
  assert len(log) == len(decisions)
  if _repeatable(case, arith):
    if not torch.equal(val, val2):
      missed.append('the loss does not repeat: %r, %r' % (float(val), float(val2)))
    missed += ['decisions of call %d do not repeat' % i for i, ((kind, t), (_, d)) in enumerate(zip(log, decisions)) if kind == 'relu' and not torch.equal(t, d)]
    missed += ['%s does not repeat' % k for k in grads if not torch.equal(grads[k], grads2[k])]
  assert not missed, missed
