"""Float64 reference of the fusion network's gradients ON A RUN'S OWN DECISIONS (test infrastructure, host only).

The fusion network (oracle/fusion_ref.py) is piecewise linear between its BatchNorms: the sign of every ReLU input and the argmax
of every pooling window decide which piece an evaluation is on.  Two correct evaluations in different arithmetics can land on
different pieces -- one element out of 2e5 that lies within a rounding of its kink -- and their gradients then differ by a whole
term (3e-3 .. 1e-2 of a tensor at these sizes), which no choice of seeds excludes.  What CAN be held at rounding level: the backward
of a run is the exact derivative of the piece its forward was on.  So the reference here takes the decisions of the run under test
(fusion_ref.Decisions in replay mode), and reports its own free decisions beside them so that the test can bound how far from a kink
a differing decision lies.

Cases, recipe state, inputs and the two losses are the ones tests/test_fusion_grad_host.py (CPU) and tests/test_gpu_fusion_grad.py
(GPU) share."""
import collections
import json
import os

import numpy as np
import torch

import recipe
from make_golden_fusion import fusion_inputs
from oracle import fusion_ref

MAXDEPTH = 10.0
CHANNELS = [8, 16, 32, 64]
RECIPE_SEED = 77
PROBE_SEED = 7700

Case = collections.namedtuple('Case', 'name net B H W seed')
CASES = (
    Case('2x64x32', 'fusion', 2, 64, 32, 77),  # the existing fixture's size
    Case('1x24x32', 'fusion', 1, 24, 32, 77),  # deepest plane 3 x 4
    Case('1x8x32', 'fusion', 1, 8, 32, 77),  # deepest plane 1 x 4: BatchNorm statistics over four values
    Case('3x16x32', 'fusion', 3, 16, 32, 77),  # odd batch
    Case('1x24x40', 'fusion', 1, 24, 40, 78),  # deepest width 5: the first up-layer is not deconv2x2's
    Case('baseline 2x16x32', 'baseline', 2, 16, 32, 77),
)
FLIP_CASE = Case('1x24x40 seed 77', 'fusion', 1, 24, 40, 77)  # one decision of 202 080 differs between fp32 and fp64 (host regression only)
LOSSES = ('silog', 'linear')

# ConvTranspose2d biases in front of a train-mode BatchNorm: the BatchNorm removes the channel mean, their gradient is exactly zero
STRUCTURAL_ZEROS = tuple('feature_extraction.depth_layer%s.bias' % s for s in ('4.2', '5.1', '6.1'))

_MANIFESTS = {}


def manifest(net):
  """(key, shape) of the state_dict in its order: the fixture's for ModeFusion at CHANNELS, the module's own for Baseline."""
  if net not in _MANIFESTS:
    if net == 'fusion':
      z = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'), allow_pickle=False)
      assert [int(c) for c in z['cfg'][5:]] == CHANNELS and float(z['cfg'][0]) == MAXDEPTH and int(z['cfg'][4]) == RECIPE_SEED
      _MANIFESTS[net] = [(k, tuple(s)) for k, s in json.loads(str(z['manifest']))]
    else:
      from models import mode_fusion
      with torch.random.fork_rng():
        sd = mode_fusion.Baseline(MAXDEPTH).state_dict()
      _MANIFESTS[net] = [(k, tuple(v.shape)) for k, v in sd.items()]
  return _MANIFESTS[net]


def state(net):
  """The recipe's fp32 state_dict (tests/golden/recipe.py), seed RECIPE_SEED."""
  return recipe.recipe_state(manifest(net), RECIPE_SEED)


def inputs(case):
  """depthes (6), confs (6), rgbs (4), gt as make_golden_fusion.fusion_inputs draws them, from the stream seed + 1 as the fixture's
  own (make_golden_fusion.main; tests/test_fusion.py `_case`): seed 77 at 2 x 64 x 32 IS the fixture's input.  The baseline takes the
  depth maps only."""
  return fusion_inputs(case.B, case.H, case.W, case.seed + 1, MAXDEPTH)


def input_names(case):
  names = ['depth%d' % i for i in range(6)]
  return names if case.net == 'baseline' else names + ['conf%d' % i for i in range(6)] + ['rgb%d' % i for i in range(4)]


def probe(case):
  """The fixed R of the linear probe loss, (B, 1, H, W) fp32."""
  rs = np.random.RandomState(PROBE_SEED + case.seed)
  return torch.from_numpy(rs.standard_normal((case.B, 1, case.H, case.W)).astype(np.float32))


def loss_of(kind, pred, gt, R):
  """silog: the training loss of train_fusion.py (fusion_ref.training_loss).  linear: (pred * R).sum() / pred.numel()."""
  if kind == 'silog':
    return fusion_ref.training_loss(pred, gt, MAXDEPTH)
  assert kind == 'linear'
  return (pred * R).sum() / pred.numel()


Result = collections.namedtuple('Result', 'loss pred grads decisions pre taps')


def reference(case, loss, dtype, decisions=None, perturb=None):
  """One training-mode forward and backward of the oracle in `dtype` on the CPU.

  decisions: None -- a free run; a list as Result.decisions -- replayed.  perturb: relative size of a seeded perturbation of every
  floating-point weight (the conditioning probe).  Returns Result: the loss (float), the prediction, the gradients by name (every
  parameter, then the input maps of input_names), this run's own free decisions and the inputs of those calls, and the gradients at
  the three ConvTranspose outputs by the layer's prefix (fusion only)."""
  P = {}
  rs = np.random.RandomState(991)
  for k, v in state(case.net).items():
    if v.is_floating_point() and 'running' not in k:
      v = v.to(dtype)
      if perturb:
        v = v * (1 + perturb * torch.from_numpy(rs.standard_normal(tuple(v.shape))).to(dtype))
      P[k] = v.clone().requires_grad_(True)
    else:
      P[k] = v.to(dtype).clone() if v.is_floating_point() else v.clone()
  depthes, confs, rgbs, gt = inputs(case)
  leaf = lambda ts: [t.to(dtype).requires_grad_(True) for t in ts]
  depthes, confs, rgbs = leaf(depthes), leaf(confs), leaf(rgbs)
  dec = fusion_ref.Decisions(decisions)
  taps = {}
  if case.net == 'baseline':
    pred = fusion_ref.baseline(P, depthes, MAXDEPTH, True, dec)
    ins = depthes
  else:
    pred = fusion_ref.mode_fusion(P, depthes, confs, rgbs, MAXDEPTH, True, dec, taps)
    ins = depthes + confs + rgbs
  for t in taps.values():
    t.retain_grad()
  val = loss_of(loss, pred, gt.to(dtype), probe(case).to(dtype))
  val.backward()
  grads = collections.OrderedDict((k, v.grad) for k, v in P.items() if v.requires_grad)
  grads.update(zip(input_names(case), (t.grad for t in ins)))
  return Result(float(val.detach()), pred.detach(), grads, dec.made, dec.pre, {k: t.grad for k, t in taps.items()})


def rel_l2(got, want):
  """Relative L2 error over all entries of a tensor."""
  want = want.double()
  return float((got.detach().cpu().double() - want).norm()) / max(float(want.norm()), 1e-300)


def kink_distance(kind, pre):
  """How far each decision of a call lies from its kink, in units of the rms of the call's input `pre`: |v| / rms for a ReLU input;
  (top1 - top2) / rms per pooling window, (B, C, H/2, W/2).  (A window whose maximum is zero -- all four behind a closed ReLU -- has
  distance 0: its tie is broken by position, identically in every run that shares the ReLU decisions.)"""
  pre = pre.double()
  rms = max(float(pre.pow(2).mean().sqrt()), 1e-300)
  if kind == 'relu':
    return pre.abs() / rms
  B, C, H, W = pre.shape
  win = pre[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
  top = win.topk(2, -1).values
  return (top[..., 0] - top[..., 1]) / rms


def differing(mine, theirs, pre):
  """Decisions of `mine` (a run's) against `theirs` (the free decisions of the float64 run that replayed them; `pre` its inputs):
  (count of differing decisions, largest kink distance among them).  The call sequences must match."""
  assert [(k, tuple(d.shape)) for k, d in mine] == [(k, tuple(d.shape)) for k, d in theirs], 'the call sequences differ'
  count, far = 0, 0.0
  for (kind, a), (_, b), x in zip(mine, theirs, pre):
    ne = a != b
    n = int(ne.sum())
    if n:
      count += n
      far = max(far, float(kink_distance(kind, x)[ne].max()))
  return count, far


def preactivation_error(res, res64):
  """Largest |pre - pre64| / rms(pre64) over the ReLU and pooling inputs of two runs on the same decisions."""
  return max(float((a.double() - b).abs().max()) / max(float(b.pow(2).mean().sqrt()), 1e-300) for a, b in zip(res.pre, res64.pre))


def zero_ratio(name, grad, taps64):
  """|g|_inf / max_o sum |gy_o| of a structural-zero bias gradient: gy the float64 gradient at that ConvTranspose's output."""
  gy = taps64[name[:-len('.bias')]]
  return float(grad.detach().cpu().double().abs().max()) / float(gy.abs().sum((0, 2, 3)).max())


def bounds(own, K):
  """bound_t = K * max(own_t, median_t own) over the judged tensors."""
  med = float(np.median(list(own.values())))
  return {k: K * max(v, med) for k, v in own.items()}
