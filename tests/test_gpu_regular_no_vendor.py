"""ModeDisparity(conv='Regular') -- the PSMNet SPP extractor -- entirely on libmode_hip: no vendor-library operator in a training step
or an eval forward, every step bit-repeatable, and the golden vectors of a size whose pyramid is ragged.

The guard is mode_hip.no_vendor's list (convolutions, BatchNorm, matrix products, softmax, upsampling, grid sampling) EXTENDED here by
the pooling operators (`avg_pool`, `max_pool`, `adaptive_`): the spatial pyramid of this extractor used to be four nn.AvgPool2d, four
F.interpolate(mode='bilinear', align_corners=True) and a torch.cat; it now runs on csrc/spp.hip (HF.spp_pool / HF.spp_concat).  Before
that, the first test below stopped at aten.upsample_bilinear2d.

Sizes: the configuration of tests/golden/model_regular.npz (256 x 256, maxdisp 16, B = 2, recipe state; quarter-resolution plane
64 x 64: the k = 64 level is a single pixel), and 288 x 544 (tests/golden/model_regular_ragged.npz, made by make_golden_regular_ragged.py
from the imported reference): quarter-resolution plane 72 x 136, no multiple of 64 or of 16 in either axis -- 9 x 17 blocks at k = 8
against 4 x 8 at k = 16, 2 x 4 at k = 32, 1 x 2 at k = 64.  Every convolution of the network stays on the own kernels at 288 x 544 (the
guard would name one that does not), so no nearer size had to be chosen.

Arithmetic: the product's default (mode_hip.functional.CONV_ARITH = 'bf16x6', the split kernels).  The 320 -> 128 convolution behind
the pyramid is wider than the fp32 MFMA kernel's 128 channels; it has an own kernel on the split path only, so with the A/B
arithmetic 'f32' that one layer still runs in the vendor library and the guard says so.  The claim, and these tests, are for the
default."""
import contextlib
import json

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import recipe
from oracle import mode_ref

import models
import no_vendor
from mode_hip import functional as HF
from test_gpu_model import DISP_TOL, _check_disp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORBIDDEN = tuple(no_vendor.FORBIDDEN) + ('avg_pool', 'max_pool', 'adaptive_')


class _StrictGuard(TorchDispatchMode):
  """mode_hip.no_vendor._Guard with the longer list."""

  def __init__(self):
    super().__init__()
    self.seen = 0

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    name = str(func)
    if any(bad in name for bad in FORBIDDEN):
      raise AssertionError('vendor-library arithmetic on the path: %s' % name)
    self.seen += 1
    return func(*args, **(kwargs or {}))


@contextlib.contextmanager
def strictly_no_vendor():
  with _StrictGuard() as g:
    yield g


def _case(z):
  maxdisp, H, W, B, seed = [int(v) for v in z['cfg']]
  manifest = [(k, tuple(s)) for k, s in json.loads(str(z['manifest']))]
  left, right = recipe.recipe_images(B, H, W, seed + 1)
  gt = recipe.recipe_disparity(B, H, W, seed + 2, maxdisp)
  return maxdisp, manifest, seed, left.to(DEV), right.to(DEV), gt.to(DEV)


def _net(maxdisp, manifest, seed):
  net = models.ModeDisparity(maxdisp, 'Regular').to(DEV)
  assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == manifest
  net.load_state_dict(recipe.recipe_state(manifest, seed))
  return net


def _train_step(net, left, right, gt):
  net.train()
  preds = net(left, right)
  loss = mode_ref.training_loss(preds, gt, ~torch.isnan(gt))
  loss.backward()
  return preds, loss


def _bits(t):
  return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def test_regular_step_and_eval_forward_use_no_vendor_operator_and_repeat(golden):
  """A training step (forward, loss, backward) and an eval forward inside the strict guard; the training step twice from the same
  state: loss, every parameter gradient and every BatchNorm running statistic bit-equal."""
  assert HF.CONV_ARITH == 'bf16x6'
  maxdisp, manifest, seed, left, right, gt = _case(golden('model_regular.npz'))
  runs = []
  for _ in range(2):
    net = _net(maxdisp, manifest, seed)
    with strictly_no_vendor() as g:
      preds, loss = _train_step(net, left, right, gt)
      torch.cuda.synchronize()
    assert g.seen > 0 and bool(torch.isfinite(loss))
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert all(v is not None for v in grads.values())
    stats = {k: v for k, v in net.state_dict().items() if 'running_' in k or 'num_batches' in k}
    runs.append((loss, grads, stats))
  (loss_a, grads_a, stats_a), (loss_b, grads_b, stats_b) = runs
  assert torch.equal(_bits(loss_a), _bits(loss_b)), (float(loss_a), float(loss_b))
  differ = [k for k in grads_a if not torch.equal(_bits(grads_a[k]), _bits(grads_b[k]))]
  assert not differ, 'gradients differ between two identical steps: %s' % differ[:8]
  differ = [k for k in stats_a if not torch.equal(_bits(stats_a[k]), _bits(stats_b[k]))]
  assert not differ, 'BatchNorm statistics differ between two identical steps: %s' % differ[:8]
  net.eval()
  with torch.no_grad(), strictly_no_vendor() as g:
    pred = net(left, right)
    again = net(left, right)
  assert g.seen > 0 and pred.shape[-2:] == left.shape[-2:] and torch.equal(_bits(pred), _bits(again))


def test_regular_at_a_ragged_size_against_the_reference(golden):
  """288 x 544 (quarter plane 72 x 136) against the imported reference's golden vectors, inside the strict guard.

  Bounds as tests/test_gpu_model.py::test_regular_extractor_variant (same recipe state, same kind of fixture): the error against the
  float64 network is held against the reference's own fp32 error E_ref -- mean at most max(mean_floor, 2 x the reference's mean), with
  that test's mean_floor rule (DISP_TOL / 3 for the split-bf16 3x3 layers, the arithmetic here); max at most max(DISP_TOL,
  8 x E_ref).  The factor 8 is that test's and is not taken from this test's result: on this ill-conditioned fixture (random
  initialisation, round-off amplified ~10^3 x) the maximum over the pixels is one draw that equally exact evaluations move between 0.8
  and 4.0 x E_ref (documented there); 8 is twice that spread, and a wrong layer is an O(0.1 .. 1) px difference, > 200 x E_ref.
  Loss and per-parameter gradient sums: that test's tolerances."""
  z = golden('model_regular_ragged.npz')
  maxdisp, manifest, seed, left, right, gt = _case(z)
  assert tuple(left.shape[-2:]) == (288, 544)
  assert HF.CONV_ARITH == 'bf16x6'
  mean_floor = DISP_TOL / 3
  net = _net(maxdisp, manifest, seed)
  with strictly_no_vendor():
    preds, loss = _train_step(net, left, right, gt)
  e_ref = max(np.abs(z['train/pred%d' % i] - z['truth64/train_pred%d' % i]).max() for i in (1, 2, 3))
  for i, p in enumerate(preds):
    _check_disp('regular ragged train pred%d' % (i + 1), p[:, :, ::4, ::4], z['train/pred%d' % (i + 1)], z['truth64/train_pred%d' % (i + 1)], e_ref,
                mean_floor=mean_floor, max_factor=8.0)
  print('loss %.6f, reference %.6f' % (float(loss), float(z['train/loss'])))
  assert abs(float(loss.detach()) - float(z['train/loss'])) < 2e-4 * float(z['train/loss'])
  grads = dict(net.named_parameters())
  worst = max((abs(float(grads[str(n)].grad.double().abs().sum()) - s) / (5e-2 * s + 1e-4), str(n)) for n, s in zip(z['train/grad_names'], z['train/grad_abs_sum']))
  print('worst gradient sum: %.3f of its allowance (%s)' % worst)
  for n, s in zip(z['train/grad_names'], z['train/grad_abs_sum']):
    assert abs(float(grads[str(n)].grad.double().abs().sum()) - s) <= 5e-2 * s + 1e-4, str(n)
  sd = net.state_dict()
  for k in z.files:
    if k.startswith('bn/'):
      sd[k[3:]] = torch.from_numpy(z[k]).to(DEV)
  net.load_state_dict(sd)
  net.eval()
  with torch.no_grad(), strictly_no_vendor():
    pred = net(left, right)
  _check_disp('regular ragged eval pred3', pred[:, :, ::4, ::4], z['eval/pred3'], z['truth64/eval_pred3'],
              np.abs(z['eval/pred3'] - z['truth64/eval_pred3']).max(), mean_floor=mean_floor, max_factor=8.0)
