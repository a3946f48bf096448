"""GPU (-m gpu): HF.photometric_loss (csrc/photometric.hip) against the float64 restatement of tests/photometric_ref.py, and
its entries on ModeDisparity and ModeMultiView.

The yardstick of the parity test is the restatement's own float32 error against float64, computed here on the CPU: the kernel's
error on the loss and on the gradient (max over elements, relative to max|g64|) may be at most 4 times that -- two bits for the
different association of the nine-term window sums and of the reduction.  Nothing is excluded from the comparison.

Measured on an MI355X (kernel error / yardstick, loss and worst map's gradient): see DESIGN 22."""
import pytest
import torch

import photometric_ref as R

import models
from mode_hip import functional as HF
from utils.rig import CameraRig

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['x'.join(str(v) for v in c) for c in R.CASES]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _run(case_or_inputs, want_grad=True, **kw):
  """-> (loss, stats (K, 3), [gdisp_k]) on the CPU."""
  left, right, disps = R.make_case(*case_or_inputs) if len(case_or_inputs) == 5 else case_or_inputs
  ds = [d.to(DEV).requires_grad_(want_grad) for d in disps]
  weights = kw.pop('weights', R.WEIGHTS[:len(ds)])
  loss, stats = HF.photometric_loss(left.to(DEV), right.to(DEV), ds, weights, return_stats=True, **kw)
  if want_grad:
    loss.backward()
  return loss.detach().cpu(), stats.cpu(), [d.grad.cpu() if want_grad else None for d in ds]


def _parity(case, tag, **kw):
  l64, s64, g64 = R.reference(case, torch.float64, **kw)
  l32, s32, g32 = R.reference(case, torch.float32, **kw)
  loss, stats, grads = _run(case, **kw)
  assert torch.equal(stats[:, 0], s64[:, 0]), (stats[:, 0], s64[:, 0])
  yl = abs(float(l32) - float(l64))
  el = abs(float(loss.double()) - float(l64))
  print('%s %s: loss %.9g, error %.3e, yardstick %.3e, ratio %.2f' % (tag, case, float(loss), el, yl, el / yl))
  worst = 0.0
  for k, (g, a, b) in enumerate(zip(grads, g32, g64)):
    scale = float(b.abs().max())
    yg = float((a.double() - b).abs().max()) / scale
    eg = float((g.double() - b).abs().max()) / scale
    worst = max(worst, eg / yg)
    print('  map %d: max|g64| %.3e, gradient error %.3e, yardstick %.3e of it, ratio %.2f' % (k, scale, eg, yg, eg / yg))
  # photo and smooth one by one: fp64 means of fp32 terms whose ten or so operations each round to 2^-24, so 1e-5 of the float64 value
  for j in (1, 2):
    assert float((stats[:, j] - s64[:, j]).abs().max()) <= 1e-5 * float(s64[:, j].abs().max())
  assert el <= 4 * yl, (el, yl)
  assert worst <= 4, worst


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_parity_with_the_float64_restatement(case):
  _parity(case, 'parity')


@pytest.mark.parametrize('name,case,kw', [
    ('warp_l1', R.CASES[0], dict(alpha=0.0, lam=0.0)),
    ('ssim', R.CASES[2], dict(alpha=1.0, lam=0.0)),
], ids=['warp_l1', 'ssim'])
def test_the_pieces_alone(name, case, kw):
  _parity(case, name, **kw)


def test_smoothness_alone():
  """lam = 1 with all weight on the smoothness term: every disparity is moved outside the field of view (d + W + 5), so no window is
  valid, the photometric term is exactly zero and the loss and its gradient are those of the edge-aware smoothness alone."""
  case = R.CASES[1]
  left, right, disps = R.make_case(*case)
  W = case[2]
  disps = [d + (W + 5) for d in disps]
  wts = R.WEIGHTS[:len(disps)]
  ds64 = [d.double().requires_grad_(True) for d in disps]
  l64, s64 = R.photometric_loss(left, right, ds64, wts, lam=1.0)
  g64 = torch.autograd.grad(l64, ds64)
  ds32 = [d.clone().requires_grad_(True) for d in disps]
  l32, _ = R.photometric_loss(left, right, ds32, wts, lam=1.0)
  g32 = torch.autograd.grad(l32, ds32)
  l64, l32 = l64.detach(), l32.detach()
  loss, stats, grads = _run((left, right, disps), lam=1.0)
  assert int(stats[0, 0]) == int(s64[0, 0]) == 0 and float(stats[0, 1]) == 0 and float(s64[0, 2]) > 0
  yl, el = abs(float(l32) - float(l64)), abs(float(loss.double()) - float(l64))
  print('smoothness: loss %.9g, error %.3e, yardstick %.3e, ratio %.2f' % (float(loss), el, yl, el / yl))
  for g, a, b in zip(grads, g32, g64):
    scale = float(b.abs().max())
    yg, eg = float((a.double() - b).abs().max()) / scale, float((g.double() - b).abs().max()) / scale
    print('  gradient error %.3e, yardstick %.3e, ratio %.2f' % (eg, yg, eg / yg))
    assert eg <= 4 * yg
  assert el <= 4 * yl


def test_edges_forward():
  B, H, W, K, maxd = R.CASES[0]
  left, right, disps = R.make_case(B, H, W, 1, maxd)
  w = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
  # x == 0 and x == W - 1 exactly, everywhere: every pixel valid, Rh = R[h, 0] and R[h, W - 1]
  for d in (w.clone(), w - (W - 1)):
    loss, stats, _ = _run((left, right, [d]), want_grad=False)
    l64, s64 = R.photometric_loss(left, right, [d.double()], R.WEIGHTS[:1])
    assert int(stats[0, 0]) == int(s64[0, 0]) == B * H * (W - 2)
    assert abs(float(loss) - float(l64)) <= 1e-6 * abs(float(l64))
  # outside the field of view everywhere: nothing valid, photo = 0, a finite loss, and without smoothness a gradient of exact zeros
  d = torch.full((B, H, W), W + 5.0)
  loss, stats, _ = _run((left, right, [d]), want_grad=False)
  assert int(stats[0, 0]) == 0 and float(stats[0, 1]) == 0 and bool(torch.isfinite(loss))
  loss, stats, (g,) = _run((left, right, [d]), lam=0.0)
  assert float(loss) == 0 and bool((g == 0).all())
  # a NaN disparity makes its pixel invalid and nothing else
  d = disps[0].clone()
  d[0, 7, 9] = float('nan')
  loss, stats, _ = _run((left, right, [d]), want_grad=False, lam=0.0)
  l64, s64 = R.photometric_loss(left, right, [d.double()], R.WEIGHTS[:1], lam=0.0)
  assert bool(torch.isfinite(loss)) and int(stats[0, 0]) == int(s64[0, 0])
  assert int(stats[0, 0]) < int(R.reference((B, H, W, 1, maxd), torch.float64)[1][0, 0])
  assert abs(float(loss) - float(l64)) <= 1e-6 * abs(float(l64))


@pytest.mark.parametrize('shift', [1, 33])
def test_rolling_the_rows_rolls_the_gradient(shift):
  """H is periodic: the loss has no seam, and the per-pixel arithmetic does not depend on where a pixel lies in its tile."""
  case = R.CASES[3]
  left, right, disps = R.make_case(*case)
  loss, stats, grads = _run(case)
  rl, rs, rg = _run((left.roll(shift, 2), right.roll(shift, 2), [d.roll(shift, 1) for d in disps]))
  for a, b in zip(grads, rg):
    assert torch.equal(a.roll(shift, 1), b)
  assert torch.equal(stats[:, 0], rs[:, 0])
  assert float(((stats - rs).abs() / stats.abs()).max()) <= 1e-12  # fp64 sums in another order
  assert abs(float(rl) - float(loss)) <= 2.0 ** -22 * abs(float(loss))  # the fp32 rounding of such a sum


def test_repeatable_on_any_stream():
  case = R.CASES[3]
  first = _run(case)
  second = _run(case)
  side = torch.cuda.Stream(DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    third = _run(case)
  side.synchronize()
  for other in (second, third):
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    for a, b in zip(first[2], other[2]):
      assert torch.equal(a, b)


def _tiny_disparity():
  import test_gpu_multiview as M
  maxdisp, H, W, sd = M._disparity_state('model_wc_tiny.npz')
  assert (maxdisp, H, W) == (16, 64, 32)
  net = models.ModeDisparity(maxdisp, 'Sphere', H, W, 'Cassini').to(DEV)
  net.load_state_dict(sd)
  return net.train(), maxdisp, H, W


def _grads(module):
  return {k: (None if p.grad is None else p.grad.clone()) for k, p in module.named_parameters()}


def test_mode_disparity_trains_without_ground_truth():
  import recipe
  from models import stage3d
  from no_vendor import no_vendor_arithmetic
  net, maxdisp, H, W = _tiny_disparity()
  left, right = [t.to(DEV) for t in recipe.recipe_images(2, H, W, 311)]
  with no_vendor_arithmetic():
    loss, preds = net.forward_photometric_loss(left, right)
    loss.backward()
  assert loss.dim() == 0 and bool(torch.isfinite(loss)) and len(preds) == 3 and preds[2].shape == (2, 1, H, W)
  got = _grads(net)
  for k, g in got.items():
    assert g is not None and bool(torch.isfinite(g).all()), k
  assert any(bool(g.abs().max() > 0) for g in got.values())
  net.zero_grad(set_to_none=True)
  size = (maxdisp, H, W)
  by_hand = tuple(stage3d.head(c, size) for c in net._logits(left, right))
  want = HF.photometric_loss(left, right, by_hand, (0.5, 0.7, 1.0))
  want.backward()
  assert torch.equal(want, loss)
  for p, q in zip(preds, by_hand):
    assert torch.equal(p, q.detach()) and not p.requires_grad
  for k, g in _grads(net).items():
    assert torch.equal(g, got[k]), k


def test_mode_multiview_adapts_stage_one_to_a_rig():
  import test_gpu_rig as TR
  rig = CameraRig.deep360().subset(('12', '13', '23'))
  net, maxdepth, H, W = TR._tiny_net(rig)
  assert (H, W) == (64, 32)
  with pytest.raises(RuntimeError, match='disparity.train'):
    net.photometric_loss(TR._u8_frames(1, 6, H, W, 5))
  net.train()
  u8 = TR._u8_frames(1, 6, H, W, 47)
  frames = TR._host_normalised(u8)
  left, right, _, _ = net._ingest(frames)
  want, preds = net.disparity.forward_photometric_loss(left, right)
  want.backward()
  ref = _grads(net.disparity)
  for src in (frames, u8):
    net.zero_grad(set_to_none=True)
    loss, disp = net.photometric_loss(src)
    loss.backward()
    assert torch.equal(loss, want) and torch.equal(disp, preds[2]) and disp.shape == (3, 1, H, W) and not disp.requires_grad
    for k, p in net.named_parameters():
      if k.startswith('fusion.'):
        assert p.grad is None, k
    got = _grads(net.disparity)
    assert all(g is not None for g in got.values())
    for k, g in got.items():
      assert torch.equal(g, ref[k]), k
