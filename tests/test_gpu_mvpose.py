"""GPU (-m gpu): the gradient of the multi-view reprojection loss to the sources' poses -- HF.mv_photometric_loss with a
pose tensor (csrc/mv_pose_grad.hip), ModeMultiView.fusion_selfsup_loss(poses=) and utils.rig_refine -- against the float64
restatement of tests/mvpose_ref.py.

The poses are generic (perturbed): tests/test_mvpose_host.py asserts on the restatement that no valid pixel of the four cases has u
or v within 1e-9 of an integer and that no window's runner-up is close, so win and N are exact and the gradient is the derivative
(at exactly rectified poses it is one-sided; include/mode_hip_mvpose.h).  gposes follows DESIGN 24's bound over all S x 12 elements:
the yardstick is the float32 restatement's own error against float64 (geometry in float64 in both, as in the kernel; relative to
max|g64|), never below one fp32 ulp, 2^-23; the kernel may take 4 times the yardstick.  Nothing is excluded.

Measured ratios on an MI355X: see DESIGN 27."""
import numpy as np
import pytest
import torch

import mvphoto_ref as M
import mvpose_ref as P

from mode_hip import functional as HF
from utils.rig import CameraRig
from utils.rig_refine import RigRefinement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['x'.join(str(v) for v in c) for c in P.CASES]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _run(ref, src, depth, poses, shape=None, factor=None, with_depth=False, **kw):
  """-> (loss, stats (3 + S,), win (F, H, W), gposes in the poses' shape, gdepth or None) on the CPU through the public entry."""
  pt = torch.from_numpy(np.asarray(poses, dtype=np.float64)).clone()
  pt = (pt if shape is None else pt.reshape(shape)).requires_grad_(True)
  d = depth.detach().to(DEV).requires_grad_(with_depth)
  loss, stats, win = HF.mv_photometric_loss(ref.to(DEV), src.to(DEV), d, pt, return_stats=True, return_win=True, **kw)
  assert loss.requires_grad and loss.is_cuda and loss.dim() == 0
  (loss if factor is None else loss * factor).backward()
  assert pt.grad.shape == pt.shape and pt.grad.dtype == torch.float64 and not pt.grad.is_cuda
  return loss.detach().cpu(), stats.cpu(), win.cpu(), pt.grad, (d.grad.cpu() if with_depth else None)


def _within(tag, got, a32, b64):
  """got within 4 x the yardstick of b64 over all elements; prints and returns the ratio."""
  yard, scale = P.yardstick(a32, b64)
  assert scale > 0 and bool(torch.isfinite(got).all()), tag
  err = P.error(got.reshape(b64.shape), b64, scale)
  print('  %s: max|g64| %.3e, error %.3e, yardstick %.3e of it, ratio %.2f' % (tag, scale, err, yard, err / yard))
  assert err <= 4 * yard, (tag, err, yard)
  return err / yard


def _check(tag, got, r32, r64):
  loss, stats, win, g, _ = got
  (_, i32, g32), (_, i64, g64) = r32, r64
  assert torch.equal(i32['win'], i64['win']), 'the case sits on a kink: float32 and float64 disagree on a winner'
  assert torch.equal(win, i64['win']), (tag, int((win != i64['win']).sum()))
  assert float(stats[0]) == i64['N']
  return _within(tag, g, g32, g64)


def _refs(ref, src, depth, poses, **kw):
  return P.evaluate(ref, src, depth, poses, torch.float32, **kw), P.evaluate(ref, src, depth, poses, torch.float64, **kw)


@pytest.mark.parametrize('case', P.CASES, ids=IDS)
def test_parity_with_the_float64_restatement(case):
  """The four cases (the first has F = 2); and the depth's gradient from the new Function is the old path's, bit for bit."""
  ref, src, depth, poses = P.make_case(*case)
  got = _run(ref, src, depth, poses, with_depth=True)
  _check('gposes %s' % (case,), got, P.reference(case, torch.float32), P.reference(case, torch.float64))
  assert float(got[1][0]) >= 0.95 * case[0] * case[1] * (case[2] - 2)
  d = depth.to(DEV).requires_grad_(True)
  old = HF.mv_photometric_loss(ref.to(DEV), src.to(DEV), d, poses)
  old.backward()
  assert torch.equal(old.detach().cpu(), got[0]) and torch.equal(d.grad.cpu(), got[4])


@pytest.mark.parametrize('alpha', [0.0, 1.0], ids=['l1', 'ssim'])
@pytest.mark.parametrize('case', [P.CASES[0], P.CASES[2]], ids=[IDS[0], IDS[2]])
def test_one_photometric_term_alone(case, alpha):
  ref, src, depth, poses = P.make_case(*case)
  c = P.conditions_of(ref, src, depth, poses, alpha=alpha, lam=0.0)
  assert c['same'] and c['gap'] > 100 * c['err'], c  # (the seeds were searched at the default alpha)
  got = _run(ref, src, depth, poses, alpha=alpha, lam=0.0)
  _check('alpha = %g' % alpha, got, P.reference(case, torch.float32, alpha=alpha, lam=0.0), P.reference(case, torch.float64, alpha=alpha, lam=0.0))


def test_the_smoothness_term_does_not_reach_the_poses():
  case = P.CASES[2]
  ref, src, depth, poses = P.make_case(*case)
  a = _run(ref, src, depth, poses, lam=0.0)
  b = _run(ref, src, depth, poses, lam=0.7)
  assert torch.equal(a[3], b[3]) and bool(a[3].any()) and not torch.equal(a[0], b[0])


def test_nothing_valid_gives_exact_zeros():
  """Every source so far away that every point lands beside its pole: N = 0 and gposes is all exactly zero."""
  case = P.CASES[2]
  ref, src, depth, poses = P.make_case(*case)
  far = poses.copy()
  far[:, 3] += 1e6
  loss, stats, win, g, _ = _run(ref, src, depth, far)
  assert float(stats[0]) == 0 and bool((win == 255).all()) and not bool(g.any()) and bool(torch.isfinite(loss))


def test_a_source_that_wins_nowhere_has_a_zero_row():
  """The second source shows an unrelated image (noise, 40 standard deviations brighter: its L1 term alone, 0.15 x 9, exceeds any pe
  of the others, <= 0.85 + 0.15) and loses every window: its row is exactly zero, the others match the restatement."""
  case = P.CASES[0]
  ref, src, depth, poses = P.make_case(*case)
  src = src.clone()
  src[:, 1] = torch.randn(src[:, 1].shape, generator=torch.Generator().manual_seed(17)) * 2.0 + 40.0
  r32, r64 = _refs(ref, src, depth, poses)
  assert int((r64[1]['win'] == 1).sum()) == 0 and int((r64[1]['win'] == 0).sum()) > 0 and int((r64[1]['win'] == 2).sum()) > 0
  got = _run(ref, src, depth, poses)
  _check('a loser among three', got, r32, r64)
  assert not bool(got[3][1].any()) and bool(got[3][0].any()) and bool(got[3][2].any())
  assert not bool(r64[2][1].any())


def test_eight_sources():
  ref, src, depth, _ = M.make_case(1, 40, 24, 3)
  g = torch.Generator().manual_seed(88)
  src = torch.cat([src, torch.randn(1, 5, 3, 40, 24, generator=g) * 0.5 + src[:, :1]], 1)
  poses = P.perturbed_poses(8, 0, sources=(1, 3, 5, 7, 9, 11, 6, 8))
  c = P.conditions_of(ref, src, depth, poses)
  assert c['same'] and c['gap'] > 100 * c['err'] and c['near'] > 1e-9, c
  got = _run(ref, src, depth, poses)
  _check('S = 8', got, *_refs(ref, src, depth, poses))
  assert bool((got[1][3:] > 0).all()) and bool(got[3].abs().amax(1).gt(0).all())  # every source wins somewhere and has a gradient


def test_spoilt_depths_cost_their_pixels_only():
  """NaN, +Inf, 0 and a negative depth at single pixels, corners included: a finite gradient within the bound."""
  case = P.CASES[0]
  ref, src, depth, poses = P.make_case(*case)
  depth = depth.clone()
  for f, h, w, bad in ((0, 3, 5, float('nan')), (0, 20, 10, 0.0), (1, 7, 7, -2.0), (1, 30, 20, float('inf')), (1, 0, 0, float('nan')),
                       (0, 39, 23, 0.0), (0, 0, 23, float('inf')), (1, 39, 0, -1.0)):
    depth[f, h, w] = bad
  r32, r64 = _refs(ref, src, depth, poses)
  assert bool(torch.isfinite(r64[2]).all())
  got = _run(ref, src, depth, poses)
  _check('spoilt depths', got, r32, r64)
  assert float(got[1][0]) < case[0] * case[1] * (case[2] - 2)


def test_the_pose_forms_two_calls_and_a_side_stream_are_bit_equal():
  case = P.CASES[3]
  ref, src, depth, poses = P.make_case(*case)
  a = _run(ref, src, depth, poses)
  b = _run(ref, src, depth, poses, shape=(case[3], 3, 4))
  assert b[3].shape == (case[3], 3, 4)
  side = torch.cuda.Stream(device=DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    c = _run(ref, src, depth, poses)
  side.synchronize()
  for x, y, z in zip(a[:4], b[:4], c[:4]):
    assert torch.equal(x, y.reshape(x.shape)) and torch.equal(x, z)


def test_a_gloss_other_than_one():
  case = P.CASES[1]
  ref, src, depth, poses = P.make_case(*case)
  got = _run(ref, src, depth, poses, factor=3.0)
  (_, _, g32), (_, _, g64) = P.reference(case, torch.float32), P.reference(case, torch.float64)
  _within('3 x loss', got[3], 3.0 * g32, 3.0 * g64)


def test_pose_tensors_it_cannot_take():
  ref, src, depth, poses = P.make_case(*P.CASES[1])
  args = (ref.to(DEV), src.to(DEV), depth.to(DEV))
  for bad in (torch.from_numpy(poses).float(), torch.from_numpy(poses).reshape(1, 2, 6), torch.from_numpy(poses).repeat(2, 1), torch.from_numpy(poses).to(DEV)):
    with pytest.raises(ValueError, match=r'float64 on the CPU, \(S, 12\) or \(S, 3, 4\)'):
      HF.mv_photometric_loss(*args, bad.requires_grad_(True))
  # without requires_grad every form runs as before, and carries no graph
  for form in (torch.from_numpy(poses), torch.from_numpy(poses).to(DEV), poses.tolist()):
    assert not HF.mv_photometric_loss(*args, form).requires_grad


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
def test_fusion_selfsup_loss_carries_the_gradient_to_the_twist(u8):
  """ModeMultiView(rig = pairs 12, 13) at 64 x 32 with poses = RigRefinement(rig)(): twist.grad is the chain rule applied to
  HF.mv_photometric_loss's pose gradient on the hand-assembled inputs, the masked entries are exactly zero, and poses=None is today's."""
  import test_gpu_rig as TR
  rig = CameraRig.deep360().subset(('12', '13'))
  net, maxdepth, H, W = TR._tiny_net(rig)
  frames_u8 = TR._u8_frames(2, 4, H, W, 61)
  normalised = TR._host_normalised(frames_u8)
  frames = frames_u8 if u8 else normalised
  net.train()
  net.disparity.eval()
  refine = RigRefinement(rig)
  with torch.no_grad():
    refine.twist.copy_((torch.rand(2, 6, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 2 - 1) * 0.004)
  loss, depth = net.fusion_selfsup_loss(frames, poses=refine(), lam=0.2)
  loss.backward()
  got = refine.twist.grad.clone()
  assert bool(torch.isfinite(loss)) and got.shape == (2, 6)
  assert not bool(got[refine.mask == 0].any()) and bool(got[1, :3].any())
  leaf = refine().detach()[[1, 3]].clone().requires_grad_(True)
  want = HF.mv_photometric_loss(normalised[:, 0], normalised[:, [1, 3]], depth, leaf, lam=0.2)
  assert torch.equal(loss.detach(), want.detach())
  want.backward()
  refine.twist.grad = None
  refine()[[1, 3]].backward(leaf.grad)
  assert torch.allclose(got, refine.twist.grad, rtol=1e-12, atol=0)
  # the (2P, 12) form, and poses=None
  flat, _ = net.fusion_selfsup_loss(frames, poses=refine().reshape(4, 12), lam=0.2)
  assert torch.equal(flat.detach(), loss.detach())
  today, depth0 = net.fusion_selfsup_loss(frames, lam=0.2)
  assert torch.equal(today.detach(), HF.mv_photometric_loss(normalised[:, 0], normalised[:, [1, 3]], depth0, rig.panorama_poses()[[1, 3]], lam=0.2))
  same, _ = net.fusion_selfsup_loss(frames, poses=rig.panorama_poses(), lam=0.2)
  assert torch.equal(same.detach(), today.detach())


# ----------------------------------------------------------------------------------------------- a run with a known answer
@pytest.mark.parametrize('source', [3, 7])
def test_calibration_finds_the_true_pose_of_a_sphere(source):
  """tests/test_mvpose_host.py's run on the kernels, with the same bounds: 100 Adam steps at 64 x 32, one source at a time."""
  def loss_of(ref, src, depth, poses):
    return HF.mv_photometric_loss(ref.float().to(DEV), src.float().to(DEV), depth.float().to(DEV), poses, lam=0.0)

  (r0, t0), (r1, t1) = P.known_answer(source, loss_of)
  print('source %d: rotation error %.4f -> %.4f, translation error %.4f -> %.4f' % (source, r0, r1, t0, t1))
  assert r0 > 0.005 and r1 < r0 / 5
  if source == 7:
    assert t0 > 0.02 and t1 < t0 / 5
  else:
    assert t0 == 0 and t1 == 0
