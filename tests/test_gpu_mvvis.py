"""GPU (-m gpu): the z-buffer visibility masks of DESIGN 28 -- HF.mv_visibility (csrc/mv_visibility.hip), HF.mv_photometric_loss(masks=)
(the masked instantiation of csrc/mv_photometric.hip) and ModeMultiView.fusion_selfsup_loss(visibility=) -- against the float64
restatement of tests/mvvis_ref.py.

vis is exact: the kernel computes rho, u, v in fp64 as the restatement does, the minima are integer minima of the keys, and
tests/test_mvvis_host.py asserts on the restatement that no landing pixel, no edge of validity and no comparison with (1 + tol) zmin of
the cases sits within 1e-9 of its kink.  zbuf: the +inf pattern exactly, the finite values within one fp32 ulp (the kernel's fp64 rho
and the restatement's differ in their last bits, which the rounding to fp32 can carry over a tie).  The masked loss: win, N and the
wins per source exactly; loss and gdepth by DESIGN 24's bound -- the yardstick is the float32 restatement's own error against
float64 (max over ALL elements, relative to max|g64|), never below 2^-23 max|g64|, and the kernel may take 4 times it.

Measured ratios on an MI355X: see DESIGN 28."""
import numpy as np
import pytest
import torch

import mvphoto_ref as M
import mvpose_ref as P
import mvvis_ref as V

from mode_hip import functional as HF
from utils.rig import CameraRig

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['x'.join(str(v) for v in c) for c in V.CASES]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _vis(depth, poses, **kw):
  vis, zbuf = HF.mv_visibility(depth.to(DEV), poses, return_zbuf=True, **kw)
  assert vis.dtype == torch.uint8 and zbuf.dtype == torch.float32 and vis.is_cuda and zbuf.is_cuda and vis.shape == zbuf.shape
  assert not vis.requires_grad and not zbuf.requires_grad
  return vis.cpu(), zbuf.cpu()


def _one_ulp(got, want):
  """The +inf pattern exactly; finite values within one fp32 ulp (as integers, the bit patterns of positive floats are consecutive)."""
  inf = torch.isinf(want)
  assert torch.equal(torch.isinf(got), inf) and bool((got[inf] > 0).all()) and not bool(torch.isnan(got).any())
  steps = (got[~inf].view(torch.int32) - want[~inf].view(torch.int32)).abs()
  return int(steps.max()) if steps.numel() else 0


def _check_vis(tag, depth, poses, tol, radius, want=None):
  want = V.visibility(depth, poses, tol, radius) if want is None else want
  vis, zbuf = _vis(depth, poses, tol=tol, radius=radius)
  assert torch.equal(vis, want['vis']), (tag, tol, radius, int((vis != want['vis']).sum()))
  ulps = _one_ulp(zbuf, want['zbuf'])
  print('  %s tol %g radius %d: %d of %d visible, zbuf within %d ulp, %d target pixels empty' % (
      tag, tol, radius, int(vis.sum()), vis.numel(), ulps, int(torch.isinf(zbuf).sum())))
  assert ulps <= 1
  return vis, zbuf


# ---------------------------------------------------------------------------------------------------------------- the masks
@pytest.mark.parametrize('case', V.CASES, ids=IDS)
def test_masks_equal_the_float64_restatement(case):
  ref, src, depth, poses = V.make_case(*case)
  for tol in V.TOLS:
    for radius in V.RADII:
      vis, _ = _check_vis(str(case), depth, poses, tol, radius, V.reference_visibility(case, tol, radius))
      assert 0 < int(vis.sum()) < vis.numel()
  assert torch.equal(HF.mv_visibility(depth.to(DEV), poses).cpu(), V.reference_visibility(case)['vis'])  # the defaults: tol 0.05, radius 0


def test_spoilt_depths_are_never_visible_and_never_splat():
  """NaN, +Inf, 0 and a negative depth at single pixels, corners included: invalid for every source, so never visible; and their keys
  never reach a z-buffer: zbuf is the restatement's, which leaves them out."""
  case = V.CASES[0]
  ref, src, depth, poses = V.make_case(*case)
  depth = depth.clone()
  spots = ((0, 3, 5, float('nan')), (0, 20, 10, 0.0), (1, 7, 7, -2.0), (1, 30, 20, float('inf')), (1, 0, 0, float('nan')), (0, 39, 23, 0.0),
           (0, 0, 23, float('inf')), (1, 39, 0, -1.0))
  for f, h, w, bad in spots:
    depth[f, h, w] = bad
  c = V.exactness(depth, poses)
  assert c['land'] >= 1e-9 and c['edge'] >= 1e-9 and c['margin'] > 1e-9, c
  clean = V.reference_visibility(case, 0.05, 0)
  for radius in V.RADII:
    vis, zbuf = _check_vis('spoilt depths', depth, poses, 0.05, radius)
    for f, h, w, _ in spots:
      assert not bool(vis[f, :, h, w].any())
  # a spoilt pixel that held a z-buffer entry alone leaves it empty
  want = V.visibility(depth, poses, 0.05, 0)
  assert int(torch.isinf(want['zbuf']).sum()) >= int(torch.isinf(clean['zbuf']).sum())


def test_far_sources_see_nothing():
  """Every source translated 10^6 along its own x axis: every point lands beside its pole, nothing is valid."""
  case = V.CASES[2]
  ref, src, depth, poses = V.make_case(*case)
  far = poses.copy()
  far[:, 3] += 1e6
  for radius in V.RADII:
    vis, zbuf = _vis(depth, far, radius=radius)
    assert not bool(vis.any()) and bool((zbuf == float('inf')).all())


def test_eight_sources():
  poses = M.deep360_poses((1, 3, 5, 7, 9, 11, 6, 8))
  depth = V.smooth_depth(1, 40, 24)
  c = V.exactness(depth, poses)
  assert c['land'] >= 1e-9 and c['edge'] >= 1e-9 and c['margin'] > 1e-9, c
  for radius in V.RADII:
    vis, _ = _check_vis('S = 8', depth, poses, 0.05, radius)
    assert all(0 < int(vis[:, s].sum()) < vis[:, s].numel() for s in range(8))
  with pytest.raises(ValueError, match='source views'):
    HF.mv_visibility(depth.to(DEV), np.concatenate([poses, poses[:1]]))


def test_the_four_dimensional_layout_and_the_pose_forms():
  case = V.CASES[1]
  ref, src, depth, poses = V.make_case(*case)
  a = _vis(depth, poses)
  for d, p in ((depth.unsqueeze(1), torch.from_numpy(poses).reshape(-1, 3, 4)), (depth, poses.tolist()), (depth, torch.from_numpy(poses).to(DEV)),
               (depth.unsqueeze(1), torch.from_numpy(poses).clone().requires_grad_(True))):
    b = _vis(d, p)
    assert b[0].shape == (case[0], case[3], case[1], case[2]) and torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
  only = HF.mv_visibility(depth.to(DEV), poses)
  assert torch.is_tensor(only) and torch.equal(only.cpu(), a[0])
  for bad in (np.zeros((2, 13)), np.zeros(12), np.zeros((2, 4, 3))):
    with pytest.raises(ValueError, match=r'poses must be \(S, 12\) or \(S, 3, 4\)'):
      HF.mv_visibility(depth.to(DEV), bad)
  with pytest.raises(ValueError, match='tol'):
    HF.mv_visibility(depth.to(DEV), poses, tol=-0.1)
  with pytest.raises(ValueError, match='radius'):
    HF.mv_visibility(depth.to(DEV), poses, radius=2)


def test_two_calls_and_a_side_stream_are_bit_equal():
  case = V.CASES[3]
  ref, src, depth, poses = V.make_case(*case)
  a = _vis(depth, poses, radius=1)
  b = _vis(depth, poses, radius=1)
  side = torch.cuda.Stream(device=DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    c = _vis(depth, poses, radius=1)
  side.synchronize()
  for x, y, z in zip(a, b, c):
    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(x.view(torch.uint8), z.view(torch.uint8))


# ----------------------------------------------------------------------------------------------------------- the masked loss
def _run(ref, src, depth, poses, masks, **kw):
  """-> (loss, stats (3 + S,), win (F, H, W), gdepth) on the CPU through the public entry."""
  d = depth.detach().to(DEV).requires_grad_(True)
  m = None if masks is None else masks.to(DEV)
  loss, stats, win = HF.mv_photometric_loss(ref.to(DEV), src.to(DEV), d, poses, return_stats=True, return_win=True, masks=m, **kw)
  assert win.dtype == torch.uint8 and win.is_cuda and not win.requires_grad and stats.dtype == torch.float64 and loss.dim() == 0
  loss.backward()
  assert d.grad.shape == d.shape
  return loss.detach().cpu(), stats.cpu(), win.cpu(), d.grad.cpu()


def _within(tag, got, a32, b64, yardstick=M.yardstick, error=M.error):
  """got within 4 x the yardstick of b64 over all elements; prints and returns the ratio."""
  yard, scale = yardstick(a32, b64)
  assert scale > 0 and bool(torch.isfinite(torch.as_tensor(got)).all()), tag
  err = error(got, b64, scale)
  print('  %s: max|ref64| %.3e, error %.3e, yardstick %.3e of it, ratio %.2f' % (tag, scale, err, yard, err / yard))
  assert err <= 4 * yard, (tag, err, yard)
  return err / yard


def _all_nine(vis):
  """(F, S, H, W) masks -> (F, S, H, W) bool: the source sees all nine pixels of the window centred there (rows wrap, columns do not)."""
  v = vis != 0
  rows = v & torch.roll(v, 1, -2) & torch.roll(v, -1, -2)
  out = torch.zeros_like(rows)
  out[..., 1:-1] = rows[..., 1:-1] & rows[..., :-2] & rows[..., 2:]
  return out


@pytest.mark.parametrize('case', V.CASES, ids=IDS)
def test_masked_loss_parity_with_the_float64_restatement(case):
  F, H, W, S = case
  ref, src, depth, poses = V.make_case(*case)
  want = V.reference_visibility(case)
  masks = HF.mv_visibility(depth.to(DEV), poses)
  assert torch.equal(masks.cpu(), want['vis'])
  loss, stats, win, g = _run(ref, src, depth, poses, masks)
  (l32, i32, g32), (l64, i64, g64) = V.reference(case, torch.float32), V.reference(case, torch.float64)
  assert torch.equal(i32['win'], i64['win']), 'the case sits on a kink: float32 and float64 disagree on a winner'
  assert torch.equal(win, i64['win']), int((win != i64['win']).sum())
  assert float(stats[0]) == i64['N'] > 0.5 * F * H * (W - 2)
  for s in range(S):
    assert float(stats[3 + s]) == int((i64['win'] == s).sum()), s
  print('%s: loss %.9g, N %d, wins %s' % (case, float(loss), i64['N'], stats[3:].tolist()))
  _within('loss', loss, l32, l64)
  _within('gdepth', g.reshape(g64.shape), g32, g64)
  assert abs(float(stats[1]) - float(i64['photo'])) <= 1e-5 * abs(float(i64['photo']))
  # every masked winner sees its nine pixels, and an unmasked winner that sees its nine pixels stays the winner
  nine = _all_nine(want['vis'])
  plain = _run(ref, src, depth, poses, None)
  kept = 0
  for s in range(S):
    assert bool(nine[:, s][win == s].all()), s
    stays = (plain[2] == s) & nine[:, s]
    assert bool((win[stays] == s).all()), s
    kept += int(stays.sum())
  assert 0 < kept < int((plain[2] != 255).sum()) and float(stats[0]) < float(plain[1][0])


def test_all_ones_masks_are_the_unmasked_call():
  case = V.CASES[2]
  ref, src, depth, poses = V.make_case(*case)
  ones = torch.ones((case[0], case[3]) + case[1:3], dtype=torch.uint8)
  a = _run(ref, src, depth, poses, None)
  b = _run(ref, src, depth, poses, ones)
  c = _run(ref, src, depth, poses, ones * 255)  # read as != 0
  for x, y, z in zip(a, b, c):
    assert torch.equal(x, y) and torch.equal(x, z)
  assert float(a[1][0]) > 0 and bool(a[3].any())


def test_all_zero_masks_leave_the_smoothness_term():
  case = V.CASES[2]
  ref, src, depth, poses = V.make_case(*case)
  zeros = torch.zeros((case[0], case[3]) + case[1:3], dtype=torch.uint8)
  loss, stats, win, g = _run(ref, src, depth, poses, zeros)
  assert float(stats[0]) == 0 and float(stats[1]) == 0 and bool((win == 255).all()) and float(loss) > 0 and bool(g.any())
  loss, stats, win, g = _run(ref, src, depth, poses, zeros, lam=0.0)
  assert float(loss) == 0 and not bool(g.any()) and not bool(stats[:2].any()) and not bool(stats[3:].any()) and bool((win == 255).all())


def test_masks_it_cannot_take():
  case = V.CASES[1]
  ref, src, depth, poses = V.make_case(*case)
  args = (ref.to(DEV), src.to(DEV), depth.to(DEV), poses)
  ones = torch.ones((case[0], case[3]) + case[1:3], dtype=torch.uint8, device=DEV)
  for bad in (ones.bool(), ones.float(), ones[:, :, :-1], ones[0]):
    with pytest.raises(ValueError, match=r'masks must be a \(F, S, H, W\)'):
      HF.mv_photometric_loss(*args, masks=bad)
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    HF.mv_photometric_loss(*args, masks=ones.cpu())


def test_the_gradient_to_the_poses_under_masks():
  """A pose tensor that requires a gradient, masks from HF.mv_visibility of the same (detached) poses: gposes within 4 yardsticks of
  autograd through the masked float64 restatement, the bound of tests/test_gpu_mvpose.py; the depth's gradient comes along."""
  ref, src, depth, poses = V.make_pose_case()
  (l32, i32, g32, m32), (l64, i64, g64, m64) = V.reference_poses(torch.float32), V.reference_poses(torch.float64)
  pt = torch.from_numpy(poses).clone().requires_grad_(True)
  masks = HF.mv_visibility(depth.to(DEV), pt)
  assert torch.equal(masks.cpu(), m64) and torch.equal(i32['win'], i64['win'])
  d = depth.to(DEV).requires_grad_(True)
  loss, stats, win = HF.mv_photometric_loss(ref.to(DEV), src.to(DEV), d, pt, return_stats=True, return_win=True, masks=masks)
  loss.backward()
  assert torch.equal(win.cpu(), i64['win']) and float(stats[0]) == i64['N']
  assert pt.grad.shape == pt.shape and pt.grad.dtype == torch.float64 and not pt.grad.is_cuda
  _within('gposes under masks', pt.grad, g32, g64, P.yardstick, P.error)
  # the same masked loss with the poses as constants gives the same loss and the same gradient to the depth, bit for bit
  plain = _run(ref, src, depth, poses, masks)
  assert torch.equal(plain[0], loss.detach().cpu()) and torch.equal(plain[3], d.grad.cpu())


# ------------------------------------------------------------------------------------------------------------------ the model
def _grads_of(module):
  return {k: (None if p.grad is None else p.grad.clone()) for k, p in module.named_parameters()}


def test_fusion_selfsup_loss_with_visibility():
  """ModeMultiView(rig = pairs 12, 13) at 64 x 32 with disparity.eval(): visibility=True is HF.mv_photometric_loss with the masks of
  HF.mv_visibility(depth.detach(), poses) on the hand-assembled inputs, visibility=None is today's call, a dict passes tol and
  radius on, and every fusion parameter gets a finite gradient."""
  import test_gpu_rig as TR
  rig = CameraRig.deep360().subset(('12', '13'))
  net, maxdepth, H, W = TR._tiny_net(rig)
  assert (H, W) == (64, 32)
  normalised = TR._host_normalised(TR._u8_frames(2, 4, H, W, 61))
  net.train()
  net.disparity.eval()
  poses = rig.panorama_poses()[[1, 3]]
  loss, depth = net.fusion_selfsup_loss(normalised, lam=0.2, visibility=True)
  loss.backward()
  assert loss.dim() == 0 and bool(torch.isfinite(loss)) and depth.shape == (2, 1, H, W) and not depth.requires_grad
  masks = HF.mv_visibility(depth.detach(), poses)
  assert masks.shape == (2, 2, H, W)
  want = HF.mv_photometric_loss(normalised[:, 0], normalised[:, [1, 3]], depth, poses, lam=0.2, masks=masks)
  assert torch.equal(loss.detach(), want)
  for k, g in _grads_of(net).items():
    if k.startswith('disparity.'):
      assert g is None, k
    else:
      assert k.startswith('fusion.') and g is not None and bool(torch.isfinite(g).all()), k
  today, depth0 = net.fusion_selfsup_loss(normalised, lam=0.2, visibility=None)
  assert torch.equal(today.detach(), HF.mv_photometric_loss(normalised[:, 0], normalised[:, [1, 3]], depth0, poses, lam=0.2))
  other, depth1 = net.fusion_selfsup_loss(normalised, lam=0.2, visibility={'tol': 0.0, 'radius': 1})
  assert torch.equal(other.detach(), HF.mv_photometric_loss(normalised[:, 0], normalised[:, [1, 3]], depth1, poses, lam=0.2,
                                                             masks=HF.mv_visibility(depth1, poses, tol=0.0, radius=1)))
