"""GPU (-m gpu): the multi-view reprojection loss of DESIGN 25 -- HF.mv_photometric_loss (csrc/mv_photometric.hip) and
ModeMultiView.fusion_selfsup_loss -- against the float64 restatement of tests/mvphoto_ref.py.

win and N are exact: the kernel computes u, v in fp64 as the restatement does, and tests/test_mvphoto_host.py asserts on the
restatement that no pixel of the four cases sits on a kink of floor or of validity and that no window's runner-up is close.  Loss and
gdepth follow DESIGN 24's bound: the yardstick of a quantity is the float32 restatement's own error against float64 (geometry in
float64 in both, as in the kernel; max over ALL elements, relative to max|g64|), never below one fp32 ulp, 2^-23 max|g64|; the kernel
may take 4 times the yardstick.  Nothing is excluded.

Measured ratios on an MI355X: see DESIGN 25."""
import numpy as np
import pytest
import torch

import mvphoto_ref as M

from mode_hip import functional as HF
from utils.rig import CameraRig

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['x'.join(str(v) for v in c) for c in M.CASES]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _run(ref, src, depth, poses, **kw):
  """-> (loss, stats (3 + S,), win (F, H, W), gdepth) on the CPU through the public entry."""
  d = depth.detach().to(DEV).requires_grad_(True)
  loss, stats, win = HF.mv_photometric_loss(ref.to(DEV), src.to(DEV), d, poses, return_stats=True, return_win=True, **kw)
  assert win.dtype == torch.uint8 and win.is_cuda and not win.requires_grad and stats.dtype == torch.float64 and loss.dim() == 0
  loss.backward()
  assert d.grad.shape == d.shape
  return loss.detach().cpu(), stats.cpu(), win.cpu(), d.grad.cpu()


def _within(tag, got, a32, b64):
  """got within 4 x the yardstick of b64; prints the ratio."""
  yard, scale = M.yardstick(a32, b64)
  if scale == 0:
    assert not bool(torch.as_tensor(got).any()), tag
    return 0.0
  err = M.error(got, b64, scale)
  print('  %s: max|ref64| %.3e, error %.3e, yardstick %.3e of it, ratio %.2f' % (tag, scale, err, yard, err / yard))
  assert err <= 4 * yard, (tag, err, yard)
  return err / yard


def _check(tag, got, r32, r64):
  loss, stats, win, g = got
  l32, i32, g32 = r32
  l64, i64, g64 = r64
  S = stats.numel() - 3
  assert torch.equal(i32['win'], i64['win']), 'the case sits on a kink: float32 and float64 disagree on a winner'
  assert torch.equal(win, i64['win']), (tag, int((win != i64['win']).sum()))
  assert float(stats[0]) == i64['N']
  for s in range(S):
    assert float(stats[3 + s]) == int((i64['win'] == s).sum()), s
  print('%s: loss %.9g, N %d, wins %s' % (tag, float(loss), i64['N'], stats[3:].tolist()))
  assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
  ratios = [_within('loss', loss, l32, l64), _within('gdepth', g.reshape(g64.shape), g32, g64)]
  assert abs(float(stats[1]) - float(i64['photo'])) <= 1e-5 * abs(float(i64['photo'])) + 1e-300
  assert abs(float(stats[2]) - float(i64['smooth'])) <= 1e-5 * abs(float(i64['smooth'])) + 1e-300
  return ratios


def _refs(ref, src, depth, poses, **kw):
  return M.evaluate(ref, src, depth, poses, torch.float32, **kw), M.evaluate(ref, src, depth, poses, torch.float64, **kw)


@pytest.mark.parametrize('case', M.CASES, ids=IDS)
def test_parity_with_the_float64_restatement(case):
  ref, src, depth, poses = M.make_case(*case)
  got = _run(ref, src, depth, poses)
  _check('mv %s' % (case,), got, M.reference(case, torch.float32), M.reference(case, torch.float64))
  assert float(got[1][0]) >= 0.25 * case[0] * case[1] * (case[2] - 2)


@pytest.mark.parametrize('alpha', [0.0, 1.0], ids=['l1', 'ssim'])
@pytest.mark.parametrize('case', [M.CASES[0], M.CASES[2]], ids=[IDS[0], IDS[2]])
def test_one_photometric_term_alone(case, alpha):
  ref, src, depth, poses = M.make_case(*case)
  got = _run(ref, src, depth, poses, alpha=alpha, lam=0.0)
  _check('alpha = %g, lam = 0' % alpha, got, M.reference(case, torch.float32, alpha=alpha, lam=0.0),
         M.reference(case, torch.float64, alpha=alpha, lam=0.0))


def test_smoothness_alone():
  """Every source translated so far along its own x axis that every point lands beside its pole: nothing is valid, N = 0, photo = 0,
  the loss is lam x the smoothness term; with lam = 0 the loss is 0 and gdepth is exact zeros."""
  case = M.CASES[2]
  ref, src, depth, poses = M.make_case(*case)
  far = poses.copy()
  far[:, 3] += 1e6
  got = _run(ref, src, depth, far)
  r32, r64 = _refs(ref, src, depth, far)
  assert r64[1]['N'] == 0 and float(r64[0]) > 0
  _check('smoothness alone', got, r32, r64)
  loss, stats, win, g = got
  assert float(stats[0]) == 0 and float(stats[1]) == 0 and bool((win == 255).all()) and bool(torch.isfinite(loss)) and bool(g.any())
  loss, stats, win, g = _run(ref, src, depth, far, lam=0.0)
  assert float(loss) == 0 and not bool(g.any()) and not bool(stats[:2].any()) and not bool(stats[3:].any()) and bool((win == 255).all())


def test_spoilt_depths_cost_their_pixels_only():
  """NaN, +Inf, 0 and a negative depth at single pixels: invalid for every source (no window that contains them has a winner), in no
  smoothness pair, a gradient of exactly 0, and the loss stays finite -- with the smoothness term and without."""
  case = M.CASES[0]
  ref, src, depth, poses = M.make_case(*case)
  depth = depth.clone()
  spots = ((0, 3, 5, float('nan')), (0, 20, 10, 0.0), (1, 7, 7, -2.0), (1, 30, 20, float('inf')), (1, 0, 0, float('nan')), (0, 39, 23, 0.0))
  for f, h, w, bad in spots:
    depth[f, h, w] = bad
  for kw in ({}, {'lam': 0.0}):
    got = _run(ref, src, depth, poses, **kw)
    r32, r64 = _refs(ref, src, depth, poses, **kw)
    _check('spoilt depths %s' % (kw,), got, r32, r64)
    loss, stats, win, g = got
    H, W = case[1], case[2]
    for f, h, w, _ in spots:
      assert float(g[f, h, w]) == 0
      for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
          if 0 <= w + dx < W:
            assert int(win[f, (h + dy) % H, w + dx]) == 255
    assert float(stats[0]) < case[0] * H * (W - 2)


def test_eight_sources():
  case = (1, 40, 24, 8)
  ref, src, depth, _ = M.make_case(*case[:3], 3)
  g = torch.Generator().manual_seed(88)
  src = torch.cat([src, torch.randn(1, 5, 3, 40, 24, generator=g) * 0.5 + src[:, :1]], 1)
  poses = M.deep360_poses((1, 3, 5, 7, 9, 11, 6, 8))
  got = _run(ref, src, depth, poses)
  r32, r64 = _refs(ref, src, depth, poses)
  _check('S = 8', got, r32, r64)
  assert bool((got[1][3:] > 0).all())  # every source wins somewhere
  with pytest.raises(ValueError, match='source views'):
    HF.mv_photometric_loss(ref.to(DEV), torch.cat([src, src[:, :1]], 1).to(DEV), depth.to(DEV), np.concatenate([poses, poses[:1]]))


def test_the_four_dimensional_layout_and_the_pose_forms():
  case = M.CASES[1]
  ref, src, depth, poses = M.make_case(*case)
  a = _run(ref, src, depth, poses)
  b = _run(ref, src, depth.unsqueeze(1), torch.from_numpy(poses).reshape(-1, 3, 4))
  assert b[3].shape == (case[0], 1, case[1], case[2])
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3].squeeze(1))
  c = HF.mv_photometric_loss(ref.to(DEV), src.to(DEV), depth.to(DEV), poses.tolist())
  assert torch.equal(c.cpu(), a[0]) and not c.requires_grad


def test_two_calls_and_a_side_stream_are_bit_equal():
  case = M.CASES[3]
  ref, src, depth, poses = M.make_case(*case)
  a = _run(ref, src, depth, poses)
  b = _run(ref, src, depth, poses)
  side = torch.cuda.Stream(device=DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    c = _run(ref, src, depth, poses)
  side.synchronize()
  for x, y, z in zip(a, b, c):
    assert torch.equal(x, y) and torch.equal(x, z)


# ------------------------------------------------------------------------------------------------------------------ the model
def _grads_of(module):
  return {k: (None if p.grad is None else p.grad.clone()) for k, p in module.named_parameters()}


def _rig():
  return CameraRig.deep360().subset(('12', '13'))


@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
def test_fusion_selfsup_loss_is_the_loss_on_the_frames_own_panoramas(u8):
  """ModeMultiView(rig = pairs 12, 13) at 64 x 32 with disparity.eval(): the loss is HF.mv_photometric_loss on the hand-assembled
  inputs (reference = panorama 0, sources = panoramas 1 and 3 with their poses), every fusion parameter gets a finite gradient and no
  disparity parameter gets one."""
  import test_gpu_rig as TR
  rig = _rig()
  assert rig.reference_panorama() == 0 and rig.default_sources() == (1, 3)
  net, maxdepth, H, W = TR._tiny_net(rig)
  assert (H, W) == (64, 32)
  frames_u8 = TR._u8_frames(2, 4, H, W, 61)
  normalised = TR._host_normalised(frames_u8)
  frames = frames_u8 if u8 else normalised
  with pytest.raises(RuntimeError, match='training step of the fusion network'):
    net.fusion_selfsup_loss(frames)
  net.train()
  net.disparity.eval()
  loss, depth = net.fusion_selfsup_loss(frames, lam=0.2)
  loss.backward()
  assert loss.dim() == 0 and bool(torch.isfinite(loss)) and depth.shape == (2, 1, H, W) and not depth.requires_grad
  want = HF.mv_photometric_loss(normalised[:, 0], normalised[:, [1, 3]], depth, rig.panorama_poses()[[1, 3]], lam=0.2)
  assert torch.equal(loss.detach(), want)
  for k, g in _grads_of(net).items():
    if k.startswith('disparity.'):
      assert g is None, k
    else:
      assert k.startswith('fusion.') and g is not None and bool(torch.isfinite(g).all()), k
  assert any(bool(g.abs().max() > 0) for k, g in _grads_of(net.fusion).items())
  # chosen sources
  one, _ = net.fusion_selfsup_loss(frames, sources=(3,), lam=0.2)
  assert torch.equal(one.detach(), HF.mv_photometric_loss(normalised[:, 0], normalised[:, [3]], depth, rig.panorama_poses()[[3]], lam=0.2))


@pytest.mark.parametrize('handoff_grad', ['depth', 'full'])
def test_fusion_selfsup_loss_fine_tunes_stage_one(handoff_grad):
  import test_gpu_rig as TR
  kw = {'handoff_grad': 'full', 'conf_png': False} if handoff_grad == 'full' else {}
  net, maxdepth, H, W = TR._tiny_net(_rig(), **kw)
  frames = TR._host_normalised(TR._u8_frames(2, 4, H, W, 62))
  net.train()
  loss, depth = net.fusion_selfsup_loss(frames)
  loss.backward()
  assert bool(torch.isfinite(loss))
  got = _grads_of(net)
  for k, g in got.items():
    assert g is not None and bool(torch.isfinite(g).all()), k
  assert any(bool(g.abs().max() > 0) for k, g in got.items() if k.startswith('disparity.'))


def test_fusion_selfsup_loss_refuses_what_it_cannot_run():
  import models
  import test_gpu_rig as TR
  net = models.ModeMultiView(16, 1000., 64, 32, channels=(8, 16, 32, 64), resize=True).to(DEV).train()
  with pytest.raises(ValueError, match='resize'):
    net.fusion_selfsup_loss(TR._u8_frames(1, 12, 64, 32, 7))
  net = models.ModeMultiView(16, 1000., 64, 32, channels=(8, 16, 32, 64), dbname='other').to(DEV).train()
  with pytest.raises(ValueError, match=r'CameraRig\.square\(0\.6 \* sqrt\(2\)\)'):
    net.fusion_selfsup_loss(TR._host_normalised(TR._u8_frames(1, 12, 64, 32, 7)))
