"""CPU tier of the multi-view reprojection loss: the panorama poses of a rig; the float64 restatement of
tests/mvphoto_ref.py as a well-defined function (it reproduces DESIGN 22's left-view loss through the sine rule, a scene with a known
answer has its minimum at the true depth, its gradient agrees with central differences, its counts agree with loops over the
definition, and the conditions of the exact comparisons of tests/test_gpu_mvphoto.py hold); the third header parses and binds beside
the other two without moving them; and the C entries and the Python entries refuse on the host what they cannot run."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mvphoto_ref as M
import photometric_ref as R

import mode_hip
import models
from mode_hip import functional as HF
from utils.rig import CameraRig, PairPose

IDS = ['x'.join(str(v) for v in c) for c in M.CASES]


# ------------------------------------------------------------------------------------------------------------------ poses
def test_deep360_cameras_stand_at_four_points():
  """The twelve panoramas of Deep360 are pictures from four cameras: each camera gets one place from every pair it belongs to."""
  rig = CameraRig.deep360()
  poses = rig.panorama_poses()
  assert poses.shape == (12, 3, 4) and poses.dtype == np.float64
  for A in poses[:, :, :3]:
    assert np.abs(A @ A.T - np.eye(3)).max() <= 1e-12
  centres = -np.einsum('sji,sj->si', poses[:, :, :3], poses[:, :, 3])
  cam = {1: (0, 0, 0), 2: (-1, 0, 0), 3: (0, 0, -1), 4: (-1, 0, -1)}
  want = np.array([cam[int(c)] for name in rig.names for c in name], dtype=np.float64)  # pair 'ab': cameras a (left) and b (right)
  assert np.abs(centres - want).max() <= 1e-12, np.abs(centres - want).max()
  assert np.abs(rig.camera_centres() - want).max() <= 1e-12
  assert rig.default_sources() == (1, 3, 5) and rig.reference_panorama() == 0
  assert CameraRig.square(1.0).default_sources() == (1, 3, 5)
  sub = rig.subset(('12', '13'))
  assert sub.default_sources() == (1, 3) and sub.reference_panorama() == 0
  assert rig.subset(('34', '12')).reference_panorama() == 2


def test_pose_table():
  """Every row of the table: identity, rotate (A = R^T), view (A = R^T, o = t) and the right camera at (-b, 0, 0) of the left."""
  from utils import geometry
  Rm = np.asarray(geometry._rotation(0.3, -0.2, 0.1), dtype=np.float64)
  rig = CameraRig([PairPose('a', 0.5, 'identity'), PairPose('b', 0.25, 'rotate', (0.3, -0.2, 0.1)),
                   PairPose('c', 2.0, 'view', (0.7, -0.4, 0.9, 0.3, -0.2, 0.1))], rgb=(0,))
  P = rig.panorama_poses()
  assert np.array_equal(P[0], np.hstack([np.eye(3), np.zeros((3, 1))]))
  assert np.abs(P[2, :, :3] - Rm.T).max() <= 1e-15 and not P[2, :, 3].any()
  assert np.abs(P[4, :, :3] - Rm.T).max() <= 1e-15 and np.array_equal(P[4, :, 3], [0.9, 0.7, -0.4])  # t = (x0, y0, z0)
  for p, b in enumerate((0.5, 0.25, 2.0)):
    assert np.array_equal(P[2 * p + 1, :, :3], P[2 * p, :, :3]) and np.array_equal(P[2 * p + 1, :, 3], P[2 * p, :, 3] + [b, 0, 0])
  # 'view': X2 = R (X1 - t)  <=>  X1 = R^T X2 + t
  X2 = np.array([0.3, -1.2, 2.0])
  X1 = P[4, :, :3] @ X2 + P[4, :, 3]
  assert np.abs(Rm @ (X1 - np.array([0.9, 0.7, -0.4])) - X2).max() <= 1e-15
  # a rig without an identity pair has no image of the common view
  with pytest.raises(ValueError, match='common view has no image'):
    CameraRig([PairPose('b', 0.25, 'rotate', (0.3, -0.2, 0.1))], rgb=(0,)).reference_panorama()
  with pytest.raises(ValueError, match='common view has no image'):
    CameraRig.deep360().subset(('13', '24'), rgb=(0,)).reference_panorama()
  # a panorama at the common view's centre is never a default source
  assert CameraRig([PairPose('a', 0.5, 'identity'), PairPose('b', 0.5, 'rotate', (0.3, 0, 0))], rgb=(0,)).default_sources() == (1, 3)


# ------------------------------------------------------------------------------------- the sign check against existing code
def test_the_right_camera_of_an_identity_pair_is_design_22():
  """S = 1, source = panorama 1 and D = the unclipped sine-rule depth of a disparity map d: then u == w - d and v == h to 1e-9, and
  the warped image and the loss with lam = 0 are tests/photometric_ref.py's left-view ones to 1e-12.  d > 0 throughout (a negative
  disparity has a negative depth); some w - d fall below 0, where both are invalid."""
  B, H, W = 2, 40, 24
  left, right, _ = R.make_case(B, H, W, 1, 12)
  g = torch.Generator().manual_seed(5)
  d = 0.3 + 11.0 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
  D = M.sine_rule_depth(d, W)
  pose = CameraRig.deep360().panorama_poses()[1].reshape(12)
  u, v, valid = M.project(D, pose)
  w = torch.arange(W, dtype=torch.float64).view(1, 1, W)
  h = torch.arange(H, dtype=torch.float64).view(1, H, 1)
  pos = D > 0
  assert 0.6 < float(pos.double().mean()) < 1 and bool(torch.equal(pos, (w - d) > -0.5))
  assert float((u - (w - d))[pos].abs().max()) <= 1e-9 and float((v - h)[pos].abs().max()) <= 1e-9
  mean = torch.tensor(R.IMAGENET['mean'], dtype=torch.float64).view(1, 3, 1, 1)
  std = torch.tensor(R.IMAGENET['std'], dtype=torch.float64).view(1, 3, 1, 1)
  Rd = right.double() * std + mean
  Ih, ok, _, _ = M.warp(Rd, D, pose)
  Rh, ok22 = R.warp(Rd, d)
  assert torch.equal(ok, ok22) and 0.3 < float(ok.double().mean()) < 1
  assert float((Ih - Rh).abs().max()) <= 1e-12
  loss, info = M.mv_loss(left, right.unsqueeze(1), D, pose.reshape(1, 12), lam=0)
  loss22, stats22 = R.photometric_loss(left, right, [d], (1.0,), lam=0)
  assert info['N'] == int(stats22[0, 0]) and info['N'] > 100
  assert abs(float(loss) - float(loss22)) <= 1e-12


# ----------------------------------------------------------------------------------------------- a scene with a known answer
def test_the_true_depth_of_a_sphere_is_the_minimum():
  """The inside of a textured sphere of radius 4 around the common camera, rendered analytically into panoramas 0, 1, 3, 5 at
  64 x 32: the loss at D = 4 is below the loss at 3.6 and at 4.4, and at 3.6 the gradient asks for more depth."""
  ref, src, poses = M.sphere_scene(64, 32)
  out = {}
  for D in (3.6, 4.0, 4.4):
    depth = torch.full((1, 64, 32), D, dtype=torch.float64)
    out[D] = M.evaluate(ref, src, depth, poses, torch.float64)
    print('D = %.1f: loss %.6e, N = %d' % (D, float(out[D][0]), out[D][1]['N']))
  assert float(out[4.0][0]) < float(out[3.6][0]) and float(out[4.0][0]) < float(out[4.4][0])
  assert out[4.0][1]['N'] > 0.9 * 64 * 30
  loss, info, g = out[3.6]
  valid = info['valid'].any(0)
  assert float(g[valid].mean()) < 0
  assert float(out[4.4][2][out[4.4][1]['valid'].any(0)].mean()) > 0  # (and at 4.4 for less)


# -------------------------------------------------------------------------------------------------------------- the gradient
def test_closed_form_slopes_are_autograd():
  ref, src, depth, poses = M.make_case(*M.CASES[0])
  for s in range(3):
    d = depth.double().requires_grad_(True)
    u, v, valid = M.project(d, poses[s])
    du = torch.autograd.grad(u.sum(), d, retain_graph=True)[0]
    dv = torch.autograd.grad(v.sum(), d)[0]
    cu, cv = M.slopes(depth, poses[s])
    assert bool(valid.any())
    assert float((du - cu)[valid].abs().max()) <= 1e-12 * float(cu[valid].abs().max())
    assert float((dv - cv)[valid].abs().max()) <= 1e-12 * max(float(cv[valid].abs().max()), 1.0)


def test_float64_restatement_against_central_differences():
  """16 probes, where the gradient is largest in each sixteenth of the map; eps = 1e-6 in float64.  The loss is smooth over the step:
  u and v keep 2e-5 away from the kinks of floor and the runner-up of every window is 2e-5 behind (tested below; a step of 1e-6 in D
  moves u by ~1e-6 and pe by less).  Rounding of two evaluations of a loss of order 0.5 is ~1e-16 x 0.5 / 2e-6 < 1e-10; the
  truncation is eps^2 f''' / 6.  Hence 1e-9 absolute + 1e-6 of max|g|; max|g| is ~1e-3."""
  case = M.CASES[0]
  ref, src, depth, poses = M.make_case(*case)
  loss, info, g = M.reference(case, torch.float64)
  assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
  flat = g.flatten()
  n = flat.numel()
  eps = 1e-6
  gmax = float(flat.abs().max())
  for k in range(16):
    i = int(flat[k * n // 16:(k + 1) * n // 16].abs().argmax()) + k * n // 16
    vals = []
    for sg in (1, -1):
      d = depth.double().clone()
      d.view(-1)[i] += sg * eps
      vals.append(float(M.mv_loss(ref, src, d, poses)[0]))
    fd = (vals[0] - vals[1]) / (2 * eps)
    assert abs(fd - float(flat[i])) <= 1e-6 * gmax + 1e-9, (i, fd, float(flat[i]))


# --------------------------------------------------------------------------------------------------------------- brute force
def _brute_valid(depth, pose, H, W):
  """valid, floor(u), floor(v) of one frame by loops over the definition with the math module."""
  A = [pose[0:3], pose[4:7], pose[8:11]]
  o = [pose[3], pose[7], pose[11]]
  ok = [[False] * W for _ in range(H)]
  for h in range(H):
    theta = math.pi - (h + 0.5) * 2 * math.pi / H
    for w in range(W):
      phi = math.pi / 2 - (w + 0.5) * math.pi / W
      n = (math.sin(phi), math.cos(phi) * math.sin(theta), math.cos(phi) * math.cos(theta))
      D = float(depth[h, w])
      if not (math.isfinite(D) and D > 0):
        continue
      Y = [D * sum(A[r][c] * n[c] for c in range(3)) + o[r] for r in range(3)]
      rho = math.sqrt(sum(y * y for y in Y))
      if not rho > 0:
        continue
      u = (math.pi / 2 - math.asin(max(-1.0, min(1.0, Y[0] / rho)))) * W / math.pi - 0.5
      ok[h][w] = 0 <= u <= W - 1
  return ok


def test_counts_and_winners_against_loops():
  """N and win of the first case (with a few depths spoilt) by loops: validity per pixel and source from the definition with the math
  module, a window valid iff its nine pixels are, the winner the first source with the smallest pe among the valid ones."""
  case = M.CASES[0]
  ref, src, depth, poses = M.make_case(*case)
  depth = depth.clone()
  depth[0, 3, 5], depth[0, 20, 10], depth[1, 7, 7], depth[1, 30, 20] = float('nan'), 0.0, -2.0, float('inf')
  far = poses.copy()
  far[2, 3] += 7.0  # the third source from far away: much of it leaves the pole-to-pole range
  loss, info = M.mv_loss(ref, src, depth.double(), far)
  F, H, W, S = case
  n = 0
  for f in range(F):
    ok = [_brute_valid(depth[f].double(), far[s], H, W) for s in range(S)]
    for h in range(H):
      for w in range(W):
        best, arg = None, M.NO_WINNER
        if 1 <= w <= W - 2:
          for s in range(S):
            if all(ok[s][(h + dy) % H][w + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
              pe = float(info['pe'][s, f, h, w - 1])
              assert math.isfinite(pe)
              if best is None or pe < best:
                best, arg = pe, s
            else:
              assert float(info['pe'][s, f, h, w - 1]) == float('inf')
        n += arg != M.NO_WINNER
        assert int(info['win'][f, h, w]) == arg, (f, h, w)
  assert n == info['N'] and 0.5 * F * H * (W - 2) < n < F * H * (W - 2)
  assert not bool(info['valid'][:, 0, 3, 5].any()) and not bool(info['valid'][:, 1, 30, 20].any())
  assert len(set(info['win'].flatten().tolist())) == S + 1


# ------------------------------------------------------------------------- the conditions of the exact comparisons on the GPU
@pytest.mark.parametrize('case', M.CASES, ids=IDS)
def test_conditions_of_the_exact_comparisons(case):
  """Asserted on the restatement alone, for the seeds of mvphoto_ref.SEEDS; nothing is excluded from any comparison on the GPU.
    1. No pixel has u within 1e-9 of an integer or of 0 / W - 1.  No pixel has v within 1e-9 of an integer -- EXCEPT where the point
       moves along the source's rows only, |dv/dD| <= 1e-9: the right camera of the reference's own pair has v == h identically (the
       sign check above asserts it), and for odd W the centre column lies in the epipolar plane of source 3 and lands on v = H/4 - 1/2
       exactly.  There floor's choice between the row pairs (y0, q ~ 1) and (y0 + 1, q ~ 0) changes neither Ih (the bilinear is
       continuous) nor its slope in D, which that choice enters through dv/dD alone.  The test asserts that this is the only way
       in which v comes near an integer.
    2. In every window the gap between the smallest and the second-smallest pe_s exceeds 100 x the float32 restatement's largest pe
       error on the case, measured here.
    3. The float32 and float64 restatements agree on every win (and on every validity).
    4. At least 25 % of the windows have a winner."""
  F, H, W, S = case
  ref, src, depth, poses = M.make_case(*case)
  l64, i64, g64 = M.reference(case, torch.float64)
  l32, i32, g32 = M.reference(case, torch.float32)
  u, v = i64['u'], i64['v']
  du = torch.minimum((u - u.round()).abs(), torch.minimum(u.abs(), (u - (W - 1)).abs()))
  assert float(du.min()) > 1e-9, float(du.min())
  near = (v - v.round()).abs() <= 1e-9
  dvdD = torch.stack([M.slopes(depth, poses[s])[1] for s in range(S)])
  assert not bool(near.any()) or float(dvdD[near].abs().max()) <= 1e-9
  assert not bool(near[1:].any()) or W % 2 == 1  # (only the reference's own pair, and the centre column of an odd width)
  fin = torch.isfinite(i64['pe'])
  assert torch.equal(fin, torch.isfinite(i32['pe'])) and torch.equal(i32['valid'], i64['valid'])
  err = float((i32['pe'].double() - i64['pe'])[fin].abs().max())
  if S > 1:
    srt = torch.sort(i64['pe'], 0).values
    both = torch.isfinite(srt[1])
    gap = float((srt[1] - srt[0])[both].min()) if bool(both.any()) else float('inf')
  else:
    gap = float('inf')
  frac = i64['N'] / float(F * H * (W - 2))
  print('%s: min distance of u from an integer %.2e, largest float32 pe error %.2e, smallest gap %.2e, windows with a winner %.1f %%' % (
      case, float(du.min()), err, gap, 100 * frac))
  assert gap > 100 * err, (gap, err)
  assert torch.equal(i32['win'], i64['win']) and i32['N'] == i64['N']
  assert frac >= 0.25


# ------------------------------------------------------------------------------------------------------------------ binding
def test_the_third_header_parses_and_leaves_the_others_alone():
  h = mode_hip.MVPHOTO
  assert sorted(h.prototypes) == ['mode_mvphoto_loss_bwd', 'mode_mvphoto_loss_fwd', 'mode_mvphoto_version', 'mode_mvphoto_workspace_bytes']
  assert mode_hip.MVPHOTO_LAUNCHING == {'mode_mvphoto_loss_fwd', 'mode_mvphoto_loss_bwd'}
  for name in mode_hip.MVPHOTO_LAUNCHING:
    assert h.prototypes[name][1][-1] == ('mode_stream_t', 'stream'), name
  assert h.constants['MODE_MVPHOTO_VERSION'] == mode_hip.MVPHOTO_VERSION == 1
  assert h.constants['MODE_MVP_MAX_SOURCES'] == mode_hip.MVP_MAX_SOURCES == 8 and h.constants['MODE_MVP_STATS'] == mode_hip.MVP_STATS == 12
  assert h.constants['MODE_MVP_NO_WINNER'] == M.NO_WINNER == 255 and h.records == {}
  assert h.prototypes['mode_mvphoto_loss_fwd'][1][3] == ('const double*', 'poses')
  assert h.prototypes['mode_mvphoto_loss_fwd'][1][11] == ('unsigned char*', 'win')
  assert h.prototypes['mode_mvphoto_loss_bwd'][1][9] == ('const unsigned char*', 'win')
  # the other two headers' tables are their own
  assert len(mode_hip.SIGNATURES) == len(mode_hip.PROTOTYPES) == 173 and len(mode_hip.LAUNCHING) == 122 and len(mode_hip.CONSTANTS) == 42
  assert mode_hip.SELFSUP_LAUNCHING == {'mode_lr_consistency_fwd', 'mode_lr_consistency_bwd', 'mode_selfsup_view_loss_fwd',
                                        'mode_selfsup_view_loss_bwd'} and mode_hip.SELFSUP_VERSION == 1
  assert not set(h.prototypes) & (set(mode_hip.SIGNATURES) | set(mode_hip.SELFSUP.prototypes))
  assert not any(k.startswith(('MODE_MVP_', 'MODE_MVPHOTO_')) for k in list(mode_hip.CONSTANTS) + list(mode_hip.SELFSUP.constants))
  lib = mode_hip.lib()
  assert lib.mode_mvphoto_version() == 1
  for name, (res, args) in h.signatures.items():
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args, name


def test_a_stale_library_says_rebuild(monkeypatch):
  monkeypatch.setattr(mode_hip, '_lib', None)
  monkeypatch.setattr(mode_hip, 'MVPHOTO_VERSION', 2)
  with pytest.raises(RuntimeError, match='mode_hip_mvphoto.h.*rebuild'):
    mode_hip.lib()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_entries_refuse_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  p = ctypes.byref(mode_hip.PhotometricParams())
  good = np.ascontiguousarray(M.deep360_poses())
  ws = lib.mode_mvphoto_workspace_bytes(3, 2, 40, 24)
  assert ws == 12 * 2 * 3 * 1 * 8 and lib.mode_mvphoto_workspace_bytes(3, 2, 1024, 512) % 16 == 0
  assert lib.mode_mvphoto_workspace_bytes(0, 2, 40, 24) == 0 and lib.mode_mvphoto_workspace_bytes(9, 2, 40, 24) == 0
  assert lib.mode_mvphoto_workspace_bytes(3, 2, 40, 2) == 0 and lib.mode_mvphoto_workspace_bytes(3, 1 << 10, 1024, 512) == 0

  def pp(a):
    return a.ctypes.data_as(ctypes.c_void_p)

  def fwd(ref=one, src=one, depth=one, poses=None, S=3, F=2, H=40, W=24, params=p, wsp=one, wsb=ws, win=one, stats=one, loss=one):
    return lib.mode_mvphoto_loss_fwd(ref, src, depth, pp(good) if poses is None else poses, S, F, H, W, params, wsp, wsb, win, stats, loss, null)

  def bwd(ref=one, src=one, depth=one, poses=None, S=3, F=2, H=40, W=24, params=p, win=one, stats=one, gloss=one, gdepth=one):
    return lib.mode_mvphoto_loss_bwd(ref, src, depth, pp(good) if poses is None else poses, S, F, H, W, params, win, stats, gloss, gdepth, null)

  for name in ('ref', 'src', 'depth', 'poses', 'params', 'win', 'stats', 'loss'):
    assert fwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for name in ('ref', 'src', 'depth', 'poses', 'params', 'win', 'stats', 'gloss', 'gdepth'):
    assert bwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for call in (fwd, bwd):
    for S in (0, 9):
      assert call(S=S) == -1 and b'source views' in lib.mode_last_error()
    assert call(F=0) == -1
    assert call(W=2) == -1 and b'at least 3' in lib.mode_last_error()
    assert call(H=2) == -1 and b'at least 3' in lib.mode_last_error()
    for k in (0, 7, 35):  # an entry of A, of o, of the last pose
      for bad in (float('nan'), float('inf')):
        q = good.copy()
        q.reshape(-1)[k] = bad
        assert call(poses=pp(q)) == -1 and b'not finite' in lib.mode_last_error(), (k, bad)
    q = good.copy()
    q[1, 0] += 1e-8  # orthonormal to 1e-9, not to 1e-8
    assert call(poses=pp(q)) == -1 and b'orthonormal' in lib.mode_last_error()
    q = good.copy()
    q[2, 0:3] *= 2.0
    assert call(poses=pp(q)) == -1 and b'orthonormal' in lib.mode_last_error()
    q = np.ascontiguousarray(np.tile(good[:1], (8, 1)))
    q[:, 0] += 1e-11  # within the bound: these poses pass, and the size is refused after them
    assert call(S=8, F=1 << 7, H=1024, W=1024, poses=pp(q)) == -2 and b'2^31' in lib.mode_last_error()  # MODE_ERR_UNSUPPORTED
  assert fwd(wsp=null) == -3 and fwd(wsb=ws - 8) == -3 and fwd(wsp=ctypes.c_void_p(260)) == -3  # MODE_ERR_WORKSPACE


def test_python_entries_refuse_what_they_cannot_run():
  ref, src, depth, poses = M.make_case(*M.CASES[0])
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    HF.mv_photometric_loss(ref, src, depth, poses)
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, dbname='other')
  net.train()
  with pytest.raises(ValueError, match=r'CameraRig\.square\(0\.6 \* sqrt\(2\)\)'):
    net.fusion_selfsup_loss(torch.zeros(1, 12, 3, 64, 32))
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, resize=True)
  net.train()
  with pytest.raises(ValueError, match='resize'):
    net.fusion_selfsup_loss(torch.zeros(1, 12, 64, 32, 3, dtype=torch.uint8))
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, rig=CameraRig.deep360().subset(('13', '24'), rgb=(0,)))
  net.train()
  with pytest.raises(ValueError, match='common view has no image'):
    net.fusion_selfsup_loss(torch.zeros(1, 4, 3, 64, 32))
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, rig=CameraRig.deep360().subset(('12', '13')))
  net.eval()
  with pytest.raises(RuntimeError, match='training step of the fusion network'):
    net.fusion_selfsup_loss(torch.zeros(1, 4, 3, 64, 32))
  net.train()
  with pytest.raises(ValueError, match='sources'):
    net.fusion_selfsup_loss(torch.zeros(1, 4, 3, 64, 32), sources=(4,))
  with pytest.raises(ValueError, match='return_stats'):
    net.fusion_selfsup_loss(torch.zeros(1, 4, 3, 64, 32), return_stats=True)
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    net.fusion_selfsup_loss(torch.zeros(1, 4, 3, 64, 32))
