"""CPU tier of the rig self-calibration: the restatement of tests/mvpose_ref.py (the loss with the poses as a tensor) is
tests/mvphoto_ref.py's loss, its autograd is the closed form of include/mode_hip_mvpose.h and agrees with central differences along
twist directions, the conditions of the exact comparisons of tests/test_gpu_mvpose.py hold, the documented kink at exactly rectified
poses is there, utils.rig_refine.RigRefinement parameterises a rig and writes it back, a run with a known answer converges; the
fourth header parses and binds beside the other three without moving them; and the entries refuse on the host what they cannot run."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mvphoto_ref as M
import mvpose_ref as P

import mode_hip
import models
from utils import rig as rig_module
from utils.rig import CameraRig, PairPose
from utils.rig_refine import RigRefinement

IDS = ['x'.join(str(v) for v in c) for c in P.CASES]


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('case', P.CASES, ids=IDS)
def test_detached_poses_give_the_loss_of_mvphoto_ref(case):
  ref, src, depth, poses = P.make_case(*case)
  for dt in (torch.float64, torch.float32):
    a, ia = P.mv_loss(ref, src, depth.to(dt), torch.from_numpy(poses))
    b, ib = M.mv_loss(ref, src, depth.to(dt), poses)
    assert torch.equal(a, b) and torch.equal(ia['win'], ib['win']) and ia['N'] == ib['N'] and ia['N'] > 0
    assert torch.equal(ia['pe'], ib['pe']) and torch.equal(ia['u'], ib['u']) and torch.equal(ia['v'], ib['v'])


@pytest.mark.parametrize('case', P.CASES, ids=IDS)
def test_closed_form_is_autograd(case):
  """The definition of include/mode_hip_mvpose.h against autograd through the float64 restatement, to 1e-12 of max|g|."""
  ref, src, depth, poses = P.make_case(*case)
  _, _, g = P.reference(case, torch.float64)
  c = P.closed_form(ref, src, depth, poses)
  gmax = float(g.abs().max())
  print('%s: max|g| %.3e, closed form - autograd %.2e of it' % (case, gmax, float((c - g).abs().max()) / gmax))
  assert gmax > 0 and float((c - g).abs().max()) <= 1e-12 * gmax
  # and with the smoothness term switched off the gradient is the same: the term does not depend on the poses
  assert torch.equal(P.reference(case, torch.float64, lam=0.0)[2], g)


@pytest.mark.parametrize('case', P.CASES, ids=IDS)
def test_conditions_of_the_exact_comparisons(case):
  """Asserted on the restatement alone, for the seeds of mvpose_ref.SEEDS; nothing is excluded from any comparison on the GPU.
    1. No valid pixel has u or v within 1e-9 of an integer.
    2. In every window the gap between the smallest and the second-smallest pe_s exceeds 100 x the float32 restatement's largest pe
       error on the case, measured here.
    3. The float32 and float64 restatements agree on every win (and on every validity).
    4. At least 95 % of the windows have a winner."""
  c = P.conditions(case)
  print('%s: %s' % (case, c))
  assert c['near'] > 1e-9
  assert c['gap'] > 100 * c['err'], (c['gap'], c['err'])
  assert c['same']
  assert c['frac'] >= 0.95


def _floors(info):
  ok = info['valid']
  return ok, info['u'].floor()[ok], info['v'].floor()[ok], info['win']


@pytest.mark.parametrize('case', P.CASES, ids=IDS)
def test_float64_restatement_against_central_differences(case):
  """Twelve probes along twist directions (A' = Exp(t omega) A, o' = Exp(t omega) o + t tau): six single axes, on the sources in
  turn, and six seeded directions over all sources; eps = 1e-7.  The loss is smooth over the step -- asserted: no valid pixel's
  floor(u) or floor(v), no validity and no winner differs between the two evaluations (u, v keep >= 2e-5 from an integer and a twist
  of 1e-7 moves them by ~1e-6 at most).  Rounding of two evaluations of a loss of order 0.5 is ~1e-16 x 0.5 / 2e-7 < 1e-9 and the
  truncation eps^2 f''' / 6 is far below; hence 1e-6 of max|g|, max|g| ~ 0.1."""
  F, H, W, S = case
  ref, src, depth, poses = P.make_case(*case)
  P0 = torch.from_numpy(poses)
  d64 = depth.double()
  _, _, g = P.reference(case, torch.float64)
  gmax = float(g.abs().max())
  gen = torch.Generator().manual_seed(99)
  eps = 1e-7
  worst = 0.0
  for k in range(12):
    if k < 6:
      d = torch.zeros(S, 6, dtype=torch.float64)
      d[k % S, k] = 1.0
    else:
      d = torch.randn(S, 6, generator=gen, dtype=torch.float64)
      d /= d.norm()
    t = torch.zeros((), dtype=torch.float64, requires_grad=True)
    loss, _ = P.mv_loss(ref, src, d64, P.twisted(P0, t * d))
    want = float(torch.autograd.grad(loss, t)[0])
    vals, infos = [], []
    for sg in (1, -1):
      l, info = P.mv_loss(ref, src, d64, P.twisted(P0, sg * eps * d))
      vals.append(float(l))
      infos.append(_floors(info))
    for x, y in zip(*infos):
      assert torch.equal(x, y), 'a pixel crossed a kink within the step'
    fd = (vals[0] - vals[1]) / (2 * eps)
    worst = max(worst, abs(fd - want) / gmax)
    assert abs(fd - want) <= 1e-6 * gmax, (k, fd, want, gmax)
  print('%s: max|g| %.3e, worst probe %.2e of it' % (case, gmax, worst))


def test_the_gradient_is_one_sided_at_exactly_rectified_poses():
  """The documented kink, pinned: at Deep360's exact poses panorama 1 has v == h at every pixel, floor chooses a side, and source 1's
  d loss / d o_y differs from the central difference by more than 1 % of max|g|.  (With generic poses it agrees to 1e-6: above.)"""
  case = P.CASES[0]
  ref, src, depth, poses = M.make_case(*case)
  assert np.array_equal(poses[0].reshape(3, 4), np.hstack([np.eye(3), [[1.0], [0.0], [0.0]]]))  # the right camera of pair 12
  _, info, g = P.evaluate(ref, src, depth, poses, torch.float64)
  v = info['v'][0][info['valid'][0]]
  assert float((v - v.round()).abs().max()) <= 1e-9
  gmax = float(g.abs().max())
  eps = 1e-6
  vals = []
  for sg in (1, -1):
    q = poses.copy()
    q[0, 7] += sg * eps
    vals.append(float(P.mv_loss(ref, src, depth.double(), torch.from_numpy(q))[0]))
  fd = (vals[0] - vals[1]) / (2 * eps)
  print('d loss / d o_y of source 1: autograd %.6e, central difference %.6e, max|g| %.3e' % (float(g[0, 7]), fd, gmax))
  assert abs(fd - float(g[0, 7])) > 0.01 * gmax


# ------------------------------------------------------------------------------------------------------------- RigRefinement
def _random_twist(refine, seed, scale=0.3):
  g = torch.Generator().manual_seed(seed)
  with torch.no_grad():
    refine.twist.copy_((torch.rand(refine.twist.shape, generator=g, dtype=torch.float64) * 2 - 1) * scale)
  return refine


@pytest.mark.parametrize('rig', [CameraRig.deep360(), CameraRig.square(0.7)], ids=['deep360', 'square0.7'])
def test_rig_refinement(rig):
  refine = RigRefinement(rig)
  assert [k for k, _ in refine.named_parameters()] == ['twist'] and refine.twist.shape == (6, 6) and refine.twist.dtype == torch.float64
  base = rig.panorama_poses()
  assert float((refine().detach() - torch.from_numpy(base)).abs().max()) <= 1e-15
  assert refine.refined_rig() == rig
  kinds = [p.kind for p in rig.pairs]
  want = torch.tensor([[0.0] * 6 if k == 'identity' else [1.0] * 3 + [0.0] * 3 if k == 'rotate' else [1.0] * 6 for k in kinds], dtype=torch.float64)
  assert torch.equal(refine.mask, want) and 'identity' in kinds and 'rotate' in kinds and 'view' in kinds
  _random_twist(refine, 3)
  poses = refine()
  assert poses.shape == (12, 3, 4) and poses.requires_grad
  A = poses[:, :, :3].detach()
  assert float((A @ A.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12
  for k, p in enumerate(rig.pairs):
    assert torch.equal(poses[2 * k + 1, :, :3], poses[2 * k, :, :3])
    assert torch.equal(poses[2 * k + 1, :, 3], poses[2 * k, :, 3] + torch.tensor([p.exact, 0.0, 0.0], dtype=torch.float64))
    if p.kind == 'identity':
      assert torch.equal(poses[2 * k].detach(), torch.from_numpy(base[2 * k]))
    elif p.kind == 'rotate':
      assert not bool(poses[2 * k, :, 3].any())
    else:
      assert float((poses[2 * k].detach() - torch.from_numpy(base[2 * k])).abs().max()) > 0.01
  # masked entries: an exactly zero gradient, the others a gradient
  w = torch.randn(12, 3, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
  (poses * w).sum().backward()
  assert not bool(refine.twist.grad[refine.mask == 0].any()) and bool((refine.twist.grad[refine.mask == 1] != 0).all())
  # the way back
  back = refine.refined_rig()
  assert back.names == rig.names and back.rgb == rig.rgb and [p.kind for p in back.pairs] == kinds
  assert [p.baseline for p in back.pairs] == [p.baseline for p in rig.pairs] and [p.exact for p in back.pairs] == [p.exact for p in rig.pairs]
  assert float(np.abs(back.panorama_poses() - poses.detach().numpy()).max()) <= 1e-12
  assert back != rig and back.pairs[0] == rig.pairs[0]


def test_rig_refinement_switches():
  rig = CameraRig.deep360()
  assert not bool(RigRefinement(rig, rotation=False).mask[:, :3].any()) and bool(RigRefinement(rig, rotation=False).mask[:, 3:].any())
  assert not bool(RigRefinement(rig, translation=False).mask[:, 3:].any()) and bool(RigRefinement(rig, translation=False).mask[:, :3].any())
  frozen = _random_twist(RigRefinement(rig, rotation=False, translation=False), 4)
  assert float((frozen().detach() - torch.from_numpy(rig.panorama_poses())).abs().max()) == 0 and frozen.refined_rig() == rig
  with pytest.raises(ValueError, match='must be a CameraRig'):
    RigRefinement('deep360')


def test_euler_round_trip_and_the_gimbal():
  g = torch.Generator().manual_seed(8)
  for _ in range(50):
    pitch, roll = ((torch.rand(2, generator=g, dtype=torch.float64) * 2 - 1) * math.pi).tolist()
    yaw = float((torch.rand((), generator=g, dtype=torch.float64) * 2 - 1) * 1.5)
    got = rig_module._euler(rig_module._rotation(pitch, yaw, roll))
    assert max(abs(a - b) for a, b in zip(got, (pitch, yaw, roll))) <= 1e-12, (got, pitch, yaw, roll)
  assert rig_module._euler(np.eye(3)) == (0.0, 0.0, 0.0)
  for yaw in (math.pi / 2, -math.pi / 2, math.pi / 2 - 5e-7):
    with pytest.raises(ValueError, match='pi/2'):
      rig_module._euler(rig_module._rotation(0.3, yaw, -0.2))
  rig_module._euler(rig_module._rotation(0.3, math.pi / 2 - 2e-6, -0.2))
  with pytest.raises(ValueError, match='3 x 3'):
    rig_module._euler(np.eye(4))
  # a refinement that turns a pair into the gimbal refuses to be written back
  refine = RigRefinement(CameraRig([PairPose('a', 1.0, 'identity'), PairPose('b', 1.0, 'rotate', (0.0, math.pi / 2 - 0.1, 0.0))], rgb=(0,)))
  with torch.no_grad():
    refine.twist[1, 2] = -0.1  # R' = R Exp(-omega): about z, towards yaw = pi/2
  with pytest.raises(ValueError, match='pi/2'):
    refine.refined_rig()


# ----------------------------------------------------------------------------------------------- a run with a known answer
@pytest.mark.parametrize('source', [3, 7])
def test_calibration_finds_the_true_pose_of_a_sphere(source):
  """mvpose_ref.known_answer on the float64 restatement: source 3 (pair 13, 'rotate') brings its rotation error below one fifth of
  its start, source 7 (pair 23, 'view') its rotation and its translation error."""
  def loss_of(ref, src, depth, poses):
    return P.mv_loss(ref, src, depth, poses, lam=0.0)[0]

  (r0, t0), (r1, t1) = P.known_answer(source, loss_of)
  print('source %d: rotation error %.4f -> %.4f, translation error %.4f -> %.4f' % (source, r0, r1, t0, t1))
  assert r0 > 0.005 and r1 < r0 / 5  # (the start is off by a quarter of a degree or more)
  if source == 7:
    assert t0 > 0.02 and t1 < t0 / 5
  else:
    assert t0 == 0 and t1 == 0


# ------------------------------------------------------------------------------------------------------------------ binding
def test_the_fourth_header_parses_and_leaves_the_others_alone():
  h = mode_hip.MVPOSE
  assert sorted(h.prototypes) == ['mode_mvpose_grad', 'mode_mvpose_version', 'mode_mvpose_workspace_bytes']
  assert mode_hip.MVPOSE_LAUNCHING == {'mode_mvpose_grad'}
  assert h.prototypes['mode_mvpose_grad'][1][-1] == ('mode_stream_t', 'stream')
  assert h.constants == {'MODE_MVPOSE_VERSION': 1} and mode_hip.MVPOSE_VERSION == 1 and h.records == {}
  assert h.prototypes['mode_mvpose_grad'][1][3] == ('const double*', 'poses')
  assert h.prototypes['mode_mvpose_grad'][1][9] == ('const unsigned char*', 'win')
  assert h.prototypes['mode_mvpose_grad'][1][14] == ('double*', 'gposes')
  assert [e[0] for e in mode_hip.EXTENSIONS] == ['SELFSUP', 'MVPHOTO', 'MVPOSE']
  # the other three headers' tables are their own
  assert len(mode_hip.SIGNATURES) == len(mode_hip.PROTOTYPES) == 173 and len(mode_hip.LAUNCHING) == 122 and len(mode_hip.CONSTANTS) == 42
  assert mode_hip.SELFSUP_LAUNCHING == {'mode_lr_consistency_fwd', 'mode_lr_consistency_bwd', 'mode_selfsup_view_loss_fwd',
                                        'mode_selfsup_view_loss_bwd'} and mode_hip.SELFSUP_VERSION == 1
  assert mode_hip.MVPHOTO_LAUNCHING == {'mode_mvphoto_loss_fwd', 'mode_mvphoto_loss_bwd'} and mode_hip.MVPHOTO_VERSION == 1
  assert sorted(mode_hip.MVPHOTO.prototypes) == ['mode_mvphoto_loss_bwd', 'mode_mvphoto_loss_fwd', 'mode_mvphoto_version',
                                                 'mode_mvphoto_workspace_bytes']
  assert not set(h.prototypes) & (set(mode_hip.SIGNATURES) | set(mode_hip.SELFSUP.prototypes) | set(mode_hip.MVPHOTO.prototypes))
  assert not any(k.startswith('MODE_MVPOSE_') for k in list(mode_hip.CONSTANTS) + list(mode_hip.SELFSUP.constants) + list(mode_hip.MVPHOTO.constants))
  lib = mode_hip.lib()
  assert lib.mode_mvpose_version() == 1
  for name, (res, args) in h.signatures.items():
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args, name


def test_a_stale_library_says_rebuild(monkeypatch):
  monkeypatch.setattr(mode_hip, '_lib', None)
  monkeypatch.setattr(mode_hip, 'MVPOSE_VERSION', 2)
  with pytest.raises(RuntimeError, match='mode_hip_mvpose.h.*rebuild'):
    mode_hip.lib()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_the_entry_refuses_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  p = ctypes.byref(mode_hip.PhotometricParams())
  good = np.ascontiguousarray(P.perturbed_poses(3, 0))
  ws = lib.mode_mvpose_workspace_bytes(3, 2, 40, 24)
  assert ws == 12 * 3 * 2 * 3 * 1 * 8 and lib.mode_mvpose_workspace_bytes(3, 2, 1024, 512) % 16 == 0
  assert lib.mode_mvpose_workspace_bytes(0, 2, 40, 24) == 0 and lib.mode_mvpose_workspace_bytes(9, 2, 40, 24) == 0
  assert lib.mode_mvpose_workspace_bytes(3, 2, 40, 2) == 0 and lib.mode_mvpose_workspace_bytes(3, 1 << 10, 1024, 512) == 0

  def pp(a):
    return a.ctypes.data_as(ctypes.c_void_p)

  def call(ref=one, src=one, depth=one, poses=None, S=3, F=2, H=40, W=24, params=p, win=one, stats=one, gloss=one, wsp=one, wsb=ws, gposes=one):
    return lib.mode_mvpose_grad(ref, src, depth, pp(good) if poses is None else poses, S, F, H, W, params, win, stats, gloss, wsp, wsb, gposes, null)

  for name in ('ref', 'src', 'depth', 'poses', 'params', 'win', 'stats', 'gloss', 'gposes'):
    assert call(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
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
  q[1, 0:3] *= 1 + 1e-8  # orthonormal to 1e-9, not to 1e-8
  assert call(poses=pp(q)) == -1 and b'orthonormal' in lib.mode_last_error()
  q = np.ascontiguousarray(np.tile(good[:1], (8, 1)))
  assert call(S=8, F=1 << 7, H=1024, W=1024, poses=pp(q)) == -2 and b'2^31' in lib.mode_last_error()  # MODE_ERR_UNSUPPORTED
  assert call(wsp=null) == -3 and call(wsb=ws - 8) == -3 and call(wsp=ctypes.c_void_p(260)) == -3  # MODE_ERR_WORKSPACE
  assert b'mode_mvpose_grad' in lib.mode_last_error()


def test_python_entries_refuse_what_they_cannot_run():
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, rig=CameraRig.deep360().subset(('12', '13')))
  net.train()
  frames = torch.zeros(1, 4, 3, 64, 32)
  for bad in (torch.zeros(3, 3, 4, dtype=torch.float64), torch.zeros(4, 3, 3, dtype=torch.float64), np.zeros((4, 13))):
    with pytest.raises(ValueError, match=r'poses must be \(2P, 3, 4\) or \(2P, 12\)'):
      net.fusion_selfsup_loss(frames, poses=bad)
  refine = RigRefinement(CameraRig.deep360().subset(('12', '13')))
  with pytest.raises(ValueError, match='sources'):
    net.fusion_selfsup_loss(frames, sources=(4,), poses=refine())
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):  # as without poses: there is no CPU path
    net.fusion_selfsup_loss(frames, poses=refine())
