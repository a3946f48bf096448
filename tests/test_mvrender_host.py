"""CPU tier of the novel-view rendering: the restatement of tests/mvrender_ref.py holds the conditions that the exact
comparisons of tests/test_gpu_mvrender.py rest on, classifies the two-sphere scene, renders the analytic sphere towards its known
answer, and has the properties the definition implies (identity pose, fill and tol monotone); the sixth header parses and binds
beside the other five without moving them; the entries refuse on the host what they cannot run; utils.rig.view_pose inverts
camera_centres."""
import ctypes

import numpy as np
import pytest
import torch

import mvphoto_ref as M
import mvrender_ref as R
import mvvis_ref as V

import mode_hip
import models
from mode_hip import functional as HF
from utils.rig import CameraRig, view_pose

ALL = R.CASES + (R.SPHERES,)
IDS = ['x'.join(str(v) for v in c) for c in ALL]


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_conditions_of_the_exact_comparisons(case):
  """Asserted on the float64 restatement alone, at 1e-9 each; nothing is excluded from any comparison on the GPU.  Measured (smooth-depth
  cases / two spheres): u + 1/2, v + 1/2 from an integer >= 1.8e-6 / 3.8e-5; u from the edges >= 2.0e-4 / 3.6e-3; the two smallest rho
  of a target pixel apart by >= 7.9e-6 / 1.8e-7 (relative); the two smallest keys of a neighbourhood by >= 1.5e-6 / 1.8e-7;
  |z - 1.05 zn| / z >= 5.1e-6 / 3.3e-4; a resampling u_r from 0 and W - 1 >= 1.9e-4; u_r, v_r from an integer >= 4.6e-7.
  Both colour branches occur in every view: 6 to 72 pixels fall back to the splat's value, 96 to 99.3 % are resampled (fill = 1)."""
  c = R.exactness(case)
  print('%s: %s' % (case, c))
  for k in ('land', 'edge', 'pixel', 'near', 'margin', 'redge', 'rint'):
    assert c[k] >= 1e-9, (k, c[k])
  image, depth, poses = R.make_case(case)
  assert depth.dtype == torch.float32 and image.dtype == torch.float32 and depth.shape[-2] % 2 == 0
  for fill in R.FILLS:
    hit = R.reference(case, 0.05, fill)['hit']
    for t in range(hit.shape[1]):
      seen, resampled = hit[:, t] != R.NONE, hit[:, t] & R.RESAMPLED != 0
      assert bool((resampled <= seen).all())
      assert int(resampled.sum()) >= 1 and int((seen & ~resampled).sum()) >= 1, (fill, t)


def test_classes_of_the_two_sphere_scene():
  """fill = 1, tol = 0.05.  Measured per view: NONE on at most 0.64 % of the pixels, FILLED over a finite z (a far surface seen through
  the cracks of the magnified near one) on 1.4 to 1.8 %, holes before filling on 5 to 19 %."""
  r = R.reference(R.SPHERES, 0.05, 1)
  for t in range(3):
    hit, z = r['hit'][:, t], r['z'][:, t]
    n = float(hit.numel())
    none, through, holes = int((hit == R.NONE).sum()) / n, int(((hit & R.FILLED != 0) & torch.isfinite(z)).sum()) / n, int(torch.isinf(z).sum()) / n
    print('view %d: NONE %.4f, see-through %.4f, holes before filling %.4f' % (t, none, through, holes))
    assert none <= 0.01 and through <= 0.03 and 0 < holes


def _sphere_errors(H, W):
  """Per pose the mean absolute error of the render of the analytic sphere (depth 4) against render_sphere(pose), over the pixels that
  show something (the images are normalised, so the 0 of a NONE pixel is no colour of the scene; at most 1.2 % are NONE here):
  (resample, splat)."""
  image = M.sphere_scene(H, W)[0]
  depth = torch.full((1, H, W), M.SPHERE_RADIUS, dtype=torch.float32)
  poses = R.poses_of(3)
  want = torch.stack([M.render_sphere(p, H, W) for p in poses])
  out = []
  for t in range(3):
    errs = []
    for mode in (R.RESAMPLE, R.SPLAT):
      r = R.render(image, depth, poses, 0.05, 1, mode)
      seen = (r['hit'][0, t] != R.NONE).unsqueeze(0).expand(3, H, W)
      assert float(seen.double().mean()) >= 0.98
      errs.append(float((r['out'][0, t] - want[t]).abs()[seen].mean()))
    out.append(tuple(errs))
  return out


def test_the_known_answer():
  """The inside of the textured sphere, rendered to the three poses.  Measured mean absolute errors: at 64 x 32 resample 0.0081 to
  0.0103 and splat 0.060 to 0.099; at 136 x 72 resample 0.0020 to 0.0021 and splat 0.034 to 0.047."""
  small, large = _sphere_errors(64, 32), _sphere_errors(136, 72)
  for t in range(3):
    print('pose %d: 64 x 32 resample %.4f splat %.4f; 136 x 72 resample %.4f splat %.4f' % ((t,) + small[t] + large[t]))
    for resample, splat in (small[t], large[t]):
      assert resample <= splat / 4
    assert large[t][0] <= small[t][0] / 3


def test_the_identity_pose_shows_the_image():
  """[I | 0]: every pixel lands on itself, so index is the pixel's own and the splat is the image on columns 1 .. W - 2; the pole columns
  0 and W - 1 have u = 0 and W - 1 up to the rounding of asin(sin phi) and fall either way."""
  F, H, W = 1, 40, 24
  eye = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12)
  image, depth = V.make_case(2, 40, 24, 3)[0][:1], V.smooth_depth(F, H, W)
  r = R.render(image, depth, eye, 0.0, 0, R.SPLAT, torch.float32)
  own = torch.arange(H * W, dtype=torch.int32).view(1, 1, H, W)
  assert torch.equal(r['index'][..., 1:-1], own[..., 1:-1]) and bool((r['hit'][..., 1:-1] == R.DIRECT).all())
  assert torch.equal(r['out'][:, 0, :, :, 1:-1], image[..., 1:-1]) and torch.equal(r['range'][:, 0, :, 1:-1], depth[..., 1:-1])
  edge = r['index'][..., [0, W - 1]]
  assert bool(((edge == own[..., [0, W - 1]]) | (edge == -1)).all())


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_fill_and_tol_are_monotone(case):
  """fill = 1 never shows fewer pixels than fill = 0 (and what fill = 0 shows, fill = 1 shows too); a larger tol never has fewer DIRECT
  pixels; index names a valid pixel exactly where something is seen, and range is finite exactly there."""
  r = {(t, f): R.reference(case, t, f) for t in R.TOLS for f in R.FILLS}
  for t in R.TOLS:
    seen0, seen1 = r[(t, 0)]['hit'] != R.NONE, r[(t, 1)]['hit'] != R.NONE
    assert bool((seen0 <= seen1).all()) and int(seen1.sum()) > int(seen0.sum())
  direct = {t: r[(t, 1)]['hit'] & R.DIRECT != 0 for t in R.TOLS}
  assert bool((direct[0.0] <= direct[0.05]).all()) and int(direct[0.05].sum()) > int(direct[0.0].sum())
  HW = r[(0.05, 1)]['hit'].shape[-1] * r[(0.05, 1)]['hit'].shape[-2]
  for res in r.values():
    seen = res['hit'] != R.NONE
    assert torch.equal(res['index'] >= 0, seen) and bool((res['index'] < HW).all()) and torch.equal(torch.isfinite(res['range']), seen)
    assert bool((res['hit'] & R.DIRECT != 0).logical_and(res['hit'] & R.FILLED != 0).logical_not().all())


# ------------------------------------------------------------------------------------------------------------------ binding
def test_the_sixth_header_parses_and_leaves_the_others_alone():
  h = mode_hip.MVRENDER
  assert sorted(h.prototypes) == ['mode_mv_render', 'mode_mvrender_version', 'mode_mvrender_workspace_bytes']
  assert mode_hip.MVRENDER_LAUNCHING == {'mode_mv_render'}
  render = h.prototypes['mode_mv_render'][1]
  assert render[-1] == ('mode_stream_t', 'stream')
  assert [n for _, n in render] == ['image', 'depth', 'poses', 'T', 'F', 'C', 'H', 'W', 'tol', 'fill', 'mode', 'workspace', 'workspace_bytes', 'out',
                                    'hit', 'range', 'index', 'stream']
  assert render[2] == ('const double*', 'poses') and render[8] == ('double', 'tol') and render[14] == ('unsigned char*', 'hit')
  assert render[15] == ('float*', 'range') and render[16] == ('int*', 'index')
  assert h.constants == {'MODE_MVRENDER_VERSION': 1, 'MODE_MVR_SPLAT': 0, 'MODE_MVR_RESAMPLE': 1, 'MODE_MVR_MAX_CHANNELS': 4, 'MODE_MVR_HIT_NONE': 0,
                         'MODE_MVR_HIT_DIRECT': 1, 'MODE_MVR_HIT_FILLED': 2, 'MODE_MVR_HIT_RESAMPLED': 4}
  assert mode_hip.MVRENDER_VERSION == 1 and h.records == {}
  assert (R.SPLAT, R.RESAMPLE) == (mode_hip.MVR_SPLAT, mode_hip.MVR_RESAMPLE)
  assert (R.NONE, R.DIRECT, R.FILLED, R.RESAMPLED) == (mode_hip.MVR_HIT_NONE, mode_hip.MVR_HIT_DIRECT, mode_hip.MVR_HIT_FILLED, mode_hip.MVR_HIT_RESAMPLED)
  assert [e[0] for e in mode_hip.EXTENSIONS] == ['SELFSUP', 'MVPHOTO', 'MVPOSE'] and [e[0] for e in mode_hip.EXTENSIONS_2] == ['MVVIS']
  assert mode_hip.EXTENSIONS_3 == (('MVRENDER', 'mode_hip_mvrender.h', 'MODE_MVRENDER_VERSION', 'mode_mvrender_version'),)
  # the five older headers' tables are their own
  assert len(mode_hip.SIGNATURES) == len(mode_hip.PROTOTYPES) == 173 and len(mode_hip.LAUNCHING) == 122 and len(mode_hip.CONSTANTS) == 42
  assert mode_hip.SELFSUP_LAUNCHING == {'mode_lr_consistency_fwd', 'mode_lr_consistency_bwd', 'mode_selfsup_view_loss_fwd',
                                        'mode_selfsup_view_loss_bwd'} and mode_hip.SELFSUP_VERSION == 1
  assert mode_hip.MVPHOTO_LAUNCHING == {'mode_mvphoto_loss_fwd', 'mode_mvphoto_loss_bwd'} and mode_hip.MVPHOTO_VERSION == 1
  assert mode_hip.MVPOSE_LAUNCHING == {'mode_mvpose_grad'} and mode_hip.MVPOSE_VERSION == 1
  assert mode_hip.MVVIS_LAUNCHING == {'mode_mv_visibility', 'mode_mvphoto_loss_fwd_masked'} and mode_hip.MVVIS_VERSION == 1
  assert sorted(mode_hip.MVVIS.prototypes) == ['mode_mv_visibility', 'mode_mvphoto_loss_fwd_masked', 'mode_mvvis_version', 'mode_mvvis_workspace_bytes']
  assert mode_hip.MVVIS.constants == {'MODE_MVVIS_VERSION': 1}
  others = (mode_hip.HEADER, mode_hip.SELFSUP, mode_hip.MVPHOTO, mode_hip.MVPOSE, mode_hip.MVVIS)
  assert not any(set(h.prototypes) & set(o.prototypes) for o in others)
  assert not any(k.startswith(('MODE_MVRENDER_', 'MODE_MVR_')) for o in others for k in o.constants)
  lib = mode_hip.lib()
  assert lib.mode_mvrender_version() == 1
  for name, (res, args) in h.signatures.items():
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args, name


def test_a_stale_library_says_rebuild(monkeypatch):
  monkeypatch.setattr(mode_hip, '_lib', None)
  monkeypatch.setattr(mode_hip, 'MVRENDER_VERSION', 2)
  with pytest.raises(RuntimeError, match='mode_hip_mvrender.h.*rebuild'):
    mode_hip.lib()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _pp(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def test_workspace_sizes():
  """With n = F T H W: the keys (8 n), rho (8 n), the landing indices (4 n) and the owners (4 n), each part rounded up to 16 bytes."""
  ws = mode_hip.lib().mode_mvrender_workspace_bytes
  assert ws(3, 2, 40, 24) == 24 * 3 * 2 * 40 * 24
  assert ws(2, 1, 70, 37) == 2 * 41440 + 2 * 20720  # n = 5180: 8 n = 41440 and 4 n = 20720 are multiples of 16
  assert ws(1, 1, 3, 3) == 2 * 80 + 2 * 48  # n = 9: 72 -> 80 and 36 -> 48
  assert ws(1, 1, 3, 3) % 16 == 0 and ws(8, 1, 5, 7) % 16 == 0
  for T, F, H, W in ((0, 2, 40, 24), (9, 2, 40, 24), (3, 0, 40, 24), (3, 2, 2, 24), (3, 2, 40, 2), (3, 1 << 10, 1024, 512), (8, 1 << 7, 1024, 1024)):
    assert ws(T, F, H, W) == 0, (T, F, H, W)


def test_mv_render_refuses_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  good = R.poses_of(3)
  ws = lib.mode_mvrender_workspace_bytes(3, 2, 40, 24)

  def call(image=one, depth=one, poses=None, T=3, F=2, C=3, H=40, W=24, tol=0.05, fill=1, mode=1, wsp=one, wsb=ws, out=one, hit=one, rng=one,
           index=one):
    return lib.mode_mv_render(image, depth, _pp(good) if poses is None else poses, T, F, C, H, W, tol, fill, mode, wsp, wsb, out, hit, rng, index, null)

  for name in ('image', 'depth', 'poses', 'out', 'hit'):
    assert call(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for C in (0, 5, -1):
    assert call(C=C) == -1 and b'channels' in lib.mode_last_error(), C
  for T in (0, 9):
    assert call(T=T) == -1 and b'source views' in lib.mode_last_error()
  assert call(F=0) == -1
  assert call(W=2) == -1 and b'at least 3' in lib.mode_last_error()
  assert call(H=2) == -1 and b'at least 3' in lib.mode_last_error()
  for k in (0, 7, 35):  # an entry of A, of o, of the last pose
    for bad in (float('nan'), float('inf')):
      q = good.copy()
      q.reshape(-1)[k] = bad
      assert call(poses=_pp(q)) == -1 and b'not finite' in lib.mode_last_error(), (k, bad)
  q = good.copy()
  q[1, 0:3] *= 1 + 1e-8  # orthonormal to 1e-9, not to 1e-8
  assert call(poses=_pp(q)) == -1 and b'orthonormal' in lib.mode_last_error()
  for tol in (-1e-300, -1.0, float('nan'), float('inf'), -float('inf')):
    assert call(tol=tol) == -1 and b'tol' in lib.mode_last_error(), tol
  for fill in (-1, 2, 9):
    assert call(fill=fill) == -1 and b'fill' in lib.mode_last_error(), fill
  for mode in (-1, 2, 9):
    assert call(mode=mode) == -1 and b'mode = ' in lib.mode_last_error(), mode
  q = np.ascontiguousarray(np.tile(good[:1], (8, 1)))
  # MODE_ERR_UNSUPPORTED: the family's bound 3 F T H W < 2^31, and this entry's own C F T H W < 2^31 (here F T H W = 2^29, C = 4)
  assert call(T=8, F=1 << 7, H=1024, W=1024, poses=_pp(q)) == -2 and b'2^31' in lib.mode_last_error()
  assert call(T=8, F=1 << 6, C=4, H=1024, W=1024, poses=_pp(q)) == -2 and b'C F T H W' in lib.mode_last_error()
  assert call(T=8, F=1 << 6, C=3, H=1024, W=1024, poses=_pp(q), wsb=0) == -3  # (3 x 2^29 passes both bounds; then the workspace is short)
  assert call(wsp=null) == -3 and call(wsb=ws - 8) == -3 and call(wsp=ctypes.c_void_p(260)) == -3  # MODE_ERR_WORKSPACE
  assert b'mode_mv_render' in lib.mode_last_error()
  # range and index may be NULL: with everything else in order the call gets as far as the workspace check
  assert call(rng=null, index=null, wsb=ws - 8) == -3


def test_python_entries_refuse_what_they_cannot_run():
  image, depth, poses = torch.zeros(1, 3, 40, 24), torch.zeros(1, 40, 24), R.poses_of(2)
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):  # there is no CPU path
    HF.mv_render(image, depth, poses)
  rig = CameraRig.deep360().subset(('12', '13'))
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, rig=rig)
  frames = torch.zeros(1, 4, 3, 64, 32)
  with pytest.raises(ValueError, match='not a parameter of the render'):
    net.render_views(frames, poses, return_index=True)
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    net.train()
    net.render_views(frames, poses)
  assert net.training and net.fusion.training  # the modes are left as they were
  with pytest.raises(ValueError, match='resize=True'):
    models.ModeMultiView(maxdisp=16, height=64, width=32, resize=True).render_views(frames, poses)


# ---------------------------------------------------------------------------------------------------------------- view_pose
def test_view_pose_inverts_camera_centres():
  rig = CameraRig.deep360()
  poses, centres = rig.panorama_poses(), rig.camera_centres()
  for P, c in zip(poses, centres):
    got = view_pose(c, P[:, :3].T)
    assert got.shape == (3, 4) and got.dtype == np.float64 and np.abs(got - P).max() <= 1e-15
    assert np.abs(-got[:, :3].T @ got[:, 3] - c).max() <= 1e-15
  assert np.array_equal(view_pose((0.1, -0.2, 0.3)), np.array([[1, 0, 0, -0.1], [0, 1, 0, 0.2], [0, 0, 1, -0.3]]))
  for bad in ((0, 0), (0, 0, float('nan'))):
    with pytest.raises(ValueError, match='centre'):
      view_pose(bad)
  for bad in (np.eye(4), 2 * np.eye(3), np.ones((3, 3))):
    with pytest.raises(ValueError, match='rotation'):
      view_pose((0, 0, 0), bad)
