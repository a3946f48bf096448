"""CPU tier of the z-buffer visibility masks: the restatement of tests/mvvis_ref.py holds the conditions that the exact
comparisons of tests/test_gpu_mvvis.py rest on, classifies an analytic two-sphere scene, has the properties the definition implies
(identity pose, radius and tol monotone), its masked loss is tests/mvphoto_ref.py's under all-ones masks and its gradient agrees with
central differences; the fifth header parses and binds beside the other four without moving them; and the entries refuse on the host
what they cannot run."""
import ctypes

import numpy as np
import pytest
import torch

import mvphoto_ref as M
import mvvis_ref as V

import mode_hip
import models
from mode_hip import functional as HF
from utils.rig import CameraRig

IDS = ['x'.join(str(v) for v in c) for c in V.CASES]


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('case', V.CASES, ids=IDS)
def test_conditions_of_the_exact_comparisons(case):
  """Asserted on the restatement alone, with the smooth depth and Deep360's sources; nothing is excluded from any comparison on the GPU.
    1. Every valid u + 1/2 and v + 1/2 is at least 1e-9 from an integer (measured: 4.0e-5, 3.2e-5, 2.6e-4, 9.1e-7).
    2. u is at least 1e-9 from 0 and W - 1.
    3. |rho - (1 + tol) zmin| > 1e-9 rho wherever the minimum is held by another pixel, for tol in {0, 0.05} and radius in {0, 1}.
    4. Between a quarter and nine tenths of the pixels of every source are visible at radius = 0 (tol = 0.05; measured 0.63 to 0.88).
    5. Some pixels are hidden and some visible at radius = 1 (measured 0.07 to 0.26 visible).
  Every H here is even: with odd H the middle row lands on the +-pi seam of a source with A = I (include/mode_hip_mvvis.h)."""
  F, H, W, S = case
  assert H % 2 == 0
  ref, src, depth, poses = V.make_case(*case)
  assert depth.dtype == torch.float32 and float(depth.min()) >= 1.5 and float(depth.max()) <= 5.5
  c = V.exactness(depth, poses)
  print('%s: %s' % (case, c))
  assert c['land'] >= 1e-9 and c['edge'] >= 1e-9 and c['margin'] > 1e-9
  r0, r1 = V.reference_visibility(case, 0.05, 0), V.reference_visibility(case, 0.05, 1)
  for s in range(S):
    share0, share1 = float(r0['vis'][:, s].float().mean()), float(r1['vis'][:, s].float().mean())
    print('  source %d: visible %.2f at radius 0, %.2f at radius 1' % (s, share0, share1))
    assert 0.25 <= share0 <= 0.9
    assert 0 < share1 < 1


@pytest.mark.parametrize('size', [(64, 32), (128, 64)], ids=['64x32', '128x64'])
def test_the_two_sphere_scene(size):
  """The wall and its occluder, tol = 0.05, radius = 0, against the analytic visibility: among the valid pixels of each source at
  most 1 % of H W mismatch (measured: at most 7 of 2048 and 13 of 8192), and wherever a source has at least 10 analytically hidden
  valid pixels at least three quarters of them are marked hidden (measured 11 of 12, 50 of 51, 18 of 22)."""
  H, W = size
  depth, poses, seen = V.two_spheres(H, W)
  assert float(depth.min()) < 1.2 and float(depth.max()) == M.SPHERE_RADIUS
  r = V.visibility(depth, poses, 0.05, 0)
  counted = 0
  for s in range(3):
    ok = r['valid'][0, s]
    vis = r['vis'][0, s] != 0
    mismatches = int((vis != seen[0, s])[ok].sum())
    hidden = ok & ~seen[0, s]
    marked = int((~vis)[hidden].sum())
    print('%d x %d, source %d: %d mismatches among %d valid pixels; %d of %d hidden pixels marked' % (H, W, s, mismatches, int(ok.sum()), marked,
                                                                                                      int(hidden.sum())))
    assert mismatches <= 0.01 * H * W
    if int(hidden.sum()) >= 10:
      counted += 1
      assert marked >= 0.75 * int(hidden.sum())
  assert counted >= 1


def test_the_identity_pose_sees_everything():
  """[I | 0]: every pixel lands on itself, alone, so with tol = 0 everything valid is visible and zbuf == depth there.  Two things
  keep "vis = 1 everywhere for either radius" from holding word for word, and the test asserts what does hold:
    - columns 0 and W - 1 have u = 0 and u = W - 1 up to the rounding of asin(sin phi), and the validity rule 0 <= u <= W - 1 then
      falls either way (26 of 960 pixels here are invalid, all in those two columns): there vis == valid and zbuf is depth or +inf;
      columns 1 .. W - 2 are valid, visible and exact;
    - at radius 1 with tol = 0 a pixel is compared with its eight neighbours and is visible iff none of them is nearer, which a
      depth map with relief does not grant: asserted as that, and with a constant depth and tol = 1e-12 (rho = D |n| is constant to
      an ulp) everything valid is visible at radius 1 as well."""
  F, H, W = 1, 40, 24
  eye = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12)
  depth = V.smooth_depth(F, H, W)
  inner = torch.zeros(H, W, dtype=torch.bool)
  inner[:, 1:-1] = True
  for radius in V.RADII:
    r = V.visibility(depth, eye, 0.0, radius)
    valid = r['valid'][0, 0]
    assert bool(valid[inner].all()) and int((~valid).sum()) < H
    assert torch.equal(r['at'][0, 0][valid], torch.arange(H * W).view(H, W)[valid])
    assert torch.equal(r['zbuf'][0, 0][valid], depth[0][valid]) and bool(torch.isinf(r['zbuf'][0, 0][~valid]).all())
    if radius == 0:
      assert torch.equal(r['vis'] != 0, r['valid'])
    else:
      rho = torch.where(valid, r['rho'][0, 0], torch.full_like(r['rho'][0, 0], float('inf')))
      nearest = (V.neighbourhood_min(rho) == rho) & valid
      assert torch.equal(r['vis'][0, 0] != 0, nearest) and bool(nearest.any()) and not bool(nearest[inner].all())
  r = V.visibility(torch.full((F, H, W), 3.0), eye, 1e-12, 1)
  assert torch.equal(r['vis'] != 0, r['valid']) and bool(r['valid'][0, 0][inner].all())


@pytest.mark.parametrize('case', V.CASES, ids=IDS)
def test_radius_and_tol_are_monotone(case):
  """radius = 1 masks are a subset of radius = 0 masks, and a larger tol never hides more."""
  r = {(t, k): V.reference_visibility(case, t, k)['vis'] for t in V.TOLS for k in V.RADII}
  for t in V.TOLS:
    assert bool((r[(t, 1)] <= r[(t, 0)]).all()) and not torch.equal(r[(t, 1)], r[(t, 0)])
  for k in V.RADII:
    assert bool((r[(0.0, k)] <= r[(0.05, k)]).all())
  a = V.reference_visibility(case, 0.05, 0)
  assert torch.equal(a['zbuf'], V.reference_visibility(case, 0.0, 1)['zbuf'])  # z depends on neither
  assert bool(torch.isinf(a['zbuf']).any()) and bool(torch.isfinite(a['zbuf']).any())
  assert bool((a['vis'] <= a['valid'].to(torch.uint8)).all())


# ------------------------------------------------------------------------------------------------------------ the masked loss
@pytest.mark.parametrize('case', V.CASES, ids=IDS)
def test_all_ones_masks_give_the_unmasked_restatement(case):
  ref, src, depth, poses = V.make_case(*case)
  ones = torch.ones((case[0], case[3]) + case[1:3], dtype=torch.uint8)
  for dt in (torch.float64, torch.float32):
    a, ia, ga = V.evaluate(ref, src, depth, poses, ones, dt)
    b, ib, gb = M.evaluate(ref, src, depth, poses, dt)
    n, inn, gn = V.evaluate(ref, src, depth, poses, None, dt)
    assert torch.equal(a, b) and torch.equal(ia['win'], ib['win']) and ia['N'] == ib['N'] > 0 and torch.equal(ga, gb)
    assert torch.equal(ia['pe'], ib['pe']) and torch.equal(a, n) and torch.equal(ga, gn)
  # and real masks change it: fewer windows, and every winner sees its nine pixels
  l, info, g = V.reference(case, torch.float64)
  assert 0 < info['N'] < ib['N']
  _every_winner_sees_its_window(info['win'], V.reference_visibility(case)['vis'])


def _every_winner_sees_its_window(win, vis):
  F, S, H, W = vis.shape
  for s in range(S):
    all9 = torch.ones((F, H, W), dtype=torch.bool)
    for dy in (-1, 0, 1):
      for dx in (-1, 0, 1):
        shifted = torch.roll(vis[:, s] != 0, (-dy, -dx), (1, 2))
        if dx:
          shifted[..., (W - 1 if dx > 0 else 0)] = False  # columns do not wrap
        all9 &= shifted
    assert bool(all9[win == s].all()), s


@pytest.mark.parametrize('case', V.CASES, ids=IDS)
def test_conditions_of_the_masked_loss(case):
  """DESIGN 25's conditions, re-asserted for the masked cases with the seeds of mvvis_ref.SEEDS:
    1. In every window the gap between the smallest and the second-smallest pe_s exceeds 100 x the float32 restatement's largest pe
       error on the case, measured here.
    2. The float32 and float64 restatements agree on every win (and on every validity).
    3. More than half the windows are won by some source (measured 0.63 to 0.82; no single source wins half of them at S = 3)."""
  ref, src, depth, poses = V.make_case(*case)
  c = V.loss_conditions(ref, src, depth, poses, V.reference_visibility(case)['vis'])
  print('%s: %s' % (case, c))
  assert c['gap'] > 100 * c['err'], (c['gap'], c['err'])
  assert c['same']
  assert c['frac'] > 0.5


def test_conditions_of_the_pose_case():
  """The case of the gradient to the poses (generic poses): the masks' and the loss's conditions together."""
  ref, src, depth, poses = V.make_pose_case()
  e = V.exactness(depth, poses)
  c = V.loss_conditions(ref, src, depth, poses, V.reference_poses(torch.float64)[3], pose_tensor=True)
  print('%s %s' % (e, c))
  assert e['land'] >= 1e-9 and e['edge'] >= 1e-9 and e['margin'] > 1e-9
  assert c['gap'] > 100 * c['err'] and c['same'] and c['frac'] > 0.5
  _, info, g, _ = V.reference_poses(torch.float64)
  near = min(float((x - x.round()).abs()[info['valid']].min()) for x in (info['u'], info['v']))
  assert near > 1e-9  # (mvpose_ref's own condition: the gradient to the poses is the derivative, not one-sided)
  assert bool(g.any())


def test_masked_float64_restatement_against_central_differences():
  """As DESIGN 25 checks the unmasked one: 16 probes, where the gradient is largest in each sixteenth of the map; eps = 1e-6 in float64,
  the masks held constant (they are constants of the gradient).  1e-9 absolute + 1e-6 of max|g|."""
  case = V.CASES[0]
  ref, src, depth, poses = V.make_case(*case)
  masks = V.reference_visibility(case)['vis']
  loss, info, g = V.reference(case, torch.float64)
  assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
  flat = g.flatten()
  n = flat.numel()
  eps = 1e-6
  gmax = float(flat.abs().max())
  assert gmax > 0
  for k in range(16):
    i = int(flat[k * n // 16:(k + 1) * n // 16].abs().argmax()) + k * n // 16
    vals = []
    for sg in (1, -1):
      d = depth.double().clone()
      d.view(-1)[i] += sg * eps
      vals.append(float(V.mv_loss(ref, src, d, poses, masks)[0]))
    fd = (vals[0] - vals[1]) / (2 * eps)
    assert abs(fd - float(flat[i])) <= 1e-6 * gmax + 1e-9, (i, fd, float(flat[i]))


# ------------------------------------------------------------------------------------------------------------------ binding
def test_the_fifth_header_parses_and_leaves_the_others_alone():
  h = mode_hip.MVVIS
  assert sorted(h.prototypes) == ['mode_mv_visibility', 'mode_mvphoto_loss_fwd_masked', 'mode_mvvis_version', 'mode_mvvis_workspace_bytes']
  assert mode_hip.MVVIS_LAUNCHING == {'mode_mv_visibility', 'mode_mvphoto_loss_fwd_masked'}
  for name in mode_hip.MVVIS_LAUNCHING:
    assert h.prototypes[name][1][-1] == ('mode_stream_t', 'stream')
  assert h.constants == {'MODE_MVVIS_VERSION': 1} and mode_hip.MVVIS_VERSION == 1 and h.records == {}
  vis = h.prototypes['mode_mv_visibility'][1]
  assert [n for _, n in vis] == ['depth', 'poses', 'S', 'F', 'H', 'W', 'tol', 'radius', 'workspace', 'workspace_bytes', 'vis', 'zbuf', 'stream']
  assert vis[1] == ('const double*', 'poses') and vis[6] == ('double', 'tol') and vis[10] == ('unsigned char*', 'vis') and vis[11] == ('float*', 'zbuf')
  # the masked forward: the arguments of mode_mvphoto_loss_fwd plus vis
  masked = h.prototypes['mode_mvphoto_loss_fwd_masked'][1]
  plain = mode_hip.MVPHOTO.prototypes['mode_mvphoto_loss_fwd'][1]
  assert ('const unsigned char*', 'vis') in masked and [p for p in masked if p[1] != 'vis'] == plain
  assert [e[0] for e in mode_hip.EXTENSIONS] == ['SELFSUP', 'MVPHOTO', 'MVPOSE'] and [e[0] for e in mode_hip.EXTENSIONS_2] == ['MVVIS']
  # the other four headers' tables are their own
  assert len(mode_hip.SIGNATURES) == len(mode_hip.PROTOTYPES) == 173 and len(mode_hip.LAUNCHING) == 122 and len(mode_hip.CONSTANTS) == 42
  assert mode_hip.SELFSUP_LAUNCHING == {'mode_lr_consistency_fwd', 'mode_lr_consistency_bwd', 'mode_selfsup_view_loss_fwd',
                                        'mode_selfsup_view_loss_bwd'} and mode_hip.SELFSUP_VERSION == 1
  assert mode_hip.MVPHOTO_LAUNCHING == {'mode_mvphoto_loss_fwd', 'mode_mvphoto_loss_bwd'} and mode_hip.MVPHOTO_VERSION == 1
  assert sorted(mode_hip.MVPHOTO.prototypes) == ['mode_mvphoto_loss_bwd', 'mode_mvphoto_loss_fwd', 'mode_mvphoto_version',
                                                 'mode_mvphoto_workspace_bytes']
  assert mode_hip.MVPOSE_LAUNCHING == {'mode_mvpose_grad'} and mode_hip.MVPOSE_VERSION == 1
  assert sorted(mode_hip.MVPOSE.prototypes) == ['mode_mvpose_grad', 'mode_mvpose_version', 'mode_mvpose_workspace_bytes']
  others = (mode_hip.HEADER, mode_hip.SELFSUP, mode_hip.MVPHOTO, mode_hip.MVPOSE)
  assert not any(set(h.prototypes) & set(o.prototypes) for o in others)
  assert not any(k.startswith('MODE_MVVIS_') for o in others for k in o.constants)
  lib = mode_hip.lib()
  assert lib.mode_mvvis_version() == 1
  for name, (res, args) in h.signatures.items():
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args, name


def test_a_stale_library_says_rebuild(monkeypatch):
  monkeypatch.setattr(mode_hip, '_lib', None)
  monkeypatch.setattr(mode_hip, 'MVVIS_VERSION', 2)
  with pytest.raises(RuntimeError, match='mode_hip_mvvis.h.*rebuild'):
    mode_hip.lib()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _pp(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _bad_poses(good):
  """[(poses, the words of the refusal)]: every way a pose table is refused."""
  out = []
  for k in (0, 7, 35):  # an entry of A, of o, of the last pose
    for bad in (float('nan'), float('inf')):
      q = good.copy()
      q.reshape(-1)[k] = bad
      out.append((q, b'not finite'))
  q = good.copy()
  q[1, 0:3] *= 1 + 1e-8  # orthonormal to 1e-9, not to 1e-8
  out.append((q, b'orthonormal'))
  return out


def test_mv_visibility_refuses_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  good = np.ascontiguousarray(M.deep360_poses())
  n = 3 * 2 * 40 * 24
  ws = lib.mode_mvvis_workspace_bytes(3, 2, 40, 24)
  assert ws == 20 * n and lib.mode_mvvis_workspace_bytes(2, 1, 70, 37) == 2 * 41440 + 20720 and lib.mode_mvvis_workspace_bytes(1, 1, 3, 3) % 16 == 0
  assert lib.mode_mvvis_workspace_bytes(0, 2, 40, 24) == 0 and lib.mode_mvvis_workspace_bytes(9, 2, 40, 24) == 0
  assert lib.mode_mvvis_workspace_bytes(3, 2, 40, 2) == 0 and lib.mode_mvvis_workspace_bytes(3, 1 << 10, 1024, 512) == 0

  def call(depth=one, poses=None, S=3, F=2, H=40, W=24, tol=0.05, radius=0, wsp=one, wsb=ws, vis=one, zbuf=one):
    return lib.mode_mv_visibility(depth, _pp(good) if poses is None else poses, S, F, H, W, tol, radius, wsp, wsb, vis, zbuf, null)

  for name in ('depth', 'poses', 'vis'):
    assert call(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for S in (0, 9):
    assert call(S=S) == -1 and b'source views' in lib.mode_last_error()
  assert call(F=0) == -1
  assert call(W=2) == -1 and b'at least 3' in lib.mode_last_error()
  assert call(H=2) == -1 and b'at least 3' in lib.mode_last_error()
  for q, words in _bad_poses(good):
    assert call(poses=_pp(q)) == -1 and words in lib.mode_last_error(), words
  for tol in (-1e-300, -1.0, float('nan'), float('inf'), -float('inf')):
    assert call(tol=tol) == -1 and b'tol' in lib.mode_last_error(), tol
  for radius in (-1, 2, 9):
    assert call(radius=radius) == -1 and b'radius' in lib.mode_last_error(), radius
  q = np.ascontiguousarray(np.tile(good[:1], (8, 1)))
  # MODE_ERR_UNSUPPORTED: the loss's own bound 3 F S H W < 2^31 (here F S H W = 2^30), and with it every F S H W >= 2^31
  assert call(S=8, F=1 << 7, H=1024, W=1024, poses=_pp(q)) == -2 and b'2^31' in lib.mode_last_error()
  assert call(S=8, F=1 << 8, H=1024, W=1024, poses=_pp(q)) == -2 and b'2^31' in lib.mode_last_error()
  assert call(wsp=null) == -3 and call(wsb=ws - 8) == -3 and call(wsp=ctypes.c_void_p(260)) == -3  # MODE_ERR_WORKSPACE
  assert b'mode_mv_visibility' in lib.mode_last_error()


def test_the_masked_forward_refuses_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  p = ctypes.byref(mode_hip.PhotometricParams())
  good = np.ascontiguousarray(M.deep360_poses())
  ws = lib.mode_mvphoto_workspace_bytes(3, 2, 40, 24)

  def call(ref=one, src=one, depth=one, poses=None, S=3, F=2, H=40, W=24, params=p, wsp=one, wsb=ws, vis=one, win=one, stats=one, loss=one):
    return lib.mode_mvphoto_loss_fwd_masked(ref, src, depth, _pp(good) if poses is None else poses, S, F, H, W, params, wsp, wsb, vis, win, stats,
                                            loss, null)

  for name in ('ref', 'src', 'depth', 'poses', 'params', 'vis', 'win', 'stats', 'loss'):
    assert call(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for S in (0, 9):
    assert call(S=S) == -1 and b'source views' in lib.mode_last_error()
  assert call(F=0) == -1
  assert call(W=2) == -1 and b'at least 3' in lib.mode_last_error()
  assert call(H=2) == -1 and b'at least 3' in lib.mode_last_error()
  for q, words in _bad_poses(good):
    assert call(poses=_pp(q)) == -1 and words in lib.mode_last_error(), words
  q = np.ascontiguousarray(np.tile(good[:1], (8, 1)))
  assert call(S=8, F=1 << 7, H=1024, W=1024, poses=_pp(q)) == -2 and b'2^31' in lib.mode_last_error()
  assert call(wsp=null) == -3 and call(wsb=ws - 8) == -3 and call(wsp=ctypes.c_void_p(260)) == -3
  assert b'mode_mvphoto_loss_fwd_masked' in lib.mode_last_error()


def test_python_entries_refuse_what_they_cannot_run():
  depth = torch.zeros(1, 40, 24)
  poses = M.deep360_poses()
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):  # there is no CPU path
    HF.mv_visibility(depth, poses)
  net = models.ModeMultiView(maxdisp=16, height=64, width=32, rig=CameraRig.deep360().subset(('12', '13')))
  net.train()
  frames = torch.zeros(1, 4, 3, 64, 32)
  for bad in ('yes', 1, {'tolerance': 0.1}, {'tol': 0.1, 'alpha': 0.5}):
    with pytest.raises(ValueError, match='visibility is None, True or a dict with tol and / or radius'):
      net.fusion_selfsup_loss(frames, visibility=bad)
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    net.fusion_selfsup_loss(frames, visibility={'tol': 0.1})
