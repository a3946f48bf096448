"""CPU tier of the bidirectional self-supervised loss: the float64 restatement of tests/selfsup_ref.py is a well-defined
function (its gradient agrees with central differences, no pixel sits on the visibility threshold, the right view is the mirrored left
view, a two-plane scene is occluded where geometry says), the second header parses and binds beside the first without moving it, and the
C entries and the Python entries refuse on the host what they cannot run."""
import ctypes

import pytest
import torch

import selfsup_ref as S

import mode_hip
import models
from mode_hip import functional as HF

IDS = ['x'.join(str(v) for v in c) for c in S.CASES]


@pytest.mark.parametrize('case', S.CASES, ids=IDS)
def test_float64_restatement_against_central_differences(case):
  """Two probed elements per view of map 0 and of the last map, where the gradient is largest in each half.  eps = 1e-6 in float64: the
  fractions of w -/+ d keep 0.05 away from the kink of floor and |e - tau| stays above 1e-4 (tested below), so the loss is smooth over
  the step; rounding of two evaluations of a loss of order maxd is ~1e-15 x maxd / 2e-6 < 1e-8.  Hence 1e-8 absolute + 1e-6 of max|g|;
  max|g| is 1e-4 .. 1e-3."""
  _, _, dls, drs = S.make_case(*case)
  K = len(dls)
  tau, dmax = S.params(case)
  loss, stats, masks, gdl, gdr = S.lr_reference(case, torch.float64)
  assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in gdl + gdr)
  eps = 1e-6
  for k in sorted({0, K - 1}):
    for side, grads in enumerate((gdl, gdr)):
      g = grads[k].flatten()
      n = g.numel()
      for i in [int(g[q * n // 2:(q + 1) * n // 2].abs().argmax()) + q * n // 2 for q in range(2)]:
        vals = []
        for sg in (1, -1):
          maps = [[d.double().clone() for d in dls], [d.double().clone() for d in drs]]
          maps[side][k].view(-1)[i] += sg * eps
          vals.append(float(S.lr_consistency(maps[0], maps[1], S.WEIGHTS[:K], tau, dmax)[0]))
        fd = (vals[0] - vals[1]) / (2 * eps)
        assert abs(fd - float(g[i])) <= 1e-6 * float(g.abs().max()) + 1e-8, (k, side, i, fd, float(g[i]))


@pytest.mark.parametrize('case', S.CASES, ids=IDS)
def test_no_pixel_sits_on_the_visibility_threshold(case):
  """The condition of the exact mask comparison on the GPU: in float64 no valid pixel has |e - tau| < 1e-4 (an fp32 e of a few units
  errs by ~1e-6), so a mask that differs is a wrong mask; float32 and float64 agree on every mask and count; and the cases are not
  degenerate: more than half of the pixels valid, a quarter to a half visible."""
  _, _, dls, drs = S.make_case(*case)
  tau, dmax = S.params(case)
  B, H, W, K, _ = case
  closest = float('inf')
  for dl, dr in zip(dls, drs):
    pair = (dl.double(), dr.double())
    for s, own, other in S.VIEWS:
      e, valid, vis = S.lr_view(pair[own], pair[other], s, tau, dmax)
      closest = min(closest, float((e[valid] - tau).abs().min()))
  print('%s: smallest |e - tau| over valid pixels %.3e' % (case, closest))
  assert closest >= 1e-4, closest
  _, s64, m64, _, _ = S.lr_reference(case, torch.float64)
  _, s32, m32, _, _ = S.lr_reference(case, torch.float32)
  assert torch.equal(m32, m64) and torch.equal(s32[..., 0].double(), s64[..., 0]) and torch.equal(s32[..., 2].double(), s64[..., 2])
  n = B * H * W
  assert bool((s64[..., 0] > 0.5 * n).all()) and bool((s64[..., 0] < 0.8 * n).all()), s64[..., 0] / n
  assert bool((s64[..., 2] > 0.25 * n).all()) and bool((s64[..., 2] < 0.5 * n).all()), s64[..., 2] / n
  assert torch.equal(m64.sum((2, 3, 4)).double(), s64[..., 2])


def test_right_view_is_the_left_view_of_the_mirrored_pair():
  """Pins the convention: mirroring along W turns x = w + d into x' = w' - d', so the right-view loss of (own, other, d) is the
  left-view loss of the three mirrored -- to 1e-12 in float64 (sums in another order), with equal counts and mirrored gradients."""
  for case in S.CASES[:3]:
    left, right, dls, drs = S.make_case(*case)
    K = len(drs)
    mask = S.lr_reference(case, torch.float64)[2][1]
    for masks in (None, mask, S.block_mask(*case)):
      a = [d.double().requires_grad_(True) for d in drs]
      la, sa = S.view_loss(right, left, a, S.WEIGHTS[:K], 1, masks)
      b = [d.double().flip(2).requires_grad_(True) for d in drs]
      lb, sb = S.view_loss(right.flip(3), left.flip(3), b, S.WEIGHTS[:K], -1, None if masks is None else masks.flip(3))
      assert torch.equal(sa[:, 0], sb[:, 0]) and (masks is mask or float(sa[:, 0].min()) > 0.2 * case[0] * case[1] * case[2])
      assert abs(float(la.detach()) - float(lb.detach())) <= 1e-12 * abs(float(la.detach()))
      for ga, gb in zip(torch.autograd.grad(la, a), torch.autograd.grad(lb, b)):
        assert float((ga - gb.flip(2)).abs().max()) <= 1e-12 * float(ga.abs().max())
    # and the left view of this file is the loss of tests/photometric_ref.py
    import photometric_ref as R
    lc, sc = S.view_loss(left, right, [d.double() for d in dls], S.WEIGHTS[:K], -1)
    ld, sd = R.photometric_loss(left, right, [d.double() for d in dls], S.WEIGHTS[:K])
    assert torch.equal(lc, ld) and torch.equal(sc, sd)


def test_two_planes_are_occluded_where_geometry_says():
  dl, dr = S.two_planes()
  loss, stats, masks = S.lr_consistency([dl], [dr], (1.0,), 1.0, 16.0)
  for v, (s, own, other) in enumerate(S.VIEWS):
    pair = (dl, dr)
    e, valid, vis = S.lr_view(pair[own], pair[other], s, 1.0, 16.0)
    occluded = (valid & ~vis)[0]
    cols = sorted(set(occluded.nonzero()[:, 1].tolist()))
    assert cols == ([15, 16, 17, 18, 19] if v == 0 else [19, 20, 21, 22, 23]), (v, cols)
    assert bool(occluded[:, cols].all())
    assert int(stats[v, 0, 0]) == 288 and float(stats[v, 0, 1]) == 200 / 288 and int(stats[v, 0, 2]) == 288 - 40
  assert float(loss) == 2 * 200 / 288


def test_the_second_header_parses_and_leaves_the_first_alone():
  h = mode_hip.SELFSUP
  assert sorted(h.prototypes) == ['mode_lr_consistency_bwd', 'mode_lr_consistency_fwd', 'mode_lr_consistency_workspace_bytes',
                                  'mode_selfsup_version', 'mode_selfsup_view_loss_bwd', 'mode_selfsup_view_loss_fwd']
  assert mode_hip.SELFSUP_LAUNCHING == {'mode_lr_consistency_fwd', 'mode_lr_consistency_bwd', 'mode_selfsup_view_loss_fwd',
                                        'mode_selfsup_view_loss_bwd'}
  for name in mode_hip.SELFSUP_LAUNCHING:
    assert h.prototypes[name][1][-1] == ('mode_stream_t', 'stream'), name
  assert h.constants['MODE_SELFSUP_VERSION'] == mode_hip.SELFSUP_VERSION == 1 and h.constants['MODE_LR_STATS'] == mode_hip.LR_STATS == 3
  assert h.constants['MODE_LR_MAX_MAPS'] == mode_hip.PHOTOMETRIC_MAX_MAPS and h.constants['MODE_SELFSUP_VIEW_STATS'] == mode_hip.PHOTOMETRIC_STATS
  assert h.records == {'mode_lr_params': [('tau', 'float', None), ('dmax', 'float', None), ('weights', 'float', 4)]}
  P = mode_hip.LrParams
  assert ctypes.sizeof(P) == 24 and (P.tau.offset, P.dmax.offset, P.weights.offset) == (0, 4, 8)
  assert h.prototypes['mode_lr_consistency_fwd'][1][9] == ('unsigned char*', 'mask')
  assert h.signatures['mode_selfsup_view_loss_fwd'][1][3] is ctypes.c_void_p
  # the first header's tables are its own: nothing of the second is in them
  assert len(mode_hip.SIGNATURES) == len(mode_hip.PROTOTYPES) == 173 and len(mode_hip.LAUNCHING) == 122 and len(mode_hip.CONSTANTS) == 42
  assert not set(h.prototypes) & set(mode_hip.SIGNATURES) and not mode_hip.SELFSUP_LAUNCHING & mode_hip.LAUNCHING
  assert not any(k.startswith(('MODE_LR_', 'MODE_SELFSUP_')) for k in mode_hip.CONSTANTS)
  lib = mode_hip.lib()
  assert lib.mode_selfsup_version() == 1
  for name, (res, args) in h.signatures.items():
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args, name


def test_a_stale_library_says_rebuild(monkeypatch):
  monkeypatch.setattr(mode_hip, '_lib', None)
  monkeypatch.setattr(mode_hip, 'SELFSUP_VERSION', 2)
  with pytest.raises(RuntimeError, match='rebuild'):
    mode_hip.lib()


def test_lr_entries_refuse_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  prm = mode_hip.LrParams()
  prm.tau, prm.dmax = 1.0, 12.0
  ws = lib.mode_lr_consistency_workspace_bytes(3, 2, 40, 24)
  assert ws == 2 * 3 * 3 * 2 * 40 * 8 and lib.mode_lr_consistency_workspace_bytes(3, 12, 1024, 512) % 16 == 0
  assert lib.mode_lr_consistency_workspace_bytes(0, 2, 40, 24) == 0 and lib.mode_lr_consistency_workspace_bytes(3, 2, 40, 1) == 0

  def fwd(dl=one, dr=one, K=3, B=2, H=40, W=24, params=None, wsp=one, wsb=ws, mask=null, stats=one, loss=one):
    return lib.mode_lr_consistency_fwd(dl, dr, K, B, H, W, ctypes.byref(prm) if params is None else params, wsp, wsb, mask, stats, loss, null)

  def bwd(dl=one, dr=one, K=3, B=2, H=40, W=24, params=None, stats=one, gloss=one, gl=one, gr=one):
    return lib.mode_lr_consistency_bwd(dl, dr, K, B, H, W, ctypes.byref(prm) if params is None else params, stats, gloss, gl, gr, null)

  for name in ('dl', 'dr', 'params', 'stats', 'loss'):
    assert fwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for name in ('dl', 'dr', 'params', 'stats', 'gloss', 'gl', 'gr'):
    assert bwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for call in (fwd, bwd):
    for K in (0, 5):
      assert call(K=K) == -1 and b'K' in lib.mode_last_error()
    assert call(B=0) == -1
    assert call(W=1) == -1 and b'at least 2' in lib.mode_last_error()
    assert call(B=1 << 20, H=1 << 11) == -2 and b'2^31' in lib.mode_last_error()  # MODE_ERR_UNSUPPORTED: the row index
    assert call(W=mode_hip.SELFSUP.constants['MODE_LR_MAX_W'] + 1) == -2 and b'row staging' in lib.mode_last_error()
    for field in ('tau', 'dmax'):
      for bad in (0.0, -1.0, float('inf'), float('nan')):
        p = mode_hip.LrParams()
        p.tau, p.dmax = 1.0, 12.0
        setattr(p, field, bad)
        assert call(params=ctypes.byref(p)) == -1 and field.encode() in lib.mode_last_error(), (field, bad)
    p = mode_hip.LrParams()
    p.tau, p.dmax = 1.0, 24.5
    assert call(params=ctypes.byref(p)) == -2 and b'beyond W' in lib.mode_last_error()
    p.dmax = 24.0
    assert call(params=ctypes.byref(p), K=0) == -1  # (dmax == W passes that check)
  assert fwd(wsp=null) == -3 and fwd(wsb=ws - 8) == -3  # MODE_ERR_WORKSPACE


def test_view_loss_entries_refuse_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  p = ctypes.byref(mode_hip.PhotometricParams())
  ws = lib.mode_photometric_loss_workspace_bytes(3, 2, 40, 24)

  def fwd(own=one, other=one, disp=one, mask=null, view=0, K=3, B=2, H=40, W=24, params=p, wsp=one, wsb=ws, stats=one, loss=one):
    return lib.mode_selfsup_view_loss_fwd(own, other, disp, mask, view, K, B, H, W, params, wsp, wsb, stats, loss, null)

  def bwd(own=one, other=one, disp=one, mask=null, view=0, K=3, B=2, H=40, W=24, params=p, stats=one, gloss=one, gdisp=one):
    return lib.mode_selfsup_view_loss_bwd(own, other, disp, mask, view, K, B, H, W, params, stats, gloss, gdisp, null)

  for name in ('own', 'other', 'disp', 'params', 'stats', 'loss'):
    assert fwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for name in ('own', 'other', 'disp', 'params', 'stats', 'gloss', 'gdisp'):
    assert bwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for call in (fwd, bwd):
    for view in (-1, 2):
      assert call(view=view) == -1 and b'view' in lib.mode_last_error()
      assert call(view=view, mask=one) == -1
    for K in (0, 5):
      assert call(K=K) == -1 and b'K' in lib.mode_last_error()
    assert call(W=2) == -1 and b'at least 3' in lib.mode_last_error()
    assert call(H=2) == -1 and b'at least 3' in lib.mode_last_error()
    assert call(B=0) == -1
    assert call(B=1 << 20, H=1024, W=512) == -2 and b'2^31' in lib.mode_last_error()
  assert fwd(wsp=null) == -3 and fwd(wsb=ws - 8) == -3 and fwd(view=1, mask=one, wsb=ws - 8) == -3


def test_python_entries_refuse_what_they_cannot_run():
  left, right, dls, drs = S.make_case(*S.CASES[0])
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    HF.lr_consistency(dls, drs, (0.5, 0.7, 1.0), dmax=12)
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    HF.photometric_loss(right, left, drs, (0.5, 0.7, 1.0), view='right')
  with pytest.raises(ValueError, match='view'):
    HF.photometric_loss(right, left, drs, (0.5, 0.7, 1.0), view='up')
  net = models.ModeDisparity(16, 'Sphere', 64, 32, 'Cassini')
  net.eval()
  x = torch.zeros(1, 3, 64, 32)
  with pytest.raises(RuntimeError, match='training'):
    net.forward_selfsup_loss(x, x)
  erp = models.ModeDisparity(16, 'Sphere', 32, 64, 'ERP')
  erp.train()
  with pytest.raises(ValueError, match='Cassini'):
    erp.forward_selfsup_loss(torch.zeros(1, 3, 32, 64), torch.zeros(1, 3, 32, 64))
