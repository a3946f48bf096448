"""GPU (-m gpu): the bidirectional self-supervised loss of DESIGN 24 -- HF.lr_consistency (csrc/lr_consistency.hip), the view loss from
either camera with a mask (HF.photometric_loss(view=, masks=); csrc/photometric.hip) and their entries on ModeDisparity and
ModeMultiView -- against the float64 restatement of tests/selfsup_ref.py.

The bound is DESIGN 22's with a floor.  The yardstick of a quantity is the float32 restatement's own error against float64 (max over
elements, relative to max|g64|), never taken below one fp32 ulp of the quantity, 2^-23 max|g64|: a correctly rounded fp32 result
already errs by half an ulp, so a smaller yardstick is luck.  The kernel may take 4 times the yardstick.  Masks and counts are exact
(tests/test_selfsup_host.py asserts that no pixel of these cases sits within 1e-4 of the threshold).  Nothing is excluded.

Measured ratios on an MI355X: see DESIGN 24."""
import pytest
import torch

import selfsup_ref as S

from mode_hip import functional as HF
from utils.rig import CameraRig

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['x'.join(str(v) for v in c) for c in S.CASES]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _within(tag, got, a32, b64):
  """got within 4 x the yardstick of b64; prints the ratio."""
  yard, scale = S.yardstick(a32, b64)
  if scale == 0:
    assert not bool(torch.as_tensor(got).any()), tag
    return 0.0
  err = S.error(got, b64, scale)
  print('  %s: max|ref64| %.3e, error %.3e, yardstick %.3e of it, ratio %.2f' % (tag, scale, err, yard, err / yard))
  assert err <= 4 * yard, (tag, err, yard)
  return err / yard


def _lr(dls, drs, weights, tau, dmax):
  """-> (loss, masks (2, K, B, H, W) uint8, stats (2, K, 3), [gdl_k], [gdr_k]) on the CPU."""
  ls = [d.detach().to(DEV).requires_grad_(True) for d in dls]
  rs = [d.detach().to(DEV).requires_grad_(True) for d in drs]
  loss, masks, stats = HF.lr_consistency(ls, rs, weights, tau=tau, dmax=dmax, return_masks=True, return_stats=True)
  assert masks.dtype == torch.uint8 and masks.is_cuda and stats.shape == (2, len(ls), 3) and not masks.requires_grad
  loss.backward()
  return loss.detach().cpu(), masks.cpu(), stats.cpu(), [d.grad.cpu() for d in ls], [d.grad.cpu() for d in rs]


def _lr_refs(dls, drs, weights, tau, dmax):
  out = []
  for dt in (torch.float32, torch.float64):
    xs = [d.detach().clone().to(dt).requires_grad_(True) for d in list(dls) + list(drs)]  # (a clone: .to() of the same dtype is d itself)
    K = len(dls)
    loss, stats, masks = S.lr_consistency(xs[:K], xs[K:], weights, tau, dmax)
    g = S._grads(loss, xs)
    out.append((loss.detach(), stats, masks, g[:K], g[K:]))
  return out


def _lr_check(tag, got, r32, r64):
  loss, masks, stats, gdl, gdr = got
  l64, s64, m64, gl64, gr64 = r64
  l32, s32, m32, gl32, gr32 = r32
  assert torch.equal(m32, m64), 'the case sits on the threshold: float32 and float64 disagree on a mask'
  assert torch.equal(masks.bool(), m64), tag
  assert torch.equal(stats[..., 0], s64[..., 0]) and torch.equal(stats[..., 2], s64[..., 2]), (stats, s64)
  assert bool(((masks == 0) | (masks == 1)).all())
  print('%s: loss %.9g' % (tag, float(loss)))
  ratios = [_within('loss', loss, l32, l64)]
  assert float((stats[..., 1] - s64[..., 1]).abs().max()) <= 1e-6 * float(s64[..., 1].abs().max()) + 1e-300
  for side, g, a, b in (('gdl', gdl, gl32, gl64), ('gdr', gdr, gr32, gr64)):
    for k in range(len(g)):
      assert bool(torch.isfinite(g[k]).all())
      ratios.append(_within('%s[%d]' % (side, k), g[k], a[k], b[k]))
  return ratios


@pytest.mark.parametrize('case', S.CASES, ids=IDS)
def test_lr_parity_with_the_float64_restatement(case):
  _, _, dls, drs = S.make_case(*case)
  tau, dmax = S.params(case)
  got = _lr(dls, drs, S.WEIGHTS[:len(dls)], tau, dmax)
  _lr_check('lr %s' % (case,), got, S.lr_reference(case, torch.float32), S.lr_reference(case, torch.float64))


def _small(H=6, W=20, seed=3):
  """One smooth pair of maps (1, H, W) in [1, 6): every pixel's own is inside [0, dmax = 8]."""
  g = torch.Generator().manual_seed(seed)
  return 1 + 5 * torch.rand(1, H, W, generator=g), 1 + 5 * torch.rand(1, H, W, generator=g)


def _edge(tag, dl, dr, tau=1.5, dmax=8.0):
  got = _lr([dl], [dr], (1.0,), tau, dmax)
  r32, r64 = _lr_refs([dl], [dr], (1.0,), tau, dmax)
  _lr_check(tag, got, r32, r64)
  return got


def test_lr_edges_of_the_row():
  """x == 0 exactly (left view, own = w) and x == W - 1 exactly (right view, own = W - 1 - w): valid, sampled at the row's first and last
  column (x0 = W - 2, t = 1 at the far end)."""
  dl, dr = _small()
  W = dl.shape[-1]
  base = _edge('base', dl, dr)
  dl2, dr2 = dl.clone(), dr.clone()
  for w in range(0, 9):
    dl2[0, w % 6, w] = float(w)
    dr2[0, (w + 1) % 6, W - 1 - w] = float(w)
  got = _edge('x == 0, x == W - 1', dl2, dr2)
  for w in range(0, 9):  # valid: each is counted whatever its e (the reference's `valid` says so; here through the counts)
    e, valid, _ = S.lr_view(dl2.double(), dr2.double(), -1, 1.5, 8.0)
    assert bool(valid[0, w % 6, w]) and float(e[0, w % 6, w]) == abs(w - float(dr2[0, w % 6, 0]))
    e, valid, _ = S.lr_view(dr2.double(), dl2.double(), 1, 1.5, 8.0)
    assert bool(valid[0, (w + 1) % 6, W - 1 - w]) and float(e[0, (w + 1) % 6, W - 1 - w]) == abs(w - float(dl2[0, (w + 1) % 6, W - 1]))
  assert float(got[2][0, 0, 0]) >= float(base[2][0, 0, 0])


def test_lr_own_at_and_above_dmax():
  dl, dr = _small()
  base = _edge('base', dl, dr)
  at, above = dl.clone(), dl.clone()
  at[0, 2, 12] = 8.0
  above[0, 2, 12] = float(torch.nextafter(torch.tensor(8.0), torch.tensor(9.0)))
  got_at, got_above = _edge('own == dmax', at, dr), _edge('own just above dmax', above, dr)
  assert float(base[2][0, 0, 0]) == float(got_at[2][0, 0, 0]) == float(got_above[2][0, 0, 0]) + 1  # left view's N_valid
  e, valid, _ = S.lr_view(above.double(), dr.double(), -1, 1.5, 8.0)
  assert not bool(valid[0, 2, 12]) and bool(S.lr_view(at.double(), dr.double(), -1, 1.5, 8.0)[1][0, 2, 12])


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', '-inf'])
def test_lr_a_non_finite_value_costs_its_pixel_only(bad):
  """In own: that pixel of own's view turns invalid and nothing else of that view.  The same element is `other` for the opposite view:
  there exactly the pixels that sample it turn invalid.  Every gradient stays finite."""
  dl, dr = _small()
  base = _edge('base', dl, dr)
  dl2 = dl.clone()
  dl2[0, 3, 10] = bad
  got = _edge('dl[3, 10] = %s' % bad, dl2, dr)
  assert float(got[2][0, 0, 0]) == float(base[2][0, 0, 0]) - 1  # left view: one pixel fewer
  # right view: the pixels of row 3 whose x0 or x0 + 1 is column 10
  x = torch.arange(20, dtype=torch.float64) + dr[0, 3].double()
  x0 = x.floor().clamp(max=18)
  hit = int((((x0 == 10) | (x0 == 9)) & (x <= 19)).sum())
  assert hit >= 1 and float(got[2][1, 0, 0]) == float(base[2][1, 0, 0]) - hit
  changed = (got[1] != base[1]).nonzero()
  assert bool((changed[:, 3] == 3).all())  # only row 3's mask bytes can differ
  for g in got[3] + got[4]:
    assert bool(torch.isfinite(g).all())


def test_lr_nothing_valid():
  dl, dr = _small()
  got = _edge('all invalid', dl + 20, dr + 20)
  loss, masks, stats, gdl, gdr = got
  assert float(loss) == 0 and not bool(masks.any()) and not bool(stats.any())
  assert not bool(gdl[0].any()) and not bool(gdr[0].any())


def test_lr_four_maps_and_the_four_dimensional_layout():
  case = (2, 40, 24, 4, 12)
  _, _, dls, drs = S.make_case(*case)
  tau, dmax = S.params(case)
  got = _lr(dls, drs, S.WEIGHTS[:4], tau, dmax)
  r32, r64 = _lr_refs(dls, drs, S.WEIGHTS[:4], tau, dmax)
  _lr_check('K = 4', got, r32, r64)
  four = _lr([d.unsqueeze(1) for d in dls], [d.unsqueeze(1) if k % 2 else d for k, d in enumerate(drs)], S.WEIGHTS[:4], tau, dmax)
  assert torch.equal(four[0], got[0]) and torch.equal(four[1], got[1]) and torch.equal(four[2], got[2])
  for a, b in zip(four[3] + four[4], got[3] + got[4]):
    assert a.dim() in (3, 4) and torch.equal(a.reshape(b.shape), b)
  assert four[3][0].shape == (2, 1, 40, 24)


# ------------------------------------------------------------------------------------------------------------- the view loss
def _view(own, other, disps, view, masks=None, want_grad=True, **kw):
  """-> (loss, stats (K, 3), [gdisp_k]) on the CPU through the public entry."""
  ds = [d.detach().to(DEV).requires_grad_(want_grad) for d in disps]
  m = None if masks is None else masks.to(DEV)
  loss, stats = HF.photometric_loss(own.to(DEV), other.to(DEV), ds, S.WEIGHTS[:len(ds)], return_stats=True, view=('left', 'right')[view], masks=m, **kw)
  if want_grad:
    loss.backward()
  return loss.detach().cpu(), stats.cpu(), [d.grad.cpu() if want_grad else None for d in ds]


def _inputs(case, view):
  left, right, dls, drs = S.make_case(*case)
  return (left, right, dls) if view == 0 else (right, left, drs)


@pytest.mark.parametrize('case', S.CASES, ids=IDS)
def test_view_zero_without_a_mask_is_the_loss_of_design_22(case):
  """The new entries with view = 0 and mask = NULL against today's entries: loss, statistics and gradient bit for bit -- the proof
  that templating the kernels moved nothing."""
  left, right, dls, _ = S.make_case(*case)
  K = len(dls)
  l, r = left.to(DEV), right.to(DEV)
  old = [d.to(DEV).requires_grad_(True) for d in dls]
  new = [d.to(DEV).requires_grad_(True) for d in dls]
  prm = HF._photometric_params(K, S.WEIGHTS[:K], 0.85, 0.1, 1.0, None, None)
  la, sa = HF.PhotometricLossFunction.apply(l, r, prm, *old)
  lb, sb = HF.ViewLossFunction.apply(l, r, None, 0, prm, *new)
  (2 * la).backward()
  (2 * lb).backward()
  assert torch.equal(la, lb) and torch.equal(sa, sb) and float(sa[:, 0].min()) > 0
  for a, b in zip(old, new):
    assert torch.equal(a.grad, b.grad) and bool(a.grad.abs().max() > 0)
  lc = HF.photometric_loss(l, r, [d.to(DEV) for d in dls], S.WEIGHTS[:K])
  assert torch.equal(lc, la)


@pytest.mark.parametrize('case', S.CASES, ids=IDS)
@pytest.mark.parametrize('view,masked', [(1, False), (0, True), (1, True), (0, 'blocks'), (1, 'blocks')],
                         ids=['right', 'left-lr', 'right-lr', 'left-blocks', 'right-blocks'])
def test_view_loss_parity_with_the_float64_restatement(case, view, masked):
  """The right view; both views with the consistency masks of the case (independent random maps: hardly a window of nine visible pixels
  is left, so this is the smoothness term and the few windows); both views with the block mask, which keeps most windows."""
  own, other, maps = _inputs(case, view)
  masks = None
  if masked == 'blocks':
    masks = S.block_mask(*case)
  elif masked:
    masks = S.lr_reference(case, torch.float64)[2][view]
  l64, s64, g64 = S.view_reference(case, torch.float64, view, masked)
  l32, s32, g32 = S.view_reference(case, torch.float32, view, masked)
  loss, stats, grads = _view(own, other, maps, view, masks)
  print('view %d %s %s: loss %.9g, N_valid %s' % (view, masked, case, float(loss), stats[:, 0].tolist()))
  assert torch.equal(stats[:, 0], s64[:, 0]), (stats[:, 0], s64[:, 0])
  if masked != True:  # noqa: E712 (the consistency masks leave next to nothing)
    assert float(stats[:, 0].min()) > 0.15 * case[0] * case[1] * case[2]
  _within('loss', loss, l32, l64)
  for k, g in enumerate(grads):
    _within('gdisp[%d]' % k, g, g32[k], g64[k])
  for j in (1, 2):
    assert float((stats[:, j] - s64[:, j]).abs().max()) <= 1e-5 * float(s64[:, j].abs().max())


@pytest.mark.parametrize('view', [0, 1], ids=['left', 'right'])
def test_masks_of_ones_and_of_zeros(view):
  case = S.CASES[2]
  own, other, maps = _inputs(case, view)
  B, H, W, K, _ = case
  plain = _view(own, other, maps, view) if view == 1 else None
  ones = _view(own, other, maps, view, torch.ones(K, B, H, W, dtype=torch.uint8))
  if view == 0:  # the unmasked left view is today's path: compare with it all the same
    plain = _view(own, other, maps, 0)
  assert torch.equal(plain[0], ones[0]) and torch.equal(plain[1], ones[1])
  for a, b in zip(plain[2], ones[2]):
    assert torch.equal(a, b)
  as_bool = _view(own, other, maps, view, torch.ones(K, B, H, W, dtype=torch.bool))
  assert torch.equal(as_bool[0], ones[0])
  loss, stats, grads = _view(own, other, maps, view, torch.zeros(K, B, H, W, dtype=torch.uint8), lam=0.0)
  assert float(loss) == 0 and not bool(stats[:, 0].any()) and all(not bool(g.any()) for g in grads)
  loss, stats, grads = _view(own, other, maps, view, torch.zeros(K, B, H, W, dtype=torch.uint8))
  assert not bool(stats[:, 0].any()) and float(stats[:, 1].abs().max()) == 0 and float(loss) > 0  # the smoothness term is left


# ----------------------------------------------------------------------------------------- repeatability and invariance
def _everything(case, shift=0):
  """Consistency, then both views' loss with its masks, all inputs rolled by `shift` rows -> the tensors to compare."""
  left, right, dls, drs = S.make_case(*case)
  left, right = left.roll(shift, 2), right.roll(shift, 2)
  dls, drs = [d.roll(shift, 1) for d in dls], [d.roll(shift, 1) for d in drs]
  tau, dmax = S.params(case)
  lr = _lr(dls, drs, S.WEIGHTS[:len(dls)], tau, dmax)
  vl = _view(left, right, dls, 0, lr[1][0])
  vr = _view(right, left, drs, 1, lr[1][1])
  vb = _view(right, left, drs, 1, S.block_mask(*case).roll(shift, 2))
  return {'rolling': [lr[1]] + lr[3] + lr[4] + vl[2] + vr[2] + vb[2], 'scalars': [lr[0], lr[2], vl[0], vl[1], vr[0], vr[1], vb[0], vb[1]]}


@pytest.fixture(scope='module')
def unrolled():
  return _everything(S.CASES[3])


def test_repeatable_on_any_stream(unrolled):
  second = _everything(S.CASES[3])
  side = torch.cuda.Stream(DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    third = _everything(S.CASES[3])
  side.synchronize()
  for other in (second, third):
    for key in ('rolling', 'scalars'):
      for a, b in zip(unrolled[key], other[key]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('shift', [1, 33])
def test_rolling_the_rows_rolls_masks_and_gradients(unrolled, shift):
  """H is periodic and a pixel's arithmetic does not depend on where its row lies: masks, gdl, gdr and gdisp roll bit for bit.  The
  counts are equal; the fp64 sums are taken in another order."""
  rolled = _everything(S.CASES[3], shift)
  for a, b in zip(unrolled['rolling'], rolled['rolling']):
    assert torch.equal(a.roll(shift, a.dim() - 2), b)
  for a, b in zip(unrolled['scalars'], rolled['scalars']):
    assert float((a.double() - b.double()).abs().max()) <= 2.0 ** -22 * float(a.double().abs().max())
  assert torch.equal(unrolled['scalars'][1][..., 0], rolled['scalars'][1][..., 0]) and torch.equal(unrolled['scalars'][1][..., 2], rolled['scalars'][1][..., 2])


# ------------------------------------------------------------------------------------------------------------------ the models
def _grads_of(module):
  return {k: (None if p.grad is None else p.grad.clone()) for k, p in module.named_parameters()}


def test_mode_disparity_trains_both_views():
  import recipe
  import test_gpu_photometric as TP
  from models import stage3d
  from no_vendor import no_vendor_arithmetic
  net, maxdisp, H, W = TP._tiny_disparity()
  left, right = [t.to(DEV) for t in recipe.recipe_images(2, H, W, 311)]
  wts = (0.5, 0.7, 1.0)
  with no_vendor_arithmetic():
    loss, pl, pr = net.forward_selfsup_loss(left, right, lr_weight=0.5, tau=2.0)
    loss.backward()
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and len(pl) == len(pr) == 3 and pr[2].shape == (2, 1, H, W)
    got = _grads_of(net)
    for k, g in got.items():
      assert g is not None and bool(torch.isfinite(g).all()), k
    assert any(bool(g.abs().max() > 0) for g in got.values())
    net.zero_grad(set_to_none=True)
    # the same pieces by hand
    size = (maxdisp, H, W)
    hl = tuple(stage3d.head(c, size) for c in net._logits(left, right))
    hr = tuple(stage3d.head(c, size).flip(3) for c in net._logits(right.flip(3).contiguous(), left.flip(3).contiguous()))
    lr, masks = HF.lr_consistency(hl, hr, wts, tau=2.0, dmax=maxdisp, return_masks=True)
    want = (HF.photometric_loss(left, right, hl, wts, view='left', masks=masks[0]) +
            HF.photometric_loss(right, left, hr, wts, view='right', masks=masks[1]))
    want = want + 0.5 * lr
    want.backward()
    assert torch.equal(want, loss)
    for p, q in zip(pl + pr, hl + hr):
      assert torch.equal(p, q.detach()) and not p.requires_grad
    for k, g in _grads_of(net).items():
      assert torch.equal(g, got[k]), k
    # without the remedy: the two view losses and nothing else
    plain, ql, qr = net.forward_selfsup_loss(left, right, occlusion=False, lr_weight=0)
    assert torch.equal(ql[2], pl[2]) and torch.equal(qr[2], pr[2])
    two = HF.photometric_loss(left, right, ql, wts) + HF.photometric_loss(right, left, qr, wts, view='right')
    assert torch.equal(plain.detach(), two)


def test_mode_multiview_adapts_stage_one_with_the_remedy():
  import test_gpu_rig as TR
  rig = CameraRig.deep360().subset(('12', '13', '23'))
  net, maxdepth, H, W = TR._tiny_net(rig)
  assert (H, W) == (64, 32)
  with pytest.raises(RuntimeError, match='disparity.train'):
    net.selfsup_loss(TR._u8_frames(1, 6, H, W, 5))
  net.train()
  u8 = TR._u8_frames(1, 6, H, W, 47)
  frames = TR._host_normalised(u8)
  left, right, _, _ = net._ingest(frames)
  want, preds, _ = net.disparity.forward_selfsup_loss(left, right)
  want.backward()
  ref = _grads_of(net.disparity)
  for src in (frames, u8):
    net.zero_grad(set_to_none=True)
    loss, disp = net.selfsup_loss(src)
    loss.backward()
    assert torch.equal(loss, want) and torch.equal(disp, preds[2]) and disp.shape == (3, 1, H, W) and not disp.requires_grad
    for k, p in net.named_parameters():
      if k.startswith('fusion.'):
        assert p.grad is None, k
    got = _grads_of(net.disparity)
    assert all(g is not None for g in got.values())
    for k, g in got.items():
      assert torch.equal(g, ref[k]), k
