"""The gradient through the confidence and through the half-size path, CPU tier: the three entries are declared, exported and bound and
check their arguments on the host (no launch); the options of ModeMultiView and disp2depth_frames_gpu; the float64 oracle of the
head's confidence gradient (oracle/mode_ref.py confidence_map under autograd) against the closed form p_d (m_d - conf) gconf and against
the reference's own three-grid_sample expression; the host references of tests/conf_grad_ref.py against autograd."""
import ctypes
import os
import re

import pytest
import torch

import conf_grad_ref as C
import mode_hip
import models
from oracle import mode_ref
from utils import geometry as HG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mode_head_bwd_conf', 'mode_multiview_handoff_bwd_full', 'mode_decimate2_bwd')
NULL, ONE = ctypes.c_void_p(0), ctypes.c_void_p(16)


def test_entries_are_declared_exported_and_bound():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mode_hip.h')).read(), flags=re.S)
  lib = mode_hip.lib()
  for name in NEW:
    assert re.search(r'\bint\s+%s\s*\(' % name, src), name
    assert hasattr(lib, name) and name in mode_hip.SIGNATURES, name
  assert len(mode_hip.SIGNATURES['mode_head_bwd_conf'][1]) == len(mode_hip.SIGNATURES['mode_head_bwd'][1]) + 3
  assert len(mode_hip.SIGNATURES['mode_multiview_handoff_bwd_full'][1]) == len(mode_hip.SIGNATURES['mode_multiview_handoff_bwd'][1]) + 1
  assert mode_hip.SIGNATURES['mode_decimate2_bwd'] == mode_hip.SIGNATURES['mode_decimate2']
  assert lib.mode_hip_abi_version() == 31  # additions only: no existing signature changed


def test_head_bwd_conf_validates_on_the_host():
  lib = mode_hip.lib()

  def call(logits=ONE, pred=ONE, conf=ONE, gpred=ONE, gconf=ONE, gl=ONE, ws=ONE, B=1, D4=4, H4=6, W4=8, D=16, H=24, W=32):
    return lib.mode_head_bwd_conf(logits, pred, conf, gpred, gconf, gl, ws, B, D4, H4, W4, D, H, W, NULL)

  for kw in ({'B': -1}, {'D4': 0}, {'H4': 0}, {'W4': -3}, {'D': 0}, {'H': 0}, {'W': 0}):
    assert call(**kw) == -1 and b'mode_head_bwd_conf: non-positive size' in lib.mode_last_error(), kw
  for kw in ('logits', 'pred', 'conf', 'gpred', 'gconf', 'gl'):
    assert call(**{kw: NULL}) == -1 and b'mode_head_bwd_conf: null pointer' in lib.mode_last_error(), kw
  assert call(ws=NULL) == -3 and b'workspace' in lib.mode_last_error()
  assert call(B=0, logits=NULL, pred=NULL, conf=NULL, gpred=NULL, gconf=NULL, gl=NULL, ws=NULL) == 0  # nothing to do


def test_handoff_bwd_full_validates_on_the_host():
  lib = mode_hip.lib()
  b6 = (ctypes.c_float * 6)(*[1.0] * 6)
  xf = (ctypes.c_double * 36)()

  def call(F=1, H=64, W=32, disp=ONE, gout=ONE, keys=ONE, base=ctypes.cast(b6, ctypes.c_void_p), trig=ONE, x=ctypes.cast(xf, ctypes.c_void_p),
           rowptr=ONE, target=ONE, weight=ONE, n=16, flags=0, gdisp=ONE, gconf=ONE):
    return lib.mode_multiview_handoff_bwd_full(disp, gout, keys, F, H, W, base, trig, x, rowptr, target, weight, n, flags, gdisp, gconf, NULL)

  assert call(F=-1) == -1 and b'mode_multiview_handoff_bwd_full: bad size' in lib.mode_last_error()
  assert call(H=0) == -1 and call(W=-4) == -1
  assert call(F=1 << 10, H=1024, W=1024) == -1 and b'bad size' in lib.mode_last_error()  # 3 F H W >= 2^31
  assert call(flags=4) == -1 and b'unknown flags' in lib.mode_last_error()
  assert call(flags=HG.MV_DEPTH_ONLY) == -1 and b'no confidence channels' in lib.mode_last_error()
  assert call(flags=HG.MV_CONF_PNG) == -1 and b'piecewise constant' in lib.mode_last_error()
  assert call(flags=HG.MV_CONF_PNG | HG.MV_DEPTH_ONLY) == -1
  assert call(n=-1) == -1 and b'adjoint' in lib.mode_last_error()
  assert call(n=8 * 64 * 32 + 1) == -1 and b'adjoint' in lib.mode_last_error()
  for kw in ('disp', 'gout', 'base', 'trig', 'x', 'rowptr', 'target', 'weight', 'gdisp', 'gconf'):
    assert call(**{kw: NULL}) == -1 and b'null pointer' in lib.mode_last_error(), kw
  assert call(keys=NULL) == -3 and b'key planes' in lib.mode_last_error()
  assert call(keys=ctypes.c_void_p(20)) == -3 and b'unaligned' in lib.mode_last_error()
  assert call(F=0, disp=NULL, gout=NULL, keys=NULL, gdisp=NULL, gconf=NULL) == 0  # nothing to do
  # the existing entry still takes both flags
  assert lib.mode_multiview_handoff_bwd(ONE, ONE, ONE, 0, 64, 32, ctypes.cast(b6, ctypes.c_void_p), ONE, ctypes.cast(xf, ctypes.c_void_p), ONE, ONE,
                                        ONE, 16, HG.MV_CONF_PNG | HG.MV_DEPTH_ONLY, ONE, NULL) == 0


def test_decimate2_bwd_validates_on_the_host():
  lib = mode_hip.lib()
  call = lambda gout=ONE, gin=ctypes.c_void_p(32), planes=1, H=4, W=4: lib.mode_decimate2_bwd(gout, gin, planes, H, W, NULL)
  assert call(planes=-1) == -1 and b'mode_decimate2_bwd: bad size' in lib.mode_last_error()
  assert call(H=0) == -1 and call(W=-2) == -1
  assert call(planes=1 << 20, H=1 << 10, W=1 << 10) == -1 and b'too large' in lib.mode_last_error()  # planes H W >= 2^31, as the forward
  assert lib.mode_decimate2(ONE, ctypes.c_void_p(32), 1 << 20, 1 << 10, 1 << 10, NULL) == -1
  assert call(gout=NULL) == -1 and b'null pointer' in lib.mode_last_error()
  assert call(gin=NULL) == -1 and b'null pointer' in lib.mode_last_error()
  assert call(gin=ONE) == -1 and b'in-place' in lib.mode_last_error()
  assert call(planes=0, gout=NULL, gin=NULL) == 0  # nothing to do


def test_multiview_options():
  kw = dict(channels=(8, 16, 32, 64))
  with pytest.raises(ValueError, match='rounding'):
    models.ModeMultiView(16, 10., 64, 32, handoff_grad='full', conf_png=True, **kw)
  with pytest.raises(ValueError, match='rounding'):
    models.ModeMultiView(16, 10., 64, 32, handoff_grad='full', **kw)  # conf_png=True is the default
  with pytest.raises(ValueError, match='handoff_grad'):
    models.ModeMultiView(16, 10., 64, 32, handoff_grad='confidence', **kw)
  plain = models.ModeMultiView(16, 10., 64, 32, **kw)
  full = models.ModeMultiView(16, 10., 64, 32, handoff_grad='full', conf_png=False, **kw)
  assert plain.handoff_grad == 'depth' and full.handoff_grad == 'full'
  assert list(full.state_dict().keys()) == list(plain.state_dict().keys())
  assert [tuple(v.shape) for v in full.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
  # Baseline reads no confidence: nothing is rounded on its path
  models.ModeMultiView(16, 10., 64, 32, fusion='Baseline', handoff_grad='full', conf_png=True)
  # the refusals come before any device work; the half-size refusal is that of the default module alone
  frames, gt = torch.zeros(1, 12, 64, 32, 3, dtype=torch.uint8), torch.ones(1, 64, 32)
  half = models.ModeMultiView(16, 10., 64, 32, resize=True, **kw).train()
  with pytest.raises(ValueError, match='no backward'):
    half.fusion_loss(frames, gt)
  half_full = models.ModeMultiView(16, 10., 64, 32, resize=True, handoff_grad='full', conf_png=False, **kw).train()
  with pytest.raises(NotImplementedError):  # past the refusal, at the device check
    half_full.fusion_loss(frames, gt)


def test_handoff_options_on_cpu_tensors():
  d, c = torch.zeros(1, 6, 64, 32, requires_grad=True), torch.zeros(1, 6, 64, 32, requires_grad=True)
  with pytest.raises(ValueError, match='conf_png'):
    HG.disp2depth_frames_gpu(d, c, conf_grad=True, conf_png=True)
  with pytest.raises(NotImplementedError):
    HG.disp2depth_frames_gpu(d, c, conf_grad=True)
  with pytest.raises(NotImplementedError):
    HG.disp2depth_frames_bwd(d.detach(), torch.zeros(1, 12, 64, 32), torch.zeros(1, 3, 64, 32, dtype=torch.int64), conf_grad=True)


def test_functional_refuses_cpu_tensors():
  from mode_hip import functional as HF
  lg = torch.zeros(1, 1, 4, 6, 8, requires_grad=True)
  with pytest.raises(NotImplementedError):
    HF.head_conf(lg, (16, 24, 32))
  with pytest.raises(NotImplementedError):
    HF.decimate2(torch.zeros(2, 4, 4, requires_grad=True))
  with pytest.raises(NotImplementedError):
    HF.decimate2_bwd(torch.zeros(2, 2, 2), (2, 4, 4))


# ------------------------------------------------------------------------------------------------ the oracle of the head
BORDER = ((2, 4, 6, 8), 4, 8.0)  # logits = standard normal x 8: sharp columns, many windows at the borders of the disparity axis


def _border_case():
  (B, D4, H4, W4), ratio, scale = BORDER
  size = (D4 * ratio, H4 * ratio, W4 * ratio)
  return C.rand((B, 1, D4, H4, W4), 61, scale), C.rand((B, 1) + size[1:], 63), size


def test_oracle_gradient_is_the_closed_form():
  lg, gconf, (D, H, W) = _border_case()
  up = torch.nn.functional.interpolate(lg.double(), [D, H, W], mode='trilinear', align_corners=True).squeeze(1).requires_grad_(True)
  prob = torch.softmax(up, 1)
  pred = (prob * torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)).sum(1, keepdim=True).detach()
  conf = mode_ref.confidence_map(pred, prob)
  g, = torch.autograd.grad(conf, up, gconf.double())
  m = C.window_multiplicity(pred, D)
  assert float(m.sum(1).min()) == 3 and float(m.max()) == 2  # three indices per pixel; one counted twice at a border
  closed = prob.detach() * (m - conf.detach()) * gconf.double()
  assert float((g - closed).abs().max()) <= 1e-13 * max(1.0, float(closed.abs().max()))
  r = torch.round(pred)
  at_border, top = float(((r == 0) | (r == D - 1)).double().mean()), float(conf.detach().max())
  print('round(pred) at 0 or D - 1 at %.1f %% of the pixels; conf up to %.4f' % (100 * at_border, top))
  assert at_border > 0.05 and top > 1.5  # the case has border windows, where the confidence exceeds 1


def test_oracle_is_the_three_grid_samples_of_the_reference():
  lg, gconf, (D, H, W) = _border_case()
  grads, values = [], []
  for fn in (mode_ref.confidence_map, C.confidence_three_grid_samples):
    la = lg.double().requires_grad_(True)
    pred, prob = mode_ref.disparity_head(la, D, H, W, return_prob=True)
    conf = fn(pred.detach(), prob)
    g, = torch.autograd.grad(conf, la, gconf.double())
    grads.append(g)
    values.append(conf.detach())
  assert torch.equal(values[0], values[1]) and torch.equal(grads[0], grads[1])
  assert float(grads[0].abs().max()) > 0
  # round(pred) passes nothing: with the prediction attached the gradient is the same
  la = lg.double().requires_grad_(True)
  pred, prob = mode_ref.disparity_head(la, D, H, W, return_prob=True)
  g, = torch.autograd.grad(C.confidence_three_grid_samples(pred, prob), la, gconf.double())
  assert torch.equal(g, grads[0])


def test_head_reference_splits_into_its_two_terms():
  lg, gconf, size = _border_case()
  gpred = C.rand(tuple(gconf.shape), 62)
  ref = C.head_reference(lg, gpred, gconf, size)
  la = lg.double().requires_grad_(True)
  pred, prob = mode_ref.disparity_head(la, *size, return_prob=True)
  conf = mode_ref.confidence_map(pred.detach(), prob)
  both, = torch.autograd.grad((pred * gpred.double()).sum() + (conf * gconf.double()).sum(), la)
  assert float((both - ref['g_pred'] - ref['g_conf']).abs().max()) <= 1e-12 * float(both.abs().max())
  masked, share = C.masked_gconf(lg, gconf, size)
  assert share <= 0.01 and bool((masked[ref['unstable']] == 0).all()) and torch.equal(masked[~ref['unstable']], gconf[~ref['unstable']])


# ------------------------------------------------------------------------------------------------ the other host references
def test_decimate2_reference_is_the_adjoint():
  for shape in ((3, 5, 7), (2, 4, 8), (1, 1, 1)):
    x = torch.randn(shape, dtype=torch.float64, requires_grad=True, generator=torch.Generator().manual_seed(5))
    y = x[..., ::2, ::2]
    g = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    want, = torch.autograd.grad(y, x, g)
    got = C.decimate2_bwd(g, shape)
    assert torch.equal(got, want) and not bool(torch.signbit(got[got == 0]).any())


def test_handoff_confidence_reference():
  F_, H, W = 1, 8, 4
  g = torch.Generator().manual_seed(3)
  conf = torch.rand(F_, 6, H, W, generator=g, dtype=torch.float64)
  winners = torch.stack([torch.randperm(H * W, generator=g).view(H, W) for _ in range(3)])[None]  # a source wins at most one target
  winners[torch.rand(F_, 3, H, W, generator=g) < 0.2] = -1
  gout = torch.randn(F_, 6, H, W, generator=g, dtype=torch.float64)
  c = conf.clone().requires_grad_(True)
  assert torch.autograd.gradcheck(lambda x: C.handoff_conf(x, winners), (c,), eps=1e-6, atol=1e-8, rtol=1e-8)  # linear in conf
  got = C.handoff_conf_gradient(conf, winners, gout)
  assert torch.equal(got[:, 0], gout[:, 0])
  assert torch.equal(got[:, 3:], C.winners_scatter(winners, gout[:, 3:]))
  for p, pair in ((1, '13'), (2, '14')):
    # the rotation's taps sum to 1 per target (border padding): the adjoint keeps the total
    assert abs(float(got[:, p].sum()) - float(gout[:, p].sum())) <= 1e-12 * float(gout[:, p].abs().sum())
