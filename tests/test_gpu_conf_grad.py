"""The gradient through the confidence and through the half-size path, GPU tier: mode_head_bwd_conf against the float64 oracle
(oracle/mode_ref.py under autograd), mode_multiview_handoff_bwd_full on the cases of tests/test_gpu_handoff_grad.py (exact where the
gradient is a copy or a pick, DESIGN 4's standing criterion where it is a sum), mode_decimate2_bwd bit for bit, and
ModeMultiView(handoff_grad='full').fusion_loss against the hand composition of public pieces with torch.equal.

The head's bound is that of test_head_fwd_bwd_conf: max |glogits - ref| < 1e-4 max(1, max |ref|).  The confidence's upstream gradient is
zeroed where the float64 prediction lies within 1e-3 of a half-integer (either rounding is legitimate there, and the two place the
window one disparity apart); at most 1 % of a case's pixels may be zeroed that way."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import conf_grad_ref as C
import handoff_ref as R
import recipe
import test_gpu_handoff_grad as TG

import models
from dataloader import gpu_ingest
from mode_hip import functional as HF
from models import mode_multiview
from utils import geometry as HG

DEV = 'cuda:0'
bits = lambda t: t.view(torch.int32)

# (B, D4, H4, W4), ratio, scale of the logits
HEAD_CASES = [
    ((2, 4, 6, 8), 4, 3.0),      # one-kernel fast form
    ((1, 12, 5, 7), 4, 3.0),     # fast form, odd sizes
    ((1, 3, 4, 4), 3, 3.0),      # generic form, ratio 3
    ((1, 5, 4, 6), 4, 3.0),      # generic form, ratio 4
    ((2, 48, 8, 16), 4, 3.0),    # the network's D4
    ((1, 48, 4, 128), 4, 3.0),   # the network's 512-wide row
    ((1, 4, 2, 130), 4, 3.0),    # W = 520: the two-kernel form
    ((2, 4, 6, 8), 4, 8.0),      # sharp columns: windows at the borders of the disparity axis
]
HEAD_IDS = ['%s-x%d-s%g' % ('x'.join(str(n) for n in s), r, k) for s, r, k in HEAD_CASES]


@functools.lru_cache(maxsize=None)
def _head_case(shape, ratio, scale):
  """Inputs and the float64 references of one head case, computed once and shared (nothing below writes to them)."""
  B, D4, H4, W4 = shape
  size = (D4 * ratio, H4 * ratio, W4 * ratio)
  lg = C.rand((B, 1, D4, H4, W4), 61, scale)
  gpred = C.rand((B, 1) + size[1:], 62)
  gconf, zeroed = C.masked_gconf(lg, C.rand((B, 1) + size[1:], 63), size)
  ref = C.head_reference(lg, gpred, gconf, size)
  return dict(size=size, lg=lg, gpred=gpred, gconf=gconf, zeroed=zeroed, ref=ref)


def _close(got, want, what):
  err = float((got.double().cpu() - want).abs().max())
  bound = 1e-4 * max(1.0, float(want.abs().max()))
  print('%s: max err %.3e (bound %.3e, max |ref| %.3e)' % (what, err, bound, float(want.abs().max())))
  assert err < bound, (what, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize('case', HEAD_CASES, ids=HEAD_IDS)
def test_head_bwd_conf_against_float64(case):
  z = _head_case(*case)
  size, ref = z['size'], z['ref']
  print('%s: %.3f %% of the pixels within 1e-3 of a half-integer (their gconf zeroed)' % (case, 100 * z['zeroed']))
  assert z['zeroed'] <= 0.01
  lg, gp, gc = z['lg'].to(DEV), z['gpred'].to(DEV), z['gconf'].to(DEV)
  pred, conf = HF.head_fwd(lg, size, with_confidence=True)
  both = HF.head_bwd_conf(lg, pred, conf, gp, gc, size)
  assert both.shape == lg.shape and both.dtype == torch.float32
  _close(both, ref['g_pred'] + ref['g_conf'], 'both terms')
  # without a confidence gradient: the bits of mode_head_bwd
  zero = torch.zeros_like(gc)
  assert torch.equal(bits(HF.head_bwd_conf(lg, pred, conf, gp, zero, size)), bits(HF.head_bwd(lg, gp, size)))
  # the confidence term alone
  alone = HF.head_bwd_conf(lg, pred, conf, torch.zeros_like(gp), gc, size)
  _close(alone, ref['g_conf'], 'confidence term alone')
  assert float(ref['g_conf'].abs().max()) > 0
  # bit-repeatable
  assert torch.equal(bits(HF.head_bwd_conf(lg, pred, conf, gp, gc, size)), bits(both))
  # one autograd node with the forward's bits and the entry's gradient; a missing upstream gradient counts as zeros
  leaf = lg.clone().requires_grad_(True)
  p2, c2 = HF.head_conf(leaf, size)
  assert torch.equal(bits(p2), bits(pred)) and torch.equal(bits(c2), bits(conf)) and p2.grad_fn is c2.grad_fn
  g, = torch.autograd.grad((p2, c2), leaf, (gp, gc), retain_graph=True)
  assert torch.equal(bits(g), bits(both))
  g, = torch.autograd.grad(p2, leaf, gp, retain_graph=True)
  assert torch.equal(bits(g), bits(HF.head_bwd(lg, gp, size)))
  g, = torch.autograd.grad(c2, leaf, gc)
  assert torch.equal(bits(g), bits(alone))


@pytest.mark.gpu
def test_head_conf_border_case_has_border_windows():
  """The last case is there for the windows at 0 and D - 1, where an index counts twice and the confidence exceeds 1."""
  z = _head_case(*HEAD_CASES[-1])
  D = z['size'][0]
  r = torch.round(z['ref']['pred'])
  assert float(((r == 0) | (r == D - 1)).double().mean()) > 0.05 and float(z['ref']['conf'].max()) > 1.5
  pred, conf = HF.head_fwd(z['lg'].to(DEV), z['size'], with_confidence=True)
  assert float(conf.max()) > 1.5


# ------------------------------------------------------------------------------------------------ the hand-off
def _full(z, dbname):
  gdisp, gconf = HG.disp2depth_frames_bwd(z['d'], z['gout'].to(DEV), z['keys'], dbname, conf_grad=True)
  return gdisp.cpu(), gconf.cpu()


@functools.lru_cache(maxsize=None)
def _conf_refs(F, H, W, dbname):
  z = TG._case(F, H, W, dbname)
  gc = z['gout'][:, 1::2].contiguous()
  den = torch.zeros(F, 6, H, W, dtype=torch.float64)
  for f in range(F):
    for p, pair in ((1, '13'), (2, '14')):
      den[f, p] = R.rotation_adjoint_abs(gc[f, p], pair)
  return dict(gc=gc, den=den, ref64=C.handoff_conf_gradient(z['conf'], z['winner'], gc, torch.float64),
              ref32=C.handoff_conf_gradient(z['conf'], z['winner'], gc, torch.float32).double())


@pytest.mark.gpu
@pytest.mark.parametrize('dbname', ['Deep360', 'other'])
@pytest.mark.parametrize('size', TG.SIZES, ids=['x'.join(str(n) for n in s) for s in TG.SIZES])
def test_handoff_bwd_full(size, dbname):
  F, H, W = size
  z, c = TG._case(*size, dbname), _conf_refs(*size, dbname)
  gdisp, gconf = _full(z, dbname)
  assert gconf.shape == z['disp'].shape and gconf.dtype == torch.float32 and not bool(torch.isnan(gconf).any())
  assert torch.equal(bits(gdisp), bits(TG._bwd(z, dbname, False)))  # the existing entry's bits
  assert torch.equal(bits(gconf[:, 0]), bits(z['gout'][:, 1]))      # pair 12: a copy
  # pairs 23, 24, 34: the winner's pick, +0.0 everywhere else
  want = C.winners_scatter(z['winner'], c['gc'][:, 3:])
  assert torch.equal(bits(gconf[:, 3:]), bits(want))
  assert torch.equal(want, c['ref64'][:, 3:].float())  # (the scatter is what autograd finds)
  capped = z['capped']
  no_slope = z['won'] & (z['disp'][:, 3:] == 0)
  print('%s %s: %d winners, %d of them capped, %d with disp == 0' % (size, dbname, int(z['won'].sum()), int(capped.sum()), int(no_slope.sum())))
  assert bool(capped.any()) and bool(no_slope.any())
  assert bool((gconf[:, 3:][capped] != 0).any()) and bool((gconf[:, 3:][no_slope] != 0).any())
  assert torch.equal(gconf[:, 3:][capped], want[capped]) and torch.equal(gconf[:, 3:][no_slope], want[no_slope])
  assert bool((gdisp[:, 3:][capped] == 0).all()) and bool((gdisp[:, 3:][no_slope] == 0).all())  # (the depth passes nothing there)
  # pairs 13, 14: the standing criterion, nothing left out, in units of sum_k |w_k gout_tk|
  worst = [0.0, 0.0]
  for f in range(F):
    for p in (1, 2):
      e = (gconf[f, p].double() - c['ref64'][f, p]).abs() / (c['den'][f, p] + TG.TINY)
      y = (c['ref32'][f, p] - c['ref64'][f, p]).abs() / (c['den'][f, p] + TG.TINY)
      m, x, ym, yx = float(e.mean()), float(e.max()), float(y.mean()), float(y.max())
      print('%s %s frame %d pair %s: kernel mean %.3e max %.3e; float32 autograd mean %.3e max %.3e' % (size, dbname, f, HG.PAIRS[p], m, x, ym, yx))
      worst = [max(worst[0], m / max(ym, TG.FLOOR / 2)), max(worst[1], x / max(yx, TG.FLOOR / 3))]
      assert m <= max(2 * ym, TG.FLOOR) and x <= max(3 * yx, TG.FLOOR), (f, p, m, x, ym, yx)
  print('%s %s: largest ratio of the means %.3f (bound 2), of the maxima %.3f (bound 3)' % (size, dbname, worst[0], worst[1]))
  # the confidence does not depend on the disparity: sources with disp == 0 get their sum
  dead = z['disp'][:, 1:3] == 0
  assert bool(dead.any()) and bool((gconf[:, 1:3][dead] != 0).any())


@pytest.mark.gpu
def test_handoff_full_repeatable_independent_and_wired_into_autograd():
  F, H, W = 2, 48, 24
  z = TG._case(F, H, W, 'Deep360')
  gdisp, gconf = _full(z, 'Deep360')
  again = _full(z, 'Deep360')
  assert torch.equal(bits(again[0]), bits(gdisp)) and torch.equal(bits(again[1]), bits(gconf))
  # frame 1 a copy of frame 0: frame 0 of the F = 2 call is the F = 1 call (plane and key-plane offsets)
  d1, c1, g1 = z['d'][:1], z['c'][:1], z['gout'][:1].to(DEV)
  d2, c2, g2 = torch.cat((d1, d1)), torch.cat((c1, c1)), torch.cat((g1, g1))
  _, k1 = HG.disp2depth_frames_gpu(d1, c1, return_keys=True)
  _, k2 = HG.disp2depth_frames_gpu(d2, c2, return_keys=True)
  one, two = HG.disp2depth_frames_bwd(d1, g1, k1, conf_grad=True), HG.disp2depth_frames_bwd(d2, g2, k2, conf_grad=True)
  for a, b, first in zip(one, two, (gdisp, gconf)):
    assert torch.equal(b[0], b[1]) and torch.equal(b[:1], a) and torch.equal(a.cpu(), first[:1])
  # autograd returns the entry's bits for both inputs, alone or together
  g = z['gout'].to(DEV)
  d, c = z['d'].clone().requires_grad_(True), z['c'].clone().requires_grad_(True)
  out = HG.disp2depth_frames_gpu(d, c, conf_grad=True)
  assert out.requires_grad and torch.equal(out, z['out'])
  gd, gc = torch.autograd.grad(out, (d, c), g, retain_graph=True)
  assert torch.equal(bits(gd.cpu()), bits(gdisp)) and torch.equal(bits(gc.cpu()), bits(gconf))
  only, = torch.autograd.grad(out, c, g)
  assert torch.equal(bits(only.cpu()), bits(gconf))
  c = z['c'].clone().requires_grad_(True)
  only, = torch.autograd.grad(HG.disp2depth_frames_gpu(z['d'], c, conf_grad=True), c, g)
  assert torch.equal(bits(only.cpu()), bits(gconf))
  # depth_only has no confidence channels: None for conf, the depth's bits; conf_png is refused
  d, c = z['d'].clone().requires_grad_(True), z['c'].clone().requires_grad_(True)
  gd, gc = torch.autograd.grad(HG.disp2depth_frames_gpu(d, c, depth_only=True, conf_grad=True), (d, c), z['gd'].to(DEV), allow_unused=True)
  assert gc is None and torch.equal(bits(gd.cpu()), bits(gdisp))
  got = HG.disp2depth_frames_bwd(z['d'], z['gd'].to(DEV), z['keys'], depth_only=True, conf_grad=True)
  assert got[1] is None and torch.equal(bits(got[0].cpu()), bits(gdisp))
  with pytest.raises(ValueError, match='conf_png'):
    HG.disp2depth_frames_gpu(d, c, conf_png=True, conf_grad=True)
  # the default stays today's: nothing for the confidence
  d, c = z['d'].clone().requires_grad_(True), z['c'].clone().requires_grad_(True)
  gd, gc = torch.autograd.grad(HG.disp2depth_frames_gpu(d, c), (d, c), g, allow_unused=True)
  assert gc is None and torch.equal(bits(gd.cpu()), bits(gdisp))


# ------------------------------------------------------------------------------------------------ the decimation
@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 4, 8), (1, 1, 1)], ids=['3x5x7', '2x4x8', '1x1x1'])
def test_decimate2_bwd(shape):
  H, W = shape[-2:]
  g = C.rand(shape[:-2] + ((H + 1) // 2, (W + 1) // 2), 41 + sum(shape))
  want = C.decimate2_bwd(g, shape)
  got = HF.decimate2_bwd(g.to(DEV), shape).cpu()
  assert got.shape == want.shape and torch.equal(bits(got), bits(want))  # bit for bit: the zeros are +0.0
  x = C.rand(shape, 43 + sum(shape)).to(DEV)
  leaf = x.clone().requires_grad_(True)
  y = HF.decimate2(leaf)
  assert y.requires_grad and torch.equal(y, HF.decimate2(x)) and torch.equal(y.cpu(), x.cpu()[..., ::2, ::2])
  gx, = torch.autograd.grad(y, leaf, g.to(DEV))
  assert torch.equal(bits(gx.cpu()), bits(want))
  assert HF.decimate2(x).grad_fn is None
  with torch.no_grad():
    assert HF.decimate2(leaf).grad_fn is None
  # a buffer that is not 16-byte aligned takes single stores: the same bits
  if x.numel() >= 2:
    from mode_hip import check, lib, ptr, stream_of
    buf = torch.full((x.numel() + 1,), float('nan'), device=DEV)
    gd = g.to(DEV)
    check(lib().mode_decimate2_bwd(ptr(gd), ptr(buf[1:]), x.numel() // (H * W), H, W, stream_of(buf)), 'mode_decimate2_bwd')
    assert torch.equal(bits(buf[1:].cpu().view(shape)), bits(want)) and bool(torch.isnan(buf[0]))


# ------------------------------------------------------------------------------------------------ fusion_loss
def _net(**kw):
  """The tiny net of tests/test_gpu_handoff_grad.py (64 x 32, 16 disparities) with the options of this feature."""
  maxdisp, H, W, sd = TG._disparity_state('model_wc_tiny.npz')
  zf = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'))
  cfg = zf['cfg']
  maxdepth, seed, channels = float(cfg[0]), int(cfg[4]), tuple(int(c) for c in cfg[5:])
  manifest = [(k, tuple(s)) for k, s in json.loads(str(zf['manifest']))]
  net = models.ModeMultiView(maxdisp, maxdepth, H, W, channels=channels, **kw)
  net.disparity.load_state_dict(sd)
  net.fusion.load_state_dict(recipe.recipe_state(manifest, seed))
  return net.to(DEV), maxdisp, maxdepth, H, W


def _hand(hand, frames, gt, maxdisp, maxdepth, resize):
  """The two-step composition: stage 1 to HF.head_conf; the hand-off with conf_grad, the fusion network and the loss on detached leaves;
  then both leaves' gradients back through the head.  -> (loss, output, the confidence leaf's gradient)."""
  H, W = hand.height, hand.width
  if frames.dtype == torch.uint8:
    left, right, rgb = gpu_ingest.frames_u8_gpu(frames.contiguous(), want_rgb=not resize)
  else:
    left, right, rgb = mode_multiview.split_frames(frames)
  pred, conf = HF.head_conf(hand.disparity._logits(left, right)[2], (maxdisp, H, W))
  lp, lc = pred.detach().requires_grad_(True), conf.detach().requires_grad_(True)
  x = HG.disp2depth_frames_gpu(lp, lc, conf_png=False, conf_grad=True)
  if resize:
    x, rgb, gt = HF.decimate2(x), gpu_ingest.rgb_half_gpu(frames.contiguous()), gt[:, ::2, ::2]
  out = hand.fusion.feature_extraction(x, rgb)
  want = HF.silog_loss(out, gt, gt <= maxdepth, 0.5)
  want.backward()
  assert lp.grad is not None and lc.grad is not None
  torch.autograd.backward([pred, conf], [lp.grad, lc.grad])
  return want, out.detach(), lc.grad


def _same_step(net, hand, loss, depth, want, out):
  assert torch.equal(loss, want) and torch.equal(depth, out)
  have, ref = TG._grads(net), TG._grads(hand)
  for k in ref:
    assert have[k] is not None and ref[k] is not None and torch.equal(have[k], ref[k]), k
  assert all(bool(torch.isfinite(g).all()) for g in have.values())
  for k, b in hand.named_buffers():
    assert torch.equal(dict(net.named_buffers())[k], b), k
  return have


@pytest.mark.gpu
def test_fusion_loss_fine_tunes_through_the_confidence():
  net, maxdisp, maxdepth, H, W = _net(conf_png=False, handoff_grad='full')
  hand = _net(conf_png=False, handoff_grad='full')[0]
  frames, gt = TG._frames(1, H, W, 81, False), TG._gt(1, H, W, maxdepth, 82)
  net.train()
  hand.train()
  loss, depth = net.fusion_loss(frames, gt)
  loss.backward()
  want, out, gconf = _hand(hand, frames, gt, maxdisp, maxdepth, False)
  assert float(gconf.abs().max()) > 0
  have = _same_step(net, hand, loss, depth, want, out)
  # the depth-only module on the same confidence: the same loss, another gradient for stage 1
  depth_net = _net(conf_png=False)[0].train()
  dloss, _ = depth_net.fusion_loss(frames, gt)
  dloss.backward()
  other = TG._grads(depth_net)
  assert torch.equal(dloss, loss)
  differ = [k for k in have if k.startswith('disparity.') and not torch.equal(have[k], other[k])]
  same = [k for k in have if k.startswith('fusion.') and not torch.equal(have[k], other[k])]
  print('%d of %d stage-1 gradients differ from the depth-only module' % (len(differ), sum(k.startswith('disparity.') for k in have)))
  assert differ and not same


@pytest.mark.gpu
def test_fusion_loss_fine_tunes_at_half_size():
  net, maxdisp, maxdepth, H, W = _net(conf_png=False, handoff_grad='full', resize=True)
  hand = _net(conf_png=False, handoff_grad='full', resize=True)[0]
  frames, gt = TG._frames(1, H, W, 71, True), TG._gt(1, H, W, maxdepth, 72)
  net.train()
  hand.train()
  loss, depth = net.fusion_loss(frames, gt)  # (the default module refuses this: tests/test_gpu_handoff_grad.py)
  loss.backward()
  assert tuple(depth.shape) == (1, 1, H // 2, W // 2)
  want, out, gconf = _hand(hand, frames, gt, maxdisp, maxdepth, True)
  assert float(gconf.abs().max()) > 0
  have = _same_step(net, hand, loss, depth, want, out)
  assert any(float(g.abs().max()) > 0 for k, g in have.items() if k.startswith('disparity.'))


@pytest.mark.gpu
def test_the_option_changes_nothing_with_stage_one_frozen():
  full, maxdisp, maxdepth, H, W = _net(conf_png=False, handoff_grad='full')
  plain = _net(conf_png=False)[0]
  frames, gt = TG._frames(1, H, W, 91, False), TG._gt(1, H, W, maxdepth, 92)
  for net in (full, plain):
    net.train()
    net.disparity.eval()
  a, da = full.fusion_loss(frames, gt)
  b, db = plain.fusion_loss(frames, gt)
  a.backward()
  b.backward()
  assert torch.equal(a, b) and torch.equal(da, db)
  ga, gb = TG._grads(full), TG._grads(plain)
  for k in ga:
    assert (ga[k] is None and gb[k] is None) if k.startswith('disparity.') else torch.equal(ga[k], gb[k]), k
  full.eval()
  plain.eval()
  assert torch.equal(full(frames), plain(frames))
