"""The gradient of the multi-view hand-off (mode_multiview_handoff_bwd) and ModeMultiView.fusion_loss, GPU tier.

The kernel is measured against the float64 oracle of tests/handoff_ref.py by DESIGN 4's standing criterion for fp32 kernels: the same
oracle run in float32 by CPU autograd is the yardstick, the kernel's mean error may be at most 2x the yardstick's and its max at most
3x.  The z-buffer's winners are read from the forward's own keys (existing, bit-tested code): winners are discontinuous in the disparity,
and a float64 z-buffer on the CPU differs from the GPU's at a few pixels.  Structural zeros must be +0.0 bit for bit.  fusion_loss is
checked against the hand composition of public pieces with torch.equal: every piece is deterministic."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import handoff_ref as R
import recipe

import models
from dataloader import gpu_ingest
from mode_hip import functional as HF
from models import mode_multiview
from utils import geometry as HG

DEV = 'cuda:0'
SIZES = [(1, 64, 32), (3, 64, 32), (2, 48, 24)]  # plane and key-plane offsets; 1152 pixels = 4.5 blocks: the grid-stride tail
BAND = 1e-3  # left out of the scoring: raw depth this close (relative) to the 1000 clip or (absolute) to 0, winners this close to the cap
FLOOR = 2.0 ** -21  # a plane where the yardstick happens to be exact
TINY = 1e-30


@functools.lru_cache(maxsize=None)
def _case(F, H, W, dbname):
  """Inputs, the forward's winners and both oracles' gradients, computed once per case and shared (nothing below writes to them)."""
  disp, conf = R.inputs(F, H, W, 7 + F + H)
  d, c = disp.to(DEV), conf.to(DEV)
  out, keys = HG.disp2depth_frames_gpu(d, c, dbname, return_keys=True)
  assert keys.dtype == torch.int64 and tuple(keys.shape) == (F, 3, H, W)
  winner, v = R.decode_keys(keys.cpu())
  gout = torch.randn(F, 12, H, W, generator=torch.Generator().manual_seed(11 + F + H))
  gd = gout[:, 0::2].contiguous()
  base = HG._baselines(dbname)
  S = torch.stack([R.slope(disp[:, p], base[p]) for p in range(6)], 1)  # float64
  kink = torch.stack([R.near_kink(disp[:, p], base[p], BAND) for p in range(6)], 1)
  # what the error of an element is measured in: |gout_t| |S| (12, 23-34: t the target a source won), |S| sum_k |w_k gout_tk| (13, 14)
  den = torch.zeros(F, 6, H, W, dtype=torch.float64)
  den[:, 0] = gd[:, 0].double().abs() * S[:, 0].abs()
  won = torch.zeros(F, 3, H * W, dtype=torch.bool)      # sources that won a target
  capped = torch.zeros(F, 3, H * W, dtype=torch.bool)   # ... whose target is capped at 1000 (strictly above, read from the key)
  near_cap = torch.zeros(F, 3, H * W, dtype=torch.bool)
  for f in range(F):
    for p, pair in ((1, '13'), (2, '14')):
      den[f, p] = S[f, p].abs() * R.rotation_adjoint_abs(gd[f, p], pair)
    for k in range(3):
      t = (winner[f, k].reshape(-1) >= 0).nonzero()[:, 0]
      s = winner[f, k].reshape(-1)[t]
      assert s.unique().numel() == s.numel()  # a source wins at most one target
      won[f, k, s] = True
      capped[f, k, s] = v[f, k].reshape(-1)[t] > 1000
      near_cap[f, k, s] = (v[f, k].reshape(-1)[t].double() - 1000).abs() <= BAND * 1000
      den[f, 3 + k].view(-1)[s] = gd[f, 3 + k].reshape(-1)[t].double().abs() * S[f, 3 + k].reshape(-1)[s].abs()
  skip = kink.clone()
  skip[:, 3:] |= near_cap.view(F, 3, H, W) & (S[:, 3:] != 0)  # (a winner without a slope -- d == 0 gives r1 = 1000 -- is zero on either side of the cap)
  ref64 = R.gradient(disp, winner, gd, dbname, torch.float64)
  ref32 = R.gradient(disp, winner, gd, dbname, torch.float32).double()
  return dict(disp=disp, conf=conf, d=d, c=c, keys=keys, out=out, winner=winner, v=v, gout=gout, gd=gd, S=S, kink=kink, den=den, won=won.view(F, 3, H, W),
              capped=capped.view(F, 3, H, W), skip=skip, ref64=ref64, ref32=ref32)


def score(got, z):
  """Per plane (f, p): (mean, max) of |got - float64 oracle| in the units of z['den'], over the pixels that are scored."""
  err = (got.double() - z['ref64']).abs() / (z['den'] + TINY)
  F, _, H, W = err.shape
  rows = {}
  for f in range(F):
    for p in range(6):
      e = err[f, p][~z['skip'][f, p]]
      rows[f, p] = (float(e.mean()), float(e.max()))
  return rows


def assert_within_the_yardstick(got, z, what):
  F = got.shape[0]
  left_out = z['skip'].double().mean((2, 3))
  assert float(left_out.max()) <= 0.005, 'more than 0.5 %% of a plane left out of the scoring: %s' % left_out
  mine, yard = score(got, z), score(z['ref32'], z)
  worst = [0.0, 0.0]
  for key in sorted(mine):
    (m, x), (ym, yx) = mine[key], yard[key]
    print('%s frame %d pair %s: kernel mean %.3e max %.3e; float32 autograd mean %.3e max %.3e; ratios %.2f %.2f' %
          (what, key[0], HG.PAIRS[key[1]], m, x, ym, yx, m / max(ym, TINY), x / max(yx, TINY)))
    worst = [max(worst[0], m / max(ym, FLOOR / 2)), max(worst[1], x / max(yx, FLOOR / 3))]
  print('%s: largest ratio of the means %.3f (bound 2), of the maxima %.3f (bound 3); left out at most %.4f %% of a plane' %
        (what, worst[0], worst[1], 100 * float(left_out.max())))
  for key in sorted(mine):
    (m, x), (ym, yx) = mine[key], yard[key]
    assert m <= max(2 * ym, FLOOR) and x <= max(3 * yx, FLOOR), (what, key, m, x, ym, yx)


def _bwd(z, dbname, depth_only):
  g = (z['gd'] if depth_only else z['gout']).to(DEV)
  return HG.disp2depth_frames_bwd(z['d'], g, z['keys'], dbname, depth_only=depth_only).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('dbname', ['Deep360', 'other'])
@pytest.mark.parametrize('size', SIZES, ids=['x'.join(str(n) for n in s) for s in SIZES])
def test_kernel_against_float64(size, dbname):
  z = _case(*size, dbname)
  both = _bwd(z, dbname, False)
  assert both.shape == z['disp'].shape and both.dtype == torch.float32
  assert_within_the_yardstick(both, z, '%s %s' % (size, dbname))
  depth_only = _bwd(z, dbname, True)
  assert torch.equal(depth_only.view(torch.int32), both.view(torch.int32))  # the other layout reads the same gradients
  # the cases take every branch: zeros, both clips, winners, capped winners and targets nobody reached
  assert bool((z['S'] == 0).any()) and bool((z['S'] != 0).any()) and bool(z['won'].any()) and bool((z['winner'] < 0).any())


@pytest.mark.gpu
@pytest.mark.parametrize('dbname', ['Deep360', 'other'])
@pytest.mark.parametrize('size', SIZES, ids=['x'.join(str(n) for n in s) for s in SIZES])
def test_structural_zeros_are_exact(size, dbname):
  z = _case(*size, dbname)
  g = _bwd(z, dbname, False)
  bits = g.view(torch.int32)
  assert not bool(torch.isnan(g).any())
  sure = ~z['kink']  # off the band both sides agree on which side of a clip a pixel lies
  zero = (z['disp'] == 0) | ((z['S'] == 0) & sure)
  zero[:, 3:] |= ~z['won'] | z['capped']
  assert bool((z['disp'] == 0).any()) and bool(((z['S'] == 0) & (z['disp'] != 0)).any()) and bool(zero[:, 3:].any())
  assert bool((bits[zero] == 0).all()), 'a structural zero is not +0.0: %d of %d' % (int((bits[zero] != 0).sum()), int(zero.sum()))
  # planes 23, 24, 34: exactly the uncapped winners whose sine rule passes a gradient are not zero (counted off the band, where that is decidable)
  live = z['won'] & ~z['capped'] & (z['S'][:, 3:] != 0)
  assert int(((g[:, 3:] != 0) & sure[:, 3:]).sum()) == int((live & sure[:, 3:]).sum())
  if not bool((z['kink'][:, 3:] & z['won']).any()):
    assert int((g[:, 3:] != 0).sum()) == int(live.sum())
  print('%s %s: %d structural zeros, %d live winners of %d targets with a winner, %d capped' %
        (size, dbname, int(zero.sum()), int(live.sum()), int(z['won'].sum()), int(z['capped'].sum())))


@pytest.mark.gpu
def test_repeatable_independent_and_wired_into_autograd():
  F, H, W = 2, 48, 24
  z = _case(F, H, W, 'Deep360')
  first = _bwd(z, 'Deep360', False)
  assert torch.equal(_bwd(z, 'Deep360', False).view(torch.int32), first.view(torch.int32))
  # frame 1 a copy of frame 0: frame 0 of the F = 2 call is the F = 1 call (plane and key-plane offsets)
  d1, c1, g1 = z['d'][:1], z['c'][:1], z['gout'][:1].to(DEV)
  d2, c2, g2 = torch.cat((d1, d1)), torch.cat((c1, c1)), torch.cat((g1, g1))
  out1, k1 = HG.disp2depth_frames_gpu(d1, c1, return_keys=True)
  out2, k2 = HG.disp2depth_frames_gpu(d2, c2, return_keys=True)
  one, two = HG.disp2depth_frames_bwd(d1, g1, k1), HG.disp2depth_frames_bwd(d2, g2, k2)
  assert torch.equal(two[0], two[1]) and torch.equal(two[:1], one) and torch.equal(one.cpu(), first[:1])
  # autograd returns the entry's result, for every layout of the input, and nothing for the confidence
  for kw in ({}, {'conf_png': True}, {'depth_only': True}):
    d = z['d'].clone().requires_grad_(True)
    c = z['c'].clone().requires_grad_(True)
    out = HG.disp2depth_frames_gpu(d, c, **kw)
    assert out.requires_grad and torch.equal(out, HG.disp2depth_frames_gpu(z['d'], z['c'], **kw))
    g = (z['gd'] if kw.get('depth_only') else z['gout']).to(DEV)
    gd, gc = torch.autograd.grad(out, (d, c), g, allow_unused=True)
    assert gc is None and torch.equal(gd.cpu().view(torch.int32), first.view(torch.int32))
  flat = z['d'].view(6 * F, 1, H, W).clone().requires_grad_(True)
  out = HG.disp2depth_frames_gpu(flat, z['c'])
  gflat, = torch.autograd.grad(out, flat, z['gout'].to(DEV))
  assert gflat.shape == flat.shape and torch.equal(gflat.view(F, 6, H, W).cpu(), first)
  c = z['c'].clone().requires_grad_(True)
  only_conf = HG.disp2depth_frames_gpu(z['d'], c)
  assert torch.equal(only_conf, z['out']) and torch.autograd.grad(only_conf.sum(), c, allow_unused=True) == (None,)
  # without a gradient the call is today's: same bits, with and without the keys, and no graph
  plain = HG.disp2depth_frames_gpu(z['d'], z['c'])
  plain_k, keys = HG.disp2depth_frames_gpu(z['d'], z['c'], return_keys=True)
  assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, z['out']) and torch.equal(plain_k, z['out'])
  assert torch.equal(keys, z['keys']) and not keys.requires_grad
  with torch.no_grad():
    quiet = HG.disp2depth_frames_gpu(z['d'].clone().requires_grad_(True), z['c'])
  assert quiet.grad_fn is None and torch.equal(quiet, z['out'])


# ------------------------------------------------------------------------------------------------ fusion_loss
def _disparity_state(name):
  z = np.load(os.path.join(recipe.HERE, name))
  sd = recipe.fixture_state(z)
  for k in z.files:
    if k.startswith('bn/'):
      sd[k[3:]] = torch.from_numpy(z[k]).clone()
  maxdisp, H, W = [int(v) for v in z['cfg'][:3]]
  return maxdisp, H, W, sd


def _tiny_net(resize=False):
  """The tiny net of tests/test_gpu_multiview.py: model_wc_tiny's disparity state and fusion_tiny's recipe state (64 x 32, 16 disparities)."""
  maxdisp, H, W, sd = _disparity_state('model_wc_tiny.npz')
  zf = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'))
  cfg = zf['cfg']
  maxdepth, seed, channels = float(cfg[0]), int(cfg[4]), tuple(int(c) for c in cfg[5:])
  manifest = [(k, tuple(s)) for k, s in json.loads(str(zf['manifest']))]
  net = models.ModeMultiView(maxdisp, maxdepth, H, W, channels=channels, resize=resize)
  net.disparity.load_state_dict(sd)
  net.fusion.load_state_dict(recipe.recipe_state(manifest, seed))
  return net.to(DEV), maxdisp, maxdepth, H, W


def _frames(F, H, W, seed, u8):
  if u8:
    return torch.randint(0, 256, (F, 12, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)
  left, right = recipe.recipe_images(6 * F, H, W, seed)
  return torch.stack((left.view(F, 6, 3, H, W), right.view(F, 6, 3, H, W)), dim=2).reshape(F, 12, 3, H, W).to(DEV)


def _gt(F, H, W, maxdepth, seed):
  """Ground truth between 0 and 1.25 maxdepth: a fifth of it beyond the mask gt <= maxdepth."""
  return (torch.rand(F, H, W, generator=torch.Generator().manual_seed(seed)) * 1.25 * maxdepth).to(DEV)


def _rgb_of(frames):
  if frames.dtype == torch.uint8:
    return gpu_ingest.frames_u8_gpu(frames.contiguous())[2]
  return mode_multiview.split_frames(frames)[2]


def _grads(module):
  return {k: (None if p.grad is None else p.grad.clone()) for k, p in module.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize('u8', [False, True], ids=['float', 'uint8'])
@pytest.mark.parametrize('F', [1, 2])
def test_fusion_loss_with_stage_one_frozen(F, u8):
  """net.train(); net.disparity.eval(): the loss and every fusion gradient of the hand composition of public pieces, bit for bit."""
  net, maxdisp, maxdepth, H, W = _tiny_net()
  hand, _, _, _, _ = _tiny_net()
  frames, gt = _frames(F, H, W, 51 + F, u8), _gt(F, H, W, maxdepth, 61 + F)
  hand.eval()
  _, st = hand(frames, return_stages=True)
  hand.fusion.train()
  out = hand.fusion.feature_extraction(st['fusion_input'], _rgb_of(frames))
  want = HF.silog_loss(out, gt, gt <= maxdepth, 0.5)
  want.backward()
  net.train()
  net.disparity.eval()
  loss, depth = net.fusion_loss(frames, gt)
  assert loss.dim() == 0 and bool(torch.isfinite(loss)) and torch.equal(loss, want)
  assert not depth.requires_grad and torch.equal(depth, out.detach())
  loss.backward()
  have, ref = _grads(net), _grads(hand)
  for k in ref:
    if k.startswith('disparity.'):
      assert have[k] is None, k
    else:
      assert have[k] is not None and torch.equal(have[k], ref[k]), k
  assert any(float(g.abs().max()) > 0 for k, g in have.items() if g is not None)
  for k, b in hand.named_buffers():
    assert torch.equal(dict(net.named_buffers())[k], b), k
  other, _ = net.fusion_loss(frames, gt, lamda=0.85, maxdepth=0.5 * maxdepth)
  assert torch.equal(other, HF.silog_loss(net.fusion.feature_extraction(st['fusion_input'], _rgb_of(frames)), gt, gt <= 0.5 * maxdepth, 0.85))


@pytest.mark.gpu
def test_fusion_loss_at_half_size():
  """resize=True as Deep360DatasetFusion(resize=True, training=True): decimated hand-off, halved 8-bit RGB, gt[:, ::2, ::2], no upsampling."""
  net, maxdisp, maxdepth, H, W = _tiny_net(resize=True)
  hand, _, _, _, _ = _tiny_net(resize=True)
  frames, gt = _frames(1, H, W, 71, True), _gt(1, H, W, maxdepth, 72)
  hand.eval()
  _, st = hand(frames, return_stages=True)
  assert tuple(st['fusion_input'].shape) == (1, 12, H // 2, W // 2)
  hand.fusion.train()
  out = hand.fusion.feature_extraction(st['fusion_input'], st['rgb'])
  half = gt[:, ::2, ::2]
  want = HF.silog_loss(out, half, half <= maxdepth, 0.5)
  net.train()
  net.disparity.eval()
  loss, depth = net.fusion_loss(frames, gt)
  assert torch.equal(loss, want) and tuple(depth.shape) == (1, 1, H // 2, W // 2) and torch.equal(depth, out.detach())
  with pytest.raises(ValueError):
    net.fusion_loss(_frames(1, H, W, 73, False), gt)  # halving needs the 8-bit frames
  net.disparity.train()
  with pytest.raises(ValueError, match='no backward'):
    net.fusion_loss(frames, gt)


@pytest.mark.gpu
def test_fusion_loss_fine_tunes_the_disparity_stage():
  """net.train(): the gradient of the loss reaches every stage-1 parameter through the hand-off's backward, and equals the two-step
  composition: stage 1 alone, the rest on a detached leaf, then pred.backward(leaf.grad)."""
  net, maxdisp, maxdepth, H, W = _tiny_net()
  hand, _, _, _, _ = _tiny_net()
  F = 1
  frames, gt = _frames(F, H, W, 81, False), _gt(F, H, W, maxdepth, 82)
  net.train()
  with pytest.raises(RuntimeError, match='inference only'):
    net(frames)
  loss, depth = net.fusion_loss(frames, gt)
  loss.backward()
  have = _grads(net)
  assert all(g is not None and bool(torch.isfinite(g).all()) for g in have.values()), [k for k, g in have.items() if g is None]
  assert any(float(g.abs().max()) > 0 for k, g in have.items() if k.startswith('disparity.'))
  hand.train()
  left, right, rgb = mode_multiview.split_frames(frames)
  size = (maxdisp, H, W)
  cost3 = hand.disparity._logits(left, right)[2]
  pred = HF.head(cost3, size)
  conf = HF.head_fwd(cost3.detach(), size, with_confidence=True)[1]
  leaf = pred.detach().requires_grad_(True)
  out = hand.fusion.feature_extraction(HG.disp2depth_frames_gpu(leaf, conf, conf_png=True), rgb)
  want = HF.silog_loss(out, gt, gt <= maxdepth, 0.5)
  want.backward()
  assert leaf.grad is not None and float(leaf.grad.abs().max()) > 0
  pred.backward(leaf.grad)
  assert torch.equal(loss, want) and torch.equal(depth, out.detach())
  ref = _grads(hand)
  for k in ref:
    assert torch.equal(have[k], ref[k]), k
  for k, b in hand.named_buffers():
    assert torch.equal(dict(net.named_buffers())[k], b), k
  net.fusion.eval()
  with pytest.raises(RuntimeError, match='fusion_loss'):
    net.fusion_loss(frames, gt)
